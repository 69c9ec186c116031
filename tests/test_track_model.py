"""Known answers of tests/track_model.py, the specification of the device tracker, that need no cv2: worked by hand or true by construction."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_model as tm  # noqa: E402


def texture(h, w, dx=0, dy=0):
    """Band-limited: the shortest period is 2 pi / 0.45 = 14 pixels, so the 21-pixel window sees unambiguous structure and a shift of 6
    pixels stays within the top pyramid level's reach."""
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x - dx, y - dy
    v = 128 + 40 * np.sin(x * 0.31 + 0.2) * np.cos(y * 0.23) + 35 * np.sin(x * 0.13 + y * 0.19 + 1) + 30 * np.cos(x * 0.07 - y * 0.11) + \
        15 * np.sin(x * 0.45 - y * 0.4)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


@pytest.mark.parametrize('base,peak', [(50, 200), (200, 60), (0, 255), (100, 111)])
def test_a_lone_pixel_is_one_corner_with_score_difference_minus_one(base, peak):
    img = np.full((15, 15), base, np.uint8)
    img[7, 8] = peak
    corners = tm.fast_corners(img)
    assert corners.dtype == np.float32 and corners.tolist() == [[8.0, 7.0]]
    scores = tm.fast_scores(img)
    assert scores[7, 8] == abs(peak - base) - 1 and np.count_nonzero(scores) == 1


def test_a_difference_at_the_threshold_is_no_corner():
    img = np.full((15, 15), 100, np.uint8)
    img[7, 7] = 110                                       # brighter than p + t must be STRICT
    assert len(tm.fast_corners(img)) == 0
    assert len(tm.fast_corners(img, threshold=9)) == 1


def test_step_edge_constant_and_small_images_have_no_corners():
    edge = np.full((20, 24), 30, np.uint8)
    edge[:, 12:] = 220                                    # at most 8 contiguous circle pixels lie across a straight edge
    assert tm.fast_corners(edge).shape == (0, 2)
    assert len(tm.fast_corners(edge.T.copy())) == 0
    assert len(tm.fast_corners(np.full((20, 24), 99, np.uint8))) == 0
    assert len(tm.fast_corners(np.arange(36, dtype=np.uint8).reshape(6, 6) * 7)) == 0
    noise = ((np.arange(6 * 40).reshape(6, 40) * 2654435761) >> 7).astype(np.uint8)
    assert len(tm.fast_corners(noise)) == 0 and len(tm.fast_corners(noise.T.copy())) == 0


def test_the_corner_of_a_bright_quadrant_is_exactly_one_corner():
    """The quadrant fades away from its corner, so the corner pixel has the one largest score.  (On an ideal two-level quadrant the corner
    pixel and its diagonal neighbour score the same, and cv2's strict comparison suppresses both: asserted below as well.)"""
    img = np.full((24, 24), 20, np.uint8)
    y, x = np.mgrid[0:12, 0:12]
    img[12:, 12:] = 220 - 4 * (x + y)
    assert tm.fast_corners(img).tolist() == [[12.0, 12.0]]
    assert tm.fast_scores(img)[12, 12] == 199
    img[12:, 12:] = 220
    assert tm.fast_scores(img)[12, 12] == tm.fast_scores(img)[13, 13] == 199 and len(tm.fast_corners(img)) == 0
    assert np.count_nonzero(tm.fast_scores(img)) >= 1     # (several pixels around it are corners before the suppression)


def test_corners_come_in_row_major_order_and_keep_off_the_edges():
    img = np.full((30, 40), 10, np.uint8)
    for x, y in ((30, 4), (5, 4), (3, 3), (36, 26), (20, 15), (2, 15), (20, 27)):
        img[y, x] = 250
    assert tm.fast_corners(img).tolist() == [[3, 3], [5, 4], [30, 4], [20, 15], [36, 26]]       # (2, 15) and (20, 27) are within 3 of an edge


def test_pyr_down_of_a_constant_and_sizes():
    for h, w in ((5, 5), (9, 7), (22, 23), (1, 6), (6, 1), (2, 2)):
        out = tm.pyr_down(np.full((h, w), 77, np.uint8))
        assert out.shape == ((h + 1) // 2, (w + 1) // 2) and (out == 77).all()


def test_pyr_down_5x5_by_hand():
    img = np.array([[10, 20, 30, 40, 50], [60, 70, 80, 90, 100], [110, 120, 130, 140, 150], [160, 170, 180, 190, 200],
                    [210, 220, 230, 240, 250]], np.uint8)
    # reflect-101: index -2 -> 2, -1 -> 1, 5 -> 3, 6 -> 2.  The image is 50 r + 10 c + 10, linear in r and c, and the kernel is symmetric, so
    # with a reflected border: horizontal pass at c = 0 -> taps c = (2, 1, 0, 1, 2) weights (1, 4, 6, 4, 1): mean column = 12/16; c = 2 -> 2;
    # c = 4 -> taps (2, 3, 4, 3, 2): 52/16.  Same for rows.  value = 50 r' + 10 c' + 10 exactly, (sum + 128) >> 8 rounds to nearest.
    eff = np.array([12 / 16, 2.0, 52 / 16])
    want = np.floor(50 * eff[:, None] + 10 * eff[None, :] + 10 + 0.5).astype(np.uint8)
    assert np.array_equal(tm.pyr_down(img), want)
    assert want.tolist() == [[55, 68, 80], [118, 130, 143], [180, 193, 205]]


def test_pyramid_stops_where_cv2_does():
    assert tm.num_levels(640, 480) == 3
    assert tm.num_levels(48, 40) == 0                     # 24 x 20: 20 <= 21
    assert tm.num_levels(44, 44) == 1                     # 22 x 22 is larger than the window, 11 x 11 is not
    assert tm.num_levels(42, 100) == 0
    assert tm.num_levels(200, 180) == 3 and tm.num_levels(100, 90) == 2 and tm.num_levels(67, 180) == 1
    assert [l.shape for l in tm.build_pyramid(np.zeros((90, 100), np.uint8))] == [(90, 100), (45, 50), (23, 25)]


def test_scharr_of_ramps():
    for slope in (1, 3, 7):
        ramp = (np.arange(12)[None, :] * slope + np.zeros((9, 1))).astype(np.uint8)
        ix, iy = tm.scharr(ramp)
        assert ix.dtype == np.int16 and (ix[:, 1:-1] == 32 * slope).all() and (ix[:, 0] == 0).all() and (ix[:, -1] == 0).all() and (iy == 0).all()
        ix, iy = tm.scharr(ramp.T.copy())
        assert (iy[1:-1] == 32 * slope).all() and (iy[0] == 0).all() and (ix == 0).all()
    ix, iy = tm.scharr(np.array([[9]], np.uint8))
    assert ix.tolist() == [[0]] and iy.tolist() == [[0]]


SHIFTS = [(6, -6), (-6, 6), (-3, 5), (1, 0), (0, -1), (4, 4), (-5, -2), (0, 0)]


@pytest.mark.parametrize('dx,dy', SHIFTS)
def test_lk_recovers_integer_shifts(dx, dy):
    early, late = texture(120, 160), texture(120, 160, dx, dy)
    ys, xs = np.mgrid[30:91:12, 30:131:12]
    points = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
    moved, found = tm.lk_track(early, late, points)
    assert moved.dtype == np.float32 and found.dtype == np.uint8 and found.all()
    error = np.abs(moved - points - np.float32([dx, dy])).max()
    assert error < 0.5, error                             # the only tolerance that tells integer shifts apart (the model: below 0.01)


def test_lk_rejects_a_flat_patch_and_loses_what_leaves_the_image():
    early, late = texture(120, 160), texture(120, 160, 1, 1)
    early[40:90, 60:120] = 77
    late[40:90, 60:120] = 77
    points = np.float32([[90, 65], [20, 20], [-12.5, 30], [171, 30], [30, -11.5], [30, 131], [0, 0], [159, 119]])
    moved, found = tm.lk_track(early, late, points)
    assert found.tolist() == [0, 1, 0, 0, 0, 0, 1, 1]     # flat: minEig; inside; four whose window lies outside; the corner pixels are inside
    late_gone = texture(120, 160, -40, 0)
    moved, found = tm.lk_track(early, late_gone, np.float32([[3, 60]]))
    assert moved.shape == (1, 2) and found.shape == (1,)
    assert tm.lk_track(early, late, np.zeros((0, 2), np.float32))[0].shape == (0, 2)


def test_subframes_follow_the_reference_order():
    assert tm.subframes(61, 37, 2, 2) == [(0, 0, 31, 19), (0, 19, 31, 18), (31, 0, 30, 19), (31, 19, 30, 18)]
    assert len(tm.subframes(9, 9, 4, 4)) == 9             # ceil(9 / 4) = 3: three columns and rows, not four
    early, late = texture(80, 96), texture(80, 96, 2, -1)
    parts = tm.track_subframes(early, late, 2, 2, max_per_subframe=5)
    assert len(parts) == 4 and all(len(c) <= 5 and len(c) == len(m) == len(f) for c, _, m, f in parts)
    feats = tm.track_pair_features(early, late, 2, 2, min_features=10 ** 6)
    assert feats == []
