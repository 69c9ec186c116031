"""Every case of tests/track_edge_cases.py reaches the path it is named for -- asserted with the models alone (tests/track_model.py,
tests/ransac_model.py), before tests/test_gpu_track_edges.py looks at a kernel's result.  The figures are the models' on these inputs; a
case whose condition fails needs another seed, never a weaker condition."""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_model as rm  # noqa: E402
import track_edge_cases as ec  # noqa: E402
import track_model as tm  # noqa: E402
from tracker_clip import model_corners, model_lk  # noqa: E402


# ---- a. more than 64 rows -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(ec.tall_cases()))
def test_tall_frames_fill_the_rounds_they_name(name):
    """Corners per band of 64 rows: every round of the compaction holds some (or none, where the case says so), and every capacity below
    the count cuts strictly inside the round named for it -- or, for ('fills', r), exactly at the end of round r with corners still to come."""
    img, bands, runs = ec.tall_cases()[name]
    assert img.shape[0] > ec.ROUND and ec.band_counts(img) == bands
    total, ends = sum(bands), np.cumsum(bands).tolist()
    for rows, cols, max_per, where in runs:
        subs = tm.subframes(img.shape[1], img.shape[0], rows, cols)
        if (rows, cols) != (1, 1):                                       # cut into columns: every sub-frame still has every round
            assert where is None
            for left, top, w, h in subs:
                part = ec.band_counts(np.ascontiguousarray(img[top:top + h, left:left + w]))
                assert h == img.shape[0] and len(part) == len(bands) and min(part) > 0 and sum(part) <= max_per, (name, part)
            assert len({w for _, _, w, _ in subs}) > 1                   # unequal widths
        elif where is None:
            assert max_per >= total
        elif isinstance(where, tuple):
            assert where[0] == 'fills' and max_per == ends[where[1]] < total
        else:
            assert where >= 1 and bands[where] > 0 and ends[where - 1] < max_per < ends[where], (name, max_per, ends)


def test_tall_cases_cover_the_rounds_the_issue_lists():
    cases = ec.tall_cases()
    assert [run[2:] for run in cases['noise 40 x 150'][2]] == [(1024, None), (300, 1), (216, ('fills', 0)), (460, 2)]
    assert cases['gap 40 x 200'][1][1] == 0 and cases['gap 40 x 200'][1][2] > 0          # a whole round with no corner, then corners again
    assert len(cases['wide 61 x 200'][1]) == 4 and cases['wide 61 x 200'][0].shape[1] % 4 == 1
    stack = ec.tall_stack()
    assert len(tm.fast_corners(stack[0])) > 0 and len(tm.fast_corners(stack[1])) == 0


# ---- b. thresholds, the largest score, ties -----------------------------------------------------------------------------------------------

def test_thresholds_change_the_corner_set():
    img = ec.threshold_frame()
    assert {t: len(tm.fast_corners(img, t)) for t in ec.THRESHOLDS} == ec.THRESHOLDS
    assert len(set(ec.THRESHOLDS.values())) == len(ec.THRESHOLDS)        # no two thresholds can be mistaken for each other


def test_binary_frames_score_the_maximum_and_tie():
    img = ec.binary_frame()
    s = tm.fast_scores(img)
    assert set(np.unique(img).tolist()) == {0, 255}
    assert (len(tm.fast_corners(img)), int(s.max()), int(np.count_nonzero(s)), ec.tie_pairs(img)) == (31, 254, 33, 1)
    blocks = ec.binary_frame(3)
    s = tm.fast_scores(blocks)
    assert (len(tm.fast_corners(blocks)), int(s.max()), int(np.count_nonzero(s)), ec.tie_pairs(blocks)) == (15, 254, 412, 612)
    assert model_corners(blocks, 2, 2, 256)[1].tolist() == [2, 1, 4, 7]
    # four scores of 254 side by side in one row, word-aligned: 0xFEFEFEFE in the kernel's packed scores
    row = (s == 254)
    quad = row[:, 0:-3] & row[:, 1:-2] & row[:, 2:-1] & row[:, 3:]
    assert quad[:, ::4].any()


@pytest.mark.parametrize('corner', ec.QUADRANT_CORNERS)
def test_quadrant_ties_straddle_a_tile_edge(corner):
    x, y = corner
    img = ec.quadrant(x, y)
    s = tm.fast_scores(img)
    assert s[y, x] == s[y + 1, x + 1] == 199 and len(tm.fast_corners(img)) == 0 and ec.tie_pairs(img) >= 1
    assert (x // 56 != (x + 1) // 56) or (y // 14 != (y + 1) // 14)       # the two tied pixels are decided by different FAST tiles


# ---- c. fewer sub-frames than asked for ---------------------------------------------------------------------------------------------------

def test_fewer_subframes_than_asked_for():
    W, H, rows, cols = ec.FEWER
    subs = tm.subframes(W, H, rows, cols)
    assert len(subs) == 49 < rows * cols and all((w, h) == (7, 7) for _, _, w, h in subs)
    sets = ec.fewer_lit_sets()
    assert sets[0].astype(int).tolist() == [1, 0] * 24 + [1]
    for lit in sets:
        assert model_corners(ec.fewer_frame(lit), rows, cols, 4)[1].tolist() == lit.astype(int).tolist()
    assert len({lit.tobytes() for lit in sets}) == 3


# ---- d. unequal pyramid depths ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(ec.MIXED))
def test_mixed_depth_launches_track_points_at_every_depth(name):
    size, _, _, want_depths = ec.MIXED[name]
    assert ec.depths(size, size, 2, 2) == want_depths and len(set(want_depths)) == 2
    early, late = ec.mixed_pair(name)
    want_counts = {'169 x 169': [124, 147, 162, 135], '85 x 85': [34, 35, 16, 23]}[name]
    for a, b, counts_are in ((early, late, want_counts), (late, early, None)):
        points, counts, _ = model_corners(a, 2, 2, ec.MIXED_MAX_PER)
        moved, found = model_lk(a, b, 2, 2, points, counts)
        assert counts_are is None or counts.tolist() == counts_are
        assert found.sum(axis=1).min() >= 10, (name, found.sum(axis=1))
        if counts_are is not None:
            assert found.sum(axis=1).tolist() == [min(c, ec.MIXED_MAX_PER) for c in counts_are]


def test_depth_three_pipeline_frame():
    early, late = ec.depth_pair()
    assert early.shape == (180, 200) and ec.depths(200, 180, 1, 1) == [3]
    points, counts, status = model_corners(early, 1, 1, ec.MIXED_MAX_PER)
    assert counts.tolist() == [412] and status.tolist() == [1] and ec.band_counts(early) == [162, 134, 116]
    assert model_lk(early, late, 1, 1, points, counts)[1].sum() == 64


# ---- e. steep gradients -------------------------------------------------------------------------------------------------------------------

def test_steep_frames_stay_finite_and_reach_large_sums():
    points = ec.steep_points()
    assert len(points) == 80
    largest = {}
    for name, early, late in ec.steep_pairs():
        assert early.shape == late.shape == (40, 48) and set(np.unique(early).tolist()) == {0, 255}
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            moved, found = tm.lk_track(early, late, points)
        assert np.isfinite(moved).all()
        largest[name] = int(np.abs(ec.raw_window_sums(early, points)[:, 0]).max())
        if name.endswith('1 px'):
            assert found.all()
    # sum Ix Ix over a window, before FLT_SCALE: far above 2^24, where float32 stops being exact (the smooth cases stay below it)
    assert largest == {'pixels, 1 px': 996817019, 'blocks, 1 px': 1774461552, 'blocks, 6 px': 1774461552}
    assert min(largest.values()) > 1 << 24
    moved, _ = tm.lk_track(*ec.steep_pairs()[2][1:], points)
    assert np.abs(moved - points).max() > 6.5                            # the six-pixel pair: tracks travel


def test_checkerboard_sums_pass_two_to_the_31():
    """Beyond what the issue asks: window sums that no int32 holds, so the 64-lane reduction must be the int64 one the kernel's header
    promises.  (Per lane, 7 x 2,550^2 is far below 2^31.)"""
    early, late, points = ec.checker_pair()
    assert np.array_equal(points, np.rint(points)) and len(points) == 80
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        moved, found = tm.lk_track(early, late, points)
    assert np.isfinite(moved).all() and found.all()
    sums = np.abs(ec.raw_window_sums(early, points))
    assert sums.max(axis=0).tolist() == [2830668300, 113403600, 3150071100]
    assert int((sums[:, [0, 2]].max(axis=1) > 1 << 31).sum()) == 44
    assert np.abs(moved - points - np.float32([1, 0])).max() < 0.5       # and the model still tracks the one-pixel shift there


# ---- f. second trips of the gather's lane strides -----------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def stride_models():
    return {name: rm.ransac_inliers(*ec.stride_launch(name)) for name in ec.STRIDE_LAUNCHES}


@pytest.mark.parametrize('name', list(ec.STRIDE_LAUNCHES))
def test_stride_launches_make_second_trips(name, stride_models):
    from meshflow_amd import ops
    n, S, (W, H, rows, cols) = ec.STRIDE_LAUNCHES[name]
    grid = ops.track_subframe_grid(W, H, rows, cols)
    assert grid[2] * grid[3] == S and max(n, S) > 64 and 2 * n * S <= 65535
    points, counts, moved, found = ec.stride_launch(name)
    assert counts.reshape(-1).tolist() == [ec.STRIDE_K[i % 6] for i in range(n * S)]
    inlier, info = stride_models[name]
    assert int(inlier.sum()) == ec.STRIDE_SURVIVORS
    for min_features in ec.STRIDE_MIN_FEATURES:
        early, late, offsets, status = rm.gather(points, moved, inlier, info, grid, min_features)
        assert len(early) == offsets[-1] > 0
        if n > 64 and min_features >= 20:                                # flagged and kept pairs on both sides of pair 64
            flagged = status == rm.PAIR_TOO_FEW
            assert flagged[:64].any() and flagged[64:].any() and (~flagged[:64]).any() and (~flagged[64:]).any()
            kept = info[:, :, 2].sum(axis=1)
            assert sorted(set(kept.tolist())) == [0, 20, 23]
            # at 21 the pairs in front of pair 64 that fall below the minimum hold survivors: `before` must leave those out
            assert ((kept > 0) & flagged)[:64].any() == (min_features == 21)
