"""`ops.lk_track` judged as if no model existed: against the float64 textbook tracker and the analytic truth of tests/lk_second_opinion.py,
with the three assertions of tests/test_lk_second_opinion.py on every judged point -- found, within 0.01 pixel of the textbook's fixed
point, and no further from the truth than the fixed point is plus 0.01.  (That the kernel equals the model bit for bit is
tests/test_gpu_track.py's business, not this file's: nothing here imports the model.)  The textbook runs on the CPU, once per scene; each
sub-frame is an image of its own with coordinates relative to it.

End to end, `DeviceTracker.track_clip` on four 128 x 96 frames cut from one homography scene: the transfer error of each fitted homography
at the four frame corners, against the truth, must not exceed that of the textbook pipeline (the same corners from
`track_definition.fast_corners`, `textbook_lk`, the host finisher) by more than 0.01 x L.  L is the largest corner leverage of the
least-squares fit, from the textbook's own tracks: each track may differ by 0.01 pixel, a corner moves by J_k d_k summed over the tracks,
so by at most 0.01 x sum_k ||J_k||, J_k the 2 x 2 derivative of the corner's image by track k's late position (to first order; taken by
central differences of `host.lsq_homography` itself).  Measured on the CPU: L = 5.00, 5.27 and 4.46 on the three pairs, from 145, 168 and
167 tracks; the device's excess over the textbook pipeline was at most 0.0003 pixel (profiles/tracker.md).  Both pipelines take their
tracks through the same outlier step, so the two fits see the same set wherever the trackers agree."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lk_second_opinion as so  # noqa: E402
import track_definition as td  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def judge_launch(dev, pairs, rows, cols, what):
    """ONE `ops.lk_track` launch: `pairs` = [(early, late, [a Reference per sub-frame, or None for a sub-frame without points])]."""
    import torch
    from meshflow_amd import ops
    h, w = pairs[0][0].shape
    sub_w, sub_h, grid_cols, grid_rows = ops.track_subframe_grid(w, h, rows, cols)
    rects = so.subframes(w, h, rows, cols)
    assert len(rects) == grid_cols * grid_rows and rects[-1][:2] == ((grid_cols - 1) * sub_w, (grid_rows - 1) * sub_h)
    most = max(len(ref.points) for _, _, refs in pairs for ref in refs if ref is not None)
    points = np.zeros((len(pairs), len(rects), most, 2), np.float32)
    counts = np.zeros((len(pairs), len(rects)), np.int32)
    for i, (early, late, refs) in enumerate(pairs):
        assert len(refs) == len(rects)
        for s, (ref, (left, top, sw, sh)) in enumerate(zip(refs, rects)):
            if ref is not None:
                assert np.array_equal(ref.early, early[top:top + sh, left:left + sw]) and np.array_equal(ref.points, ref.points.astype(np.float32))
                points[i, s, :len(ref.points)], counts[i, s] = ref.points, len(ref.points)
    moved, found = ops.lk_track(torch.from_numpy(np.stack([p[0] for p in pairs])).to(dev), torch.from_numpy(np.stack([p[1] for p in pairs])).to(dev),
                                torch.from_numpy(points).to(dev), torch.from_numpy(counts).to(dev), rows, cols)
    moved, found = moved.cpu().numpy(), found.cpu().numpy()
    assert moved.shape == points.shape and moved.dtype == np.float32 and found.shape == counts.shape + (most,) and found.dtype == np.uint8
    judged = 0
    for i, (_, _, refs) in enumerate(pairs):
        for s, ref in enumerate(refs):
            k = int(counts[i, s])
            assert not moved[i, s, k:].any() and not found[i, s, k:].any(), (what, i, s)           # zeros behind a sub-frame's points
            if ref is not None:
                so.assert_verdict(ref, moved[i, s, :k], found[i, s, :k], '%s pair %d sub-frame %d' % (what, i, s))
                judged += int(ref.judged.sum())
    return judged


def one_subframe(name):
    early, late, _, _ = so.case_scene(name)
    return early, late, [so.case_reference(name)]


@pytest.mark.parametrize('name', so.CASES)
def test_every_table_case_as_one_subframe(dev, name):
    ref = so.case_reference(name)
    assert judge_launch(dev, [one_subframe(name)], 1, 1, name) >= 0.9 * len(ref.points)


@pytest.mark.parametrize('name', so.TWO_BY_TWO)
def test_two_by_two_subframes(dev, name):
    """180 x 200 as four 90 x 100 sub-frames (pyramid depth 2 instead of 3); 61 x 45 as 31 x 23, 31 x 22, 30 x 23 and 30 x 22: unequal
    sizes, an odd left, depth 0 and a window as high as the image -- every point's window crosses two borders there."""
    early, late, _, _ = so.case_scene(name)
    refs = so.subframe_references(name, 2, 2)
    assert len(refs) == 4 and len({ref.early.shape for ref in refs}) == (4 if name.startswith('61x45') else 1)
    judged = judge_launch(dev, [(early, late, list(refs))], 2, 2, name)
    assert judged >= 0.5 * sum(len(ref.points) for ref in refs), judged


def test_three_pairs_with_different_motions_in_one_launch(dev):
    names = so.THREE_MOTIONS
    assert judge_launch(dev, [one_subframe(n) for n in names], 1, 1, 'three pairs') > 400
    mixed = [(so.case_scene(n)[0], so.case_scene(n)[1], list(so.subframe_references(n, 2, 2))) for n in names]
    assert judge_launch(dev, mixed, 2, 2, 'three pairs, 2 x 2') > 100


def test_a_subframe_without_points_between_two_full_ones(dev):
    """180 x 200 as three 60 x 200 sub-frames, the middle one with a count of 0: its slots stay zero, its neighbours are judged as ever."""
    name = so.EMPTY_MIDDLE
    early, late, _, _ = so.case_scene(name)
    refs = list(so.subframe_references(name, 1, 3))
    assert len(refs) == 3
    refs[1] = None
    assert judge_launch(dev, [(early, late, refs)], 1, 3, 'empty middle') > 200


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------

FRAME_W, FRAME_H, CUT_LEFT, CUT_TOP, SCENE_W, SCENE_H = 128, 96, 16, 12, 160, 120
MAX_PER, MIN_FEATURES = 128, 4
CORNERS = np.array([[0.0, 0.0], [FRAME_W - 1.0, 0.0], [0.0, FRAME_H - 1.0], [FRAME_W - 1.0, FRAME_H - 1.0]])


@functools.lru_cache(maxsize=None)
def clip_and_truth():
    """Frame t is the 160 x 120 scene moved t times by one homography, cut at (16, 12): every adjacent pair has the same true motion."""
    step = so.TABLE['180x200-homography'][1]
    frames = np.stack([so.scene(SCENE_H, SCENE_W, np.linalg.matrix_power(step, t))[1][CUT_TOP:CUT_TOP + FRAME_H, CUT_LEFT:CUT_LEFT + FRAME_W]
                       for t in range(4)])
    cut = so.as_homography((-CUT_LEFT, -CUT_TOP))
    return np.ascontiguousarray(frames), cut @ step @ np.linalg.inv(cut)


def corner_leverage(early, late):
    """(4,) sum over the tracks of the spectral norm of d corner / d late_k for `host.lsq_homography`, by central differences."""
    from meshflow_amd import host
    early, late = early.reshape(-1, 2), late.reshape(-1, 2)
    eps = 1e-4
    jac = np.zeros((len(late), 4, 2, 2))
    for k in range(len(late)):
        for axis in (0, 1):
            moved = []
            for sign in (1.0, -1.0):
                nudged = late.copy()
                nudged[k, axis] += sign * eps
                moved.append(so.transfer(host.lsq_homography(early, nudged), CORNERS))
            jac[k, :, :, axis] = (moved[0] - moved[1]) / (2 * eps)
    return np.linalg.norm(jac, ord=2, axis=(2, 3)).sum(axis=0)


@functools.lru_cache(maxsize=None)
def textbook_pipeline():
    """Per pair (homography, leverage (4,), the number of tracks fitted): corners of `track_definition.fast_corners` per sub-frame (the
    first MAX_PER in row-major order, as the device keeps them), `textbook_lk` with found = converged, then the tracker's own host
    finisher -- `host.ransac_inliers` per sub-frame and `host.lsq_homography` over the survivors."""
    from meshflow_amd import tracker
    frames, _ = clip_and_truth()
    rects = so.subframes(FRAME_W, FRAME_H, 2, 2)
    out = []
    for early, late in zip(frames[:-1], frames[1:]):
        points, moved = np.zeros((4, MAX_PER, 2), np.float32), np.zeros((4, MAX_PER, 2), np.float32)
        counts, found = np.zeros(4, np.int32), np.zeros((4, MAX_PER), np.uint8)
        for s, (left, top, w, h) in enumerate(rects):
            e, l = (np.ascontiguousarray(f[top:top + h, left:left + w]) for f in (early, late))
            corners = td.fast_corners(e)
            assert MIN_FEATURES <= len(corners) <= MAX_PER, len(corners)
            where, converged = so.textbook_lk(e, l, corners)
            counts[s] = len(corners)
            points[s, :len(corners)], moved[s, :len(corners)], found[s, :len(corners)] = corners, where, converged
        e, l, h = tracker.finish_pair((FRAME_W // 2, FRAME_H // 2, 2, 2), points, counts, moved.astype(np.float64), found, MIN_FEATURES)
        assert h is not None
        out.append((h, corner_leverage(e, l), len(e)))
    return out


def judge_clip(tracked):
    """`tracked`: DeviceTracker.track_clip's list for the clip above."""
    _, truth = clip_and_truth()
    want = so.transfer(truth, CORNERS)
    assert len(tracked) == 3
    for t, ((early, late, h), (textbook_h, leverage, fitted)) in enumerate(zip(tracked, textbook_pipeline())):
        assert h is not None, t
        error = so.distance(so.transfer(h, CORNERS), want)
        textbook_error = so.distance(so.transfer(textbook_h, CORNERS), want)
        print('pair %d: %d tracks (textbook %d), corner transfer error %s, textbook %s, leverage %s' %
              (t, len(early), fitted, np.round(error, 4).tolist(), np.round(textbook_error, 4).tolist(), np.round(leverage, 3).tolist()))
        assert (error <= textbook_error + so.BAR * leverage.max()).all(), (t, error, textbook_error, leverage.max())


def test_track_clip_fits_the_homography_as_well_as_the_textbook_pipeline(dev):
    import torch
    from meshflow_amd.tracker import DeviceTracker
    frames, _ = clip_and_truth()
    judge_clip(DeviceTracker(2, 2, MIN_FEATURES, device=str(dev), max_per_subframe=MAX_PER).track_clip(torch.from_numpy(frames).to(dev)))
