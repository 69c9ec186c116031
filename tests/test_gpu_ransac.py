"""The device outlier step against its specification, tests/ransac_model.py, bit for bit: `ops.ransac_inliers` (masks and all four info
fields) and `ops.gather_inliers` on the crafted sub-frames of tests/ransac_cases.py -- one launch of 3 pairs x 6 sub-frames with different
contents each, under every parameter set --, the sub-frame beyond the staged capacity, and `estimate_motion(outliers='device')` /
`DeviceTracker(outliers='device')` end to end against the model pipeline (tests/track_model.py corners and LK -> model RANSAC ->
`host.lsq_homography`).  Every case takes well under a second of model time."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_cases as rc  # noqa: E402
import ransac_model as rm  # noqa: E402
import tracker_clip  # noqa: E402
from tracker_clip import MAX_PER, SHIFTS, model_corners, model_lk, same_bits, stabilizer  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, ROWS, COLS = 100, 75, 2, 3                                         # 3 x 2 sub-frames of 34 x 38, the last column 32 and the last row 37


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def crafted():
    return rc.crafted()


@pytest.fixture(scope='module')
def crafted_model(crafted):
    """The model's (inlier, info) of the crafted launch per parameter set, computed once."""
    points, counts, moved, found = crafted
    return {p: rm.ransac_inliers(points, counts, moved, found, min_features=p[2], max_iters=p[0], seed=p[1]) for p in rc.CRAFTED_PARAMS}


def on_device(dev, *arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def run_ransac(dev, arrays, **kw):
    from meshflow_amd import ops
    points, counts, moved, found = on_device(dev, *arrays)
    inlier, info = ops.ransac_inliers(points, counts, moved, found, **kw)
    return inlier.cpu().numpy(), info.cpu().numpy()


@pytest.mark.parametrize('params', rc.CRAFTED_PARAMS)
def test_ransac_equals_the_model(dev, crafted, crafted_model, params):
    max_iters, seed, min_features = params
    inlier, info = run_ransac(dev, crafted, min_features=min_features, max_iters=max_iters, seed=seed)
    want_inlier, want_info = crafted_model[params]
    same_bits(info, want_info, ('info', params))
    same_bits(inlier, want_inlier, ('inlier', params))


def test_two_launches_give_the_same_bytes(dev, crafted):
    a, b = run_ransac(dev, crafted, seed=5), run_ransac(dev, crafted, seed=5)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_more_candidates_than_the_staged_capacity(dev):
    """max_per_subframe = 1,024 + 65, two sub-frames: the second holds a candidate in every slot, so its wavefront compacts into ITS run of
    the workspace (not the first slot's) and reads its candidates from there; the first stays in LDS."""
    arrays = rc.beyond_staged(1024)
    inlier, info = run_ransac(dev, arrays)
    want_inlier, want_info = rm.ransac_inliers(*arrays)
    assert want_info[0, :, 0].tolist() == [rm.OK, rm.OK] and want_info[0, :, 1].tolist() == [70, 1089]
    same_bits(info, want_info, 'info')
    same_bits(inlier, want_inlier, 'inlier')


@pytest.mark.parametrize('min_features', [4, 10, 150, 250])
def test_gather_equals_the_model(dev, crafted, crafted_model, min_features):
    """The pairs hold 110, 358 and 206 survivors in the model: at min_features 150 the first pair falls below it and is empty and flagged, at
    250 the first and the last."""
    from meshflow_amd import ops
    points, counts, moved, found = crafted
    want_inlier, want_info = crafted_model[(2000, 0, 10 if min_features == 10 else 4)]
    want = rm.gather(points, moved, want_inlier, want_info, ops.track_subframe_grid(W, H, ROWS, COLS), min_features)
    assert want[3].tolist() == {150: [rm.PAIR_TOO_FEW, 0, 0], 250: [rm.PAIR_TOO_FEW, 0, rm.PAIR_TOO_FEW]}.get(min_features, [0, 0, 0]), want[2]
    assert want[2].tolist() == {4: [0, 110, 468, 674], 10: [0, 101, 459, 657], 150: [0, 0, 358, 564], 250: [0, 0, 358, 358]}[min_features]
    d_points, d_moved, d_inlier, d_info = on_device(dev, points, moved, want_inlier, want_info)
    got = ops.gather_inliers(d_points, d_moved, d_inlier, d_info, W, H, ROWS, COLS, min_features)
    for g, w, what in zip(got, want, ('early', 'late', 'offsets', 'pair_status')):
        same_bits(g.cpu().numpy(), w, (what, min_features))


def test_gather_follows_the_device_ransac(dev, crafted, crafted_model):
    """The two calls chained on the device, as the tracker chains them."""
    from meshflow_amd import ops
    points, counts, moved, found = crafted
    d_points, d_counts, d_moved, d_found = on_device(dev, *crafted)
    inlier, info = ops.ransac_inliers(d_points, d_counts, d_moved, d_found, seed=5)
    got = ops.gather_inliers(d_points, d_moved, inlier, info, W, H, ROWS, COLS, 4)
    want = rm.gather(points, moved, *crafted_model[(2000, 5, 4)], ops.track_subframe_grid(W, H, ROWS, COLS), 4)
    for g, w, what in zip(got, want, ('early', 'late', 'offsets', 'pair_status')):
        same_bits(g.cpu().numpy(), w, what)


@pytest.fixture(scope='module')
def clip():
    return tracker_clip.clip()


@pytest.fixture(scope='module')
def model_pairs(clip):
    """The model pipeline per pair: tests/track_model.py corners and LK -> model RANSAC -> host.lsq_homography."""
    from meshflow_amd import ops
    grid = ops.track_subframe_grid(128, 96, 2, 2)
    out = []
    for early, late in zip(clip[:-1], clip[1:]):
        points, counts, _ = model_corners(early, 2, 2, MAX_PER)
        moved, found = model_lk(early, late, 2, 2, points, counts)
        out.append(rm.finish_pair(grid, points, counts, moved, found, 4))
    return out


def test_estimate_motion_on_the_device_equals_the_model_pipeline(dev, clip, model_pairs):
    import torch
    s = stabilizer(dev)
    d_grey = torch.from_numpy(clip).to(dev)
    tracked = s.device_tracker(MAX_PER, outliers='device').track_clip(d_grey)
    assert len(tracked) == 5
    for t, ((e, l, h), (we, wl, wh)) in enumerate(zip(tracked, model_pairs)):
        assert wh is not None and len(we) >= 16, t
        same_bits(e, we, ('early', t))
        same_bits(l, wl, ('late', t))
        same_bits(h, wh, ('homography', t))
        centre = h @ np.array([64.0, 48.0, 1.0])
        assert np.abs(centre[:2] / centre[2] - np.array([64.0, 48.0]) - np.array(SHIFTS[t])).max() < 0.5, (t, centre)
    d_disp, hom = s.estimate_motion(d_grey, max_per_subframe=MAX_PER, outliers='device')
    want_h = np.stack([h for _, _, h in model_pairs] + [np.identity(3)])
    want_disp, _ = s._get_unstabilized_vertex_displacements_from_features(6, 128, 96, [(e, l) for e, l, _ in model_pairs], want_h)
    same_bits(hom, want_h, 'homographies')
    same_bits(d_disp.cpu().numpy(), want_disp, 'd_disp')
    assert d_disp.is_cuda and d_disp.dtype == torch.float64 and tuple(d_disp.shape) == (6, 5, 5, 2)
    d_disp2, hom2 = s.estimate_motion(d_grey, chunk_pairs=2, max_per_subframe=MAX_PER, outliers='device')
    same_bits(hom2, want_h, 'homographies, chunks of 2')
    same_bits(d_disp2.cpu().numpy(), want_disp, 'd_disp, chunks of 2')


def test_chunked_clip_and_pairs_equal_one_chunk(dev, clip, model_pairs):
    import torch
    t = stabilizer(dev).device_tracker(MAX_PER, outliers='device')
    d_grey = torch.from_numpy(clip).to(dev)
    two, five = t.track_clip(d_grey, chunk_pairs=2), t.track_clip(d_grey, chunk_pairs=5)
    pairs = t.track_pairs(list(clip[:-1]), list(clip[1:]), chunk_pairs=3)
    one = t.track_pair(clip[0], clip[1])
    for a, b, c, d in zip(two, five, pairs, model_pairs):
        for x, y, z, m in zip(a, b, c, d):
            same_bits(x, y, 'chunks')
            same_bits(x, z, 'track_pairs')
            same_bits(x, m, 'model')
    for x, m in zip(one, model_pairs[0]):
        same_bits(x, m, 'track_pair')
    assert t.track_stacks(d_grey[:0], d_grey[:0]) == []                  # no pair: no result, as in the host mode
    _, (early, late, offsets, kmax) = t.track_stacks_packed(d_grey[:0], d_grey[:0])
    assert tuple(early.shape) == tuple(late.shape) == (0, 2) and offsets.tolist() == [0] and kmax == 0


def test_a_featureless_pair_raises_todays_error(dev, clip):
    import torch
    s = stabilizer(dev)
    flat = clip.copy()
    flat[2] = 128                                                        # pair (2, 3) has no corner in any sub-frame
    t = s.device_tracker(MAX_PER, outliers='device')
    got = t.track_clip(torch.from_numpy(flat).to(dev), chunk_pairs=2)
    assert got[2] == (None, None, None) and got[0][2] is not None and got[4][2] is not None
    # pair (1, 2), into the flat frame, yields whatever the model pipeline yields (tests/test_gpu_track.py says why that need not be nothing)
    from meshflow_amd import ops
    points, counts, _ = model_corners(flat[1], 2, 2, MAX_PER)
    moved, found = model_lk(flat[1], flat[2], 2, 2, points, counts)
    want = rm.finish_pair(ops.track_subframe_grid(128, 96, 2, 2), points, counts, moved, found, 4)
    assert (want[2] is None) == (got[1][2] is None)
    if want[2] is not None:
        for x, y in zip(got[1], want):
            same_bits(x, y, 'into the flat frame')
    first = 1 if want[2] is None else 2
    with pytest.raises(ValueError, match='fewer than 4 features could be tracked from frame %d to frame %d' % (first, first + 1)):
        s.estimate_motion(torch.from_numpy(flat).to(dev), max_per_subframe=MAX_PER, outliers='device')
    with pytest.raises(ValueError, match="outliers must be 'host' or 'device'"):
        s.estimate_motion(torch.from_numpy(flat).to(dev), outliers='gpu')
