"""The device tracker on the paths tests/test_gpu_track.py and tests/test_gpu_ransac.py do not reach, bit for bit against tests/track_model.py
and tests/ransac_model.py on the cases of tests/track_edge_cases.py (tests/test_track_edge_cases.py proves on the CPU that each reaches its
path): `fast_compact_kernel`'s second and later rounds of 64 rows with the capacity cutting in each, FAST at thresholds other than 10, at
the score 254 and with tied neighbours across tile edges, a grid with fewer sub-frames than asked for, LK launches whose sub-frames
differ in pyramid depth, LK on 0/255 images, and `track_gather_kernel` with more than 64 pairs and with more than 64 sub-frames.  Every
call is a legal one; every case takes well under a second of model time."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_model as rm  # noqa: E402
import track_edge_cases as ec  # noqa: E402
import track_model as tm  # noqa: E402
from tracker_clip import model_corners, model_lk, same_bits  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def on_device(dev, *arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def check_fast(dev, frames, rows, cols, max_per, threshold=None):
    """`ops.fast_corners` of a stack against the model, image by image; returns the device's (counts, status)."""
    from meshflow_amd import ops
    frames = np.stack(frames)
    kw = {} if threshold is None else {'threshold': threshold}
    points, counts, status = (t.cpu().numpy() for t in ops.fast_corners(on_device(dev, frames)[0], rows, cols, max_per, **kw))
    for i, img in enumerate(frames):
        want_points, want_counts, want_status = model_corners(img, rows, cols, max_per, **kw)
        same_bits(counts[i], want_counts, ('counts', i, max_per, threshold))
        same_bits(status[i], want_status, ('status', i, max_per, threshold))
        same_bits(points[i], want_points, ('points', i, max_per, threshold))
    return counts, status


# ---- a. sub-frames of more than 64 rows ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', list(ec.tall_cases()))
def test_fast_tall_subframes(dev, name):
    from meshflow_amd import _lib
    img, bands, runs = ec.tall_cases()[name]
    for rows, cols, max_per, where in runs:
        counts, status = check_fast(dev, [img], rows, cols, max_per)
        if (rows, cols) == (1, 1):
            assert counts.tolist() == [[sum(bands)]] and status.tolist() == [[0 if where is None else _lib.TRACK_OVERFLOW]]


def test_fast_tall_stack_counts_every_slot_from_zero(dev):
    from meshflow_amd import _lib
    counts, status = check_fast(dev, ec.tall_stack(), 1, 1, 300)
    assert counts.tolist() == [[522], [0]] and status.tolist() == [[_lib.TRACK_OVERFLOW], [0]]
    counts, _ = check_fast(dev, ec.tall_stack()[::-1], 1, 1, 1024)
    assert counts.tolist() == [[0], [522]]


# ---- b. thresholds, the largest score, ties -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('threshold', list(ec.THRESHOLDS))
def test_fast_thresholds(dev, threshold):
    counts, _ = check_fast(dev, [ec.threshold_frame()], 1, 1, 512, threshold)
    assert counts.tolist() == [[ec.THRESHOLDS[threshold]]]
    check_fast(dev, [ec.threshold_frame()], 2, 2, 512, threshold)


def test_fast_binary_frames(dev):
    counts, _ = check_fast(dev, [ec.binary_frame(), ec.binary_frame(3)], 1, 1, 256)
    assert counts.tolist() == [[31], [15]]
    counts, _ = check_fast(dev, [ec.binary_frame(3), ec.binary_frame()], 2, 2, 256)
    assert counts[0].tolist() == [2, 1, 4, 7]
    for threshold in (1, 254):
        check_fast(dev, [ec.binary_frame(), ec.binary_frame(3)], 1, 1, 256, threshold)


def test_fast_ties_across_tile_edges(dev):
    frames = [ec.quadrant(x, y) for x, y in ec.QUADRANT_CORNERS]
    counts, _ = check_fast(dev, frames, 1, 1, 64)
    assert counts.tolist() == [[0]] * 3
    # the same ties in the second column / row of sub-frames: (55, 20) and (55, 13) of a sub-frame that starts at (80, 40)
    wide = np.full((80, 160), 20, np.uint8)
    wide[40:, 80:] = ec.quadrant(55, 13)
    wide[:40, 80:] = ec.quadrant(55, 20)
    check_fast(dev, [wide], 2, 2, 64)


# ---- c. fewer sub-frames than asked for ---------------------------------------------------------------------------------------------------

def test_fast_fewer_subframes_than_asked_for(dev):
    W, H, rows, cols = ec.FEWER
    sets = ec.fewer_lit_sets()
    counts, _ = check_fast(dev, [ec.fewer_frame(sets[0])], rows, cols, 4)
    assert counts.shape == (1, 49) and counts[0].tolist() == [1, 0] * 24 + [1]
    counts, _ = check_fast(dev, [ec.fewer_frame(lit) for lit in sets], rows, cols, 4)
    assert counts.tolist() == [lit.astype(int).tolist() for lit in sets]


# ---- d. unequal pyramid depths ------------------------------------------------------------------------------------------------------------

def check_lk(dev, earlies, lates, rows, cols, max_per):
    """The model's corners of every early frame tracked into its late frame in ONE launch, against the model pair by pair."""
    from meshflow_amd import ops
    corners = [model_corners(e, rows, cols, max_per) for e in earlies]
    points, counts = np.stack([c[0] for c in corners]), np.stack([c[1] for c in corners])
    moved, found = ops.lk_track(*on_device(dev, np.stack(earlies), np.stack(lates), points, counts), rows, cols)
    moved, found = moved.cpu().numpy(), found.cpu().numpy()
    for i, (e, l) in enumerate(zip(earlies, lates)):
        want_moved, want_found = model_lk(e, l, rows, cols, points[i], counts[i])
        same_bits(found[i], want_found, ('found', i))
        same_bits(moved[i], want_moved, ('moved', i))
        assert want_found.sum(axis=1).min() >= 10
    return found


@pytest.mark.parametrize('name', list(ec.MIXED))
def test_lk_mixed_depths_in_one_launch(dev, name):
    """One launch per level serves sub-frames of two depths: the shallower ones sit out the upper launches and start from `points` at their
    OWN top level.  What this can tell apart: a start at the launch's top level (the model run that way differs in all three shallower
    sub-frames of both cases), a seed or flag taken from `moved` / `found` at a sub-frame's own top, and the level's sub-image address.
    What no result can show is the `level > top` return by itself: a wavefront that ran a level above its top would be overwritten from
    `points` at its top level, so that return saves work and reads of unwritten workspace, nothing else."""
    size, _, _, want_depths = ec.MIXED[name]
    assert ec.depths(size, size, 2, 2) == want_depths
    early, late = ec.mixed_pair(name)
    check_lk(dev, [early], [late], 2, 2, ec.MIXED_MAX_PER)
    check_lk(dev, [early, late], [late, early], 2, 2, ec.MIXED_MAX_PER)  # the second pair swapped: the late pyramid at (n_pairs S + slot)


def test_fast_into_lk_on_the_device_at_depth_three(dev):
    """200 x 180 as one sub-frame: 180 mask rows, four pyramid levels, the device's corners and counts straight into the device's LK."""
    from meshflow_amd import _lib, ops
    early, late = ec.depth_pair()
    d_early, d_late = on_device(dev, early[None], late[None])
    points, counts, status = ops.fast_corners(d_early, 1, 1, ec.MIXED_MAX_PER)
    moved, found = ops.lk_track(d_early, d_late, points, counts, 1, 1)
    want_points, want_counts, want_status = model_corners(early, 1, 1, ec.MIXED_MAX_PER)
    want_moved, want_found = model_lk(early, late, 1, 1, want_points, want_counts)
    assert want_counts.tolist() == [412] and want_status.tolist() == [_lib.TRACK_OVERFLOW] and want_found.sum() == 64
    same_bits(counts.cpu().numpy()[0], want_counts, 'counts')
    same_bits(status.cpu().numpy()[0], want_status, 'status')
    same_bits(points.cpu().numpy()[0], want_points, 'points')
    same_bits(found.cpu().numpy()[0], want_found, 'found')
    same_bits(moved.cpu().numpy()[0], want_moved, 'moved')


# ---- e. steep gradients -------------------------------------------------------------------------------------------------------------------

def test_lk_on_binary_frames(dev):
    """0/255 images: window sums near 2^31 (the model: up to 1,774,461,552 for Ix Ix), per-lane partial sums and products at their largest."""
    from meshflow_amd import ops
    points = ec.steep_points()
    pairs = ec.steep_pairs()
    for group in (pairs[:1], pairs[1:]):                                 # the per-pixel image alone; the blocked one as two pairs, 1 px and 6 px
        n = len(group)
        early, late = np.stack([e for _, e, _ in group]), np.stack([l for _, _, l in group])
        pts, counts = np.tile(points[None, None], (n, 1, 1, 1)), np.full((n, 1), len(points), np.int32)
        moved, found = ops.lk_track(*on_device(dev, early, late, pts, counts), 1, 1)
        for i, (name, e, l) in enumerate(group):
            want_moved, want_found = tm.lk_track(e, l, points)
            assert np.isfinite(want_moved).all()
            same_bits(found.cpu().numpy()[i, 0], want_found, ('found', name))
            same_bits(moved.cpu().numpy()[i, 0], want_moved, ('moved', name))


def test_lk_on_a_checkerboard_whose_window_sums_pass_int32(dev):
    """The model's sums of Ix Ix and Iy Iy exceed 2^31 in 44 of the 80 windows (up to 3,150,071,100): the wavefront's reduction must be int64."""
    from meshflow_amd import ops
    early, late, points = ec.checker_pair()
    moved, found = ops.lk_track(*on_device(dev, early[None], late[None], points[None, None], np.full((1, 1), len(points), np.int32)), 1, 1)
    want_moved, want_found = tm.lk_track(early, late, points)
    assert want_found.all()
    same_bits(found.cpu().numpy()[0, 0], want_found, 'found')
    same_bits(moved.cpu().numpy()[0, 0], want_moved, 'moved')


# ---- f. second trips of the lane strides --------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def stride_models():
    """The launches and the model's (inlier, info) of each, computed once."""
    out = {}
    for name in ec.STRIDE_LAUNCHES:
        arrays = ec.stride_launch(name)
        out[name] = (arrays, rm.ransac_inliers(*arrays))
    return out


@pytest.mark.parametrize('name', list(ec.STRIDE_LAUNCHES))
def test_ransac_and_gather_beyond_64_pairs_and_subframes(dev, stride_models, name):
    from meshflow_amd import ops
    _, _, (W, H, rows, cols) = ec.STRIDE_LAUNCHES[name]
    (points, counts, moved, found), (want_inlier, want_info) = stride_models[name]
    assert int(want_inlier.sum()) == ec.STRIDE_SURVIVORS
    d_points, d_counts, d_moved, d_found = on_device(dev, points, counts, moved, found)
    inlier, info = ops.ransac_inliers(d_points, d_counts, d_moved, d_found)
    same_bits(info.cpu().numpy(), want_info, 'info')
    same_bits(inlier.cpu().numpy(), want_inlier, 'inlier')
    d_want_inlier, d_want_info = on_device(dev, want_inlier, want_info)
    grid = ops.track_subframe_grid(W, H, rows, cols)
    for min_features in ec.STRIDE_MIN_FEATURES:
        want = rm.gather(points, moved, want_inlier, want_info, grid, min_features)
        fed = ops.gather_inliers(d_points, d_moved, d_want_inlier, d_want_info, W, H, rows, cols, min_features)
        chained = ops.gather_inliers(d_points, d_moved, inlier, info, W, H, rows, cols, min_features)
        for got, how in ((fed, 'fed the model'), (chained, 'chained')):
            for g, w, what in zip(got, want, ('early', 'late', 'offsets', 'pair_status')):
                same_bits(g.cpu().numpy(), w, (what, how, min_features))
