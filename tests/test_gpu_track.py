"""The device tracker against its specification, tests/track_model.py, bit for bit: FAST corners (positions, true counts, the status word),
pyramidal LK (positions, found flags), and `MeshFlowStabilizer.estimate_motion` / `DeviceTracker` end to end against the model pipeline fed
through the same host functions.  The frames are the smallest at which the kernels can still go wrong: more than one FAST tile per
sub-frame (tiles decide 56 x 14 pixels), widths that are no multiple of 4, sub-frames of unequal size, every pyramid depth 0-3, windows that
meet every border.  Every case takes well under a second of model time."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_model as tm  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def noise(h, w, seed):
    from meshflow_amd import synthetic
    return (synthetic.hash32(np.arange(h * w), seed) & 255).astype(np.uint8).reshape(h, w)


def canvas(h, w, seed, boxes=90):
    """A smooth texture with hashed bright and dark boxes on it: LK has gradients everywhere, FAST has the boxes' corners."""
    from meshflow_amd import synthetic
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    v = 128 + 30 * np.sin(x * 0.31 + 0.2) * np.cos(y * 0.23) + 25 * np.sin(x * 0.13 + y * 0.19 + 1) + 20 * np.cos(x * 0.07 - y * 0.11)
    r = synthetic.hash32(np.arange(boxes * 5), seed).reshape(boxes, 5)
    for bx, by, bw, bh, val in r:
        x0, y0 = int(bx % w), int(by % h)
        v[y0:y0 + 5 + int(bh % 9), x0:x0 + 5 + int(bw % 9)] += int(val % 120) - 60
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def smooth(h, w, dx=0.0, dy=0.0):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    x, y = x - dx, y - dy
    v = 128 + 40 * np.sin(x * 0.31 + 0.2) * np.cos(y * 0.23) + 35 * np.sin(x * 0.13 + y * 0.19 + 1) + 30 * np.cos(x * 0.07 - y * 0.11) + \
        15 * np.sin(x * 0.45 - y * 0.4)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def model_corners(img, rows, cols, max_per, threshold=10):
    """The model's corners of one frame in the device's layout: points (S, max, 2), counts (S,), status (S,)."""
    subs = tm.subframes(img.shape[1], img.shape[0], rows, cols)
    points = np.zeros((len(subs), max_per, 2), np.float32)
    counts = np.zeros(len(subs), np.int32)
    for s, (left, top, w, h) in enumerate(subs):
        c = tm.fast_corners(np.ascontiguousarray(img[top:top + h, left:left + w]), threshold)
        counts[s] = len(c)
        points[s, :min(len(c), max_per)] = c[:max_per]
    return points, counts, (counts > max_per).astype(np.int32)


def model_lk(early, late, rows, cols, points, counts):
    """The model's LK of one pair on the device's layout."""
    subs = tm.subframes(early.shape[1], early.shape[0], rows, cols)
    moved, found = np.zeros_like(points), np.zeros(points.shape[:2], np.uint8)
    for s, (left, top, w, h) in enumerate(subs):
        k = min(int(counts[s]), points.shape[1])
        m, f = tm.lk_track(np.ascontiguousarray(early[top:top + h, left:left + w]), np.ascontiguousarray(late[top:top + h, left:left + w]),
                           points[s, :k])
        moved[s, :k], found[s, :k] = m, f
    return moved, found


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.nonzero(got.view(np.uint8).reshape(-1) != want.view(np.uint8).reshape(-1))[0]
    assert len(bad) == 0, (what, len(bad), np.argwhere(got != want)[:5].tolist())


def check_fast(dev, frames, rows, cols, max_per=256):
    import torch
    from meshflow_amd import ops
    frames = np.stack(frames)
    points, counts, status = ops.fast_corners(torch.from_numpy(frames).to(dev), rows, cols, max_per)
    points, counts, status = points.cpu().numpy(), counts.cpu().numpy(), status.cpu().numpy()
    total = 0
    for i, img in enumerate(frames):
        want_points, want_counts, want_status = model_corners(img, rows, cols, max_per)
        same_bits(counts[i], want_counts, ('counts', i))
        same_bits(status[i], want_status, ('status', i))
        same_bits(points[i], want_points, ('points', i))
        total += int(want_counts.sum())
    return total, counts, status


def test_fast_noise_one_and_four_subframes(dev):
    frames = [noise(48, 64, 1), noise(48, 64, 2)]
    assert check_fast(dev, frames, 1, 1)[0] > 50                        # 64 x 48: two tiles across, four down
    assert check_fast(dev, frames, 2, 2)[0] > 30


def test_fast_odd_frame_unequal_subframes(dev):
    """61 x 37 as 2 x 2: sub-frames of 31 x 19, 30 x 19, 31 x 18, 30 x 18 -- widths that are no multiple of 4, frames that start at odd bytes."""
    assert check_fast(dev, [noise(37, 61, 3), noise(37, 61, 4), noise(37, 61, 5)], 2, 2)[0] > 10
    assert check_fast(dev, [noise(37, 61, 3)], 3, 5)[0] >= 0             # 13 x 13 sub-frames, the last column 9 wide


def test_fast_more_than_one_tile_each_way(dev):
    assert check_fast(dev, [noise(33, 130, 6)], 1, 1, max_per=1024)[0] > 100     # three tiles across (56), three down (14)


def test_fast_smallest_subframes_and_constant(dev):
    lone = np.full((7, 7), 40, np.uint8)
    lone[3, 3] = 200
    total, counts, _ = check_fast(dev, [lone], 1, 1)
    assert total == 1 and counts.tolist() == [[1]]                      # a 7 x 7 sub-frame has exactly one pixel that can be a corner
    assert check_fast(dev, [noise(9, 6, 7)], 1, 1)[0] == 0               # 6 wide: none
    grid = np.full((14, 13), 40, np.uint8)                               # 2 x 2: two sub-frames of 7 x 7, two of 6 x 7
    grid[3, 3] = grid[10, 3] = grid[3, 10] = grid[10, 10] = 200
    total, counts, _ = check_fast(dev, [grid], 2, 2)
    assert counts.tolist() == [[1, 1, 0, 0]]
    assert check_fast(dev, [np.full((48, 64), 77, np.uint8)], 2, 2)[0] == 0


def test_fast_overflow_keeps_the_first_in_row_major_order(dev):
    from meshflow_amd import _lib
    frame = noise(48, 64, 8)
    total, counts, status = check_fast(dev, [frame], 1, 1, max_per=8)
    assert total > 8 and counts[0, 0] == total and status[0, 0] == _lib.TRACK_OVERFLOW
    _, counts, status = check_fast(dev, [frame, np.full((48, 64), 3, np.uint8)], 1, 1, max_per=8)
    assert status.tolist() == [[_lib.TRACK_OVERFLOW], [0]]


def check_lk(dev, early, late, rows, cols, points, counts):
    """points (S, max, 2) float32, counts (S,) for ONE pair; returns the model's (moved, found)."""
    import torch
    from meshflow_amd import ops
    moved, found = ops.lk_track(torch.from_numpy(early[None]).to(dev), torch.from_numpy(late[None]).to(dev),
                                torch.from_numpy(points[None]).to(dev), torch.from_numpy(counts[None].astype(np.int32)).to(dev), rows, cols)
    want_moved, want_found = model_lk(early, late, rows, cols, points, counts)
    same_bits(found.cpu().numpy()[0], want_found, 'found')
    same_bits(moved.cpu().numpy()[0], want_moved, 'moved')
    return want_moved, want_found


def hand_points(w, h):
    """A grid, the corner pixels, edge pixels and fractional positions of a w x h sub-frame, then positions outside it (lost)."""
    ys, xs = np.mgrid[4:h:9, 5:w:11]
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32).tolist()
    pts += [[0, 0], [w - 1, 0], [0, h - 1], [w - 1, h - 1], [w / 2, 0], [0, h / 2], [w - 1, h / 2 + 0.25], [w / 2 + 0.5, h - 1],
            [10.5, 10.5], [11.75, 12.125], [w - 0.5, h - 0.5]]
    pts += [[-12.5, 5], [w + 10, 5], [5, -11.25], [5, h + 10.5]]
    return np.array(pts, np.float32)


def test_lk_subpixel_shift_in_four_subframes(dev):
    """96 x 80 as 2 x 2: a 48 x 40 sub-frame has no second pyramid level (24 x 20 is not larger than the window) and every window meets a
    border.  One sub-frame gets no point, one a single point, one has a flat patch."""
    early, late = smooth(80, 96), smooth(80, 96, 2.25, -1.5)
    early[45:80, 50:96] = 90                                             # a flat patch in sub-frame 3 = (left 48, top 40)
    late[45:80, 50:96] = 90
    pts = hand_points(48, 40)
    points = np.zeros((4, len(pts) + 3, 2), np.float32)
    points[0, :len(pts)] = pts
    points[2, 0] = (20.5, 17.25)
    points[3, :len(pts)] = pts
    points[3, len(pts)] = (30, 25)                                       # in the flat patch: (78, 65) of the frame
    counts = np.array([len(pts), 0, 1, len(pts) + 1])
    moved, found = check_lk(dev, early, late, 2, 2, points, counts)
    assert found[0, :20].all() and not found[0, len(pts) - 4:len(pts)].any()      # inside: found; outside the image: lost
    assert found[2, 0] == 1 and found[3, len(pts)] == 0                 # the single point; the flat patch is rejected by minEig
    interior = np.abs(moved[0, :12] - points[0, :12] - np.float32([2.25, -1.5]))
    assert interior.max() < 0.5, interior.max()


@pytest.mark.parametrize('rows,cols', [(1, 1), (2, 2), (1, 3)])
def test_lk_every_pyramid_depth(dev, rows, cols):
    """200 x 180: one sub-frame has levels 0-3, 100 x 90 sub-frames levels 0-2, 67 x 180 sub-frames levels 0-1 (the last one 66 wide)."""
    big = canvas(200, 230, 11)
    early, late = np.ascontiguousarray(big[12:192, 20:220]), np.ascontiguousarray(big[9:189, 25:225])      # content moves by (-5, +3)
    subs = tm.subframes(200, 180, rows, cols)
    assert sorted({tm.num_levels(w, h) for _, _, w, h in subs}) == {(1, 1): [3], (2, 2): [2], (1, 3): [1]}[(rows, cols)]
    per = [hand_points(w, h) for _, _, w, h in subs]
    points = np.zeros((len(subs), max(len(p) for p in per), 2), np.float32)
    for s, p in enumerate(per):
        points[s, :len(p)] = p
    moved, found = check_lk(dev, early, late, rows, cols, points, np.array([len(p) for p in per]))
    assert found.sum() > 10


def test_lk_large_motion_loses_points_on_the_way(dev):
    """A 14-pixel shift in a one-level sub-frame: tracks diverge, some leave the image during the iterations -- the device follows the
    model through all of it."""
    big = canvas(60, 90, 12, boxes=40)
    early, late = np.ascontiguousarray(big[5:45, 20:68]), np.ascontiguousarray(big[5:45, 6:54])
    pts = hand_points(48, 40)
    check_lk(dev, early, late, 1, 1, pts[None].copy(), np.array([len(pts)]))


SHIFTS = ((3, -2), (-4, 1), (2, 2), (-1, -3), (5, 0))                    # content motion frame t -> t + 1, pixels


@pytest.fixture(scope='module')
def clip():
    """6 frames of 128 x 96 cut from one canvas at integer offsets, and the model's tracker output per pair in the device's layout."""
    big = canvas(140, 170, 21, boxes=160)
    ox, oy, frames = 20, 20, []
    for dx, dy in ((0, 0),) + SHIFTS:
        ox, oy = ox - dx, oy - dy
        frames.append(np.ascontiguousarray(big[oy:oy + 96, ox:ox + 128]))
    return np.stack(frames)


MAX_PER = 48


@pytest.fixture(scope='module')
def model_pairs(clip):
    from meshflow_amd import ops, tracker
    grid = ops.track_subframe_grid(128, 96, 2, 2)
    out = []
    for early, late in zip(clip[:-1], clip[1:]):
        points, counts, _ = model_corners(early, 2, 2, MAX_PER)
        moved, found = model_lk(early, late, 2, 2, points, counts)
        out.append(tracker.finish_pair(grid, points, counts, moved, found, 4))
    return out


def stabilizer(dev):
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    return MeshFlowStabilizer(mesh_row_count=4, mesh_col_count=4, mesh_outlier_subframe_row_count=2, mesh_outlier_subframe_col_count=2,
                              homography_min_number_corresponding_features=4, temporal_smoothing_radius=2,
                              optimization_num_iterations=10, device=str(dev))


def test_estimate_motion_equals_the_model_pipeline(dev, clip, model_pairs):
    import torch
    s = stabilizer(dev)
    d_grey = torch.from_numpy(clip).to(dev)
    tracked = s.device_tracker(MAX_PER).track_clip(d_grey)
    assert len(tracked) == 5
    for t, ((e, l, h), (we, wl, wh)) in enumerate(zip(tracked, model_pairs)):
        assert wh is not None and len(we) >= 16, t
        same_bits(e, we, ('early', t))
        same_bits(l, wl, ('late', t))
        same_bits(h, wh, ('homography', t))
        centre = h @ np.array([64.0, 48.0, 1.0])
        assert np.abs(centre[:2] / centre[2] - np.array([64.0, 48.0]) - np.array(SHIFTS[t])).max() < 0.5, (t, centre)
    d_disp, hom = s.estimate_motion(d_grey, max_per_subframe=MAX_PER)
    want_h = np.stack([h for _, _, h in model_pairs] + [np.identity(3)])
    want_disp, _ = s._get_unstabilized_vertex_displacements_from_features(6, 128, 96, [(e, l) for e, l, _ in model_pairs], want_h)
    same_bits(hom, want_h, 'homographies')
    same_bits(d_disp.cpu().numpy(), want_disp, 'd_disp')
    assert d_disp.is_cuda and d_disp.dtype == torch.float64 and tuple(d_disp.shape) == (6, 5, 5, 2)
    out, bounds, stab = s.stabilize_resident(d_grey, d_disp, hom)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (6, 96, 128) and out.dtype == torch.uint8 and tuple(stab.shape) == (6, 5, 5, 2)


def test_chunked_clip_equals_one_chunk(dev, clip, model_pairs):
    import torch
    t = stabilizer(dev).device_tracker(MAX_PER)
    d_grey = torch.from_numpy(clip).to(dev)
    two, five = t.track_clip(d_grey, chunk_pairs=2), t.track_clip(d_grey, chunk_pairs=5)
    for a, b, c in zip(two, five, model_pairs):
        for x, y, z in zip(a, b, c):
            same_bits(x, y, 'chunks')
            same_bits(x, z, 'model')


def test_constant_frames_do_not_raise(dev, clip):
    """A constant EARLY frame has no corner in any sub-frame: where the reference dies in np.concatenate, the tracker returns the None triple.
    A constant LATE frame is not untrackable for cv2's LK, which never looks at the late image's texture: every window's mismatch vector b is
    the same wherever the window stands, so each track drifts by a fixed step and is "found" unless it leaves the image (the model on this
    clip: 138 of 192 corners found), and four pairs always fit some homography.  So the pair yields whatever the model pipeline yields --
    compared bit for bit here -- and nothing raises, in a kernel or on the host."""
    from meshflow_amd import ops, tracker
    t = stabilizer(dev).device_tracker(MAX_PER)
    flat = np.full_like(clip[0], 128)
    assert t.track_pair(flat, clip[0]) == (None, None, None)
    assert t.track_pair(flat, flat) == (None, None, None)
    got = t.track_pairs([clip[0], clip[0], flat], [clip[1], flat, clip[1]])
    assert got[0][2] is not None and got[2] == (None, None, None)
    points, counts, _ = model_corners(clip[0], 2, 2, MAX_PER)
    moved, found = model_lk(clip[0], flat, 2, 2, points, counts)
    want = tracker.finish_pair(ops.track_subframe_grid(128, 96, 2, 2), points, counts, moved, found, 4)
    assert (want[2] is None) == (got[1][2] is None)
    if want[2] is not None:
        for x, y in zip(got[1], want):
            same_bits(x, y, 'constant late frame')
