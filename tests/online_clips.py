"""What the online-session suites share (tests/test_gpu_online_session.py, _cuts, _limit and _lag_session; tests/cuts_clip.py), once, so that
no test module imports another: the ten 128 x 96 frames cut from tests/tracker_clip.py's canvas and the session they are pushed through, the
path-limit suite's shaky clip with its stabilizer and session, every form a push takes, and the slicing and comparing of clips that may be
4:2:0 pairs.  Plain functions and numbers: the fixtures stay in the test modules."""
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import luma_clip  # noqa: E402
import tracker_clip  # noqa: E402
from tracker_clip import MAX_PER, SHIFTS  # noqa: E402

W, H, R, C = 128, 96, 4, 4
S = (R + 1) * (C + 1) * 2
MORE_SHIFTS = ((-3, 2), (2, -4), (-5, 3), (4, 1))
WINDOW, ITERS, BETA, MARGIN = 4, 6, 1.0, 0.08
SESSION = dict(window=WINDOW, iters=ITERS, beta=BETA, crop_margin=MARGIN, max_per_subframe=MAX_PER)

# tests/test_gpu_online_limit.py's
K, RISE, GUARD = 32, 2, 2.0
FLOOR = 16                                                               # the canvas raised to it: the grey border byte, 0, is below every pixel
STEP = (0, -12)                                                          # content motion into frame 4; the margin leaves 7 rows, 10 columns
# a radius of 10 frames in a window of 12: at tests/tracker_clip.py's radius of 2 the smoother follows a step within two pixels
LIMIT_SESSION = dict(window=12, iters=6, beta=1.0, crop_margin=0.08, max_per_subframe=MAX_PER)


def cut_from(big):
    """Ten W x H frames of a canvas: the offsets of tests/tracker_clip.py's clip and four more."""
    ox, oy, frames = 20, 20, []
    for dx, dy in ((0, 0),) + SHIFTS + MORE_SHIFTS:
        ox, oy = ox - dx, oy - dy
        frames.append(np.ascontiguousarray(big[oy:oy + H, ox:ox + W]))
    return np.stack(frames)


def grey_clip():
    """tests/tracker_clip.py's clip with four more frames cut from the same canvas."""
    return cut_from(tracker_clip.canvas(140, 170, 21, boxes=160))


def limit_stabilizer(dev):
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    return MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, mesh_outlier_subframe_row_count=2, mesh_outlier_subframe_col_count=2,
                              homography_min_number_corresponding_features=4, temporal_smoothing_radius=10,
                              optimization_num_iterations=10, device=str(dev))


def shaky_clip():
    """14 frames of the session tests' canvas, not below FLOOR, the fourth move replaced by STEP."""
    big = np.maximum(tracker_clip.canvas(140, 170, 21, boxes=160), FLOOR)
    moves = SHIFTS + MORE_SHIFTS
    ox, oy = 20, 8
    frames = [big[oy:oy + H, ox:ox + W]]
    for dx, dy in moves[:3] + (STEP,) + moves[3:] + moves[:3]:
        ox, oy = ox - dx, oy - dy
        frames.append(big[oy:oy + H, ox:ox + W])
    return np.stack([np.ascontiguousarray(f) for f in frames])


def forms(g):
    """name -> the clip in that form, as NumPy (a pair for the 4:2:0 forms)."""
    uv = luma_clip._noise((len(g), H // 2, W // 2, 2), 256, 35).astype(np.uint8)
    return {'grey': g, 'bgr': luma_clip.bgr(g), 'nv12': (g, uv), 'bgr16': luma_clip.bgr16(g), 'bgra': luma_clip.bgra(g), 'p010': luma_clip.p010(g)}


def to_dev(clip, dev):
    import torch
    if isinstance(clip, tuple):
        return tuple(torch.from_numpy(np.ascontiguousarray(p)).to(dev) for p in clip)
    return torch.from_numpy(np.ascontiguousarray(clip)).to(dev)


def part(clip, lo, hi):
    return tuple(p[lo:hi] for p in clip) if isinstance(clip, tuple) else clip[lo:hi]


def host_of(frames):
    return tuple(p.cpu().numpy() for p in frames) if isinstance(frames, tuple) else frames.cpu().numpy()


def planes(frames):
    return [p.cpu().numpy() for p in frames] if isinstance(frames, tuple) else [frames.cpu().numpy()]


def same_frames(got, want, what):
    got, want = host_of(got), host_of(want)
    if isinstance(want, tuple):
        assert isinstance(got, tuple) and len(got) == 2, what
        for g, w, plane in zip(got, want, ('y', 'uv')):
            tracker_clip.same_bits(g, w, (what, plane))
    else:
        tracker_clip.same_bits(got, want, what)


def rectangle(margin):
    left, top = math.floor(margin * (W - 1)), math.floor(margin * (H - 1))
    return left, top, (W - 1) - left, (H - 1) - top
