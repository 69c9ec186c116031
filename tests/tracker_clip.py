"""What the outlier step's GPU tests share with tests/test_gpu_track.py's end-to-end cases, restated here so that no test module imports
another: the textured canvas and the 6-frame clip cut from it, the model's corners and LK in the device's layout (tests/track_model.py),
the bit comparison and the stabilizer of the end-to-end tests."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_model as tm  # noqa: E402

SHIFTS = ((3, -2), (-4, 1), (2, 2), (-1, -3), (5, 0))                    # content motion frame t -> t + 1, pixels
MAX_PER = 48


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


def stabilizer(dev):
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    return MeshFlowStabilizer(mesh_row_count=4, mesh_col_count=4, mesh_outlier_subframe_row_count=2, mesh_outlier_subframe_col_count=2,
                              homography_min_number_corresponding_features=4, temporal_smoothing_radius=2,
                              optimization_num_iterations=10, device=str(dev))


def clip():
    """6 frames of 128 x 96 cut from one canvas at integer offsets."""
    big = canvas(140, 170, 21, boxes=160)
    ox, oy, frames = 20, 20, []
    for dx, dy in ((0, 0),) + SHIFTS:
        ox, oy = ox - dx, oy - dy
        frames.append(np.ascontiguousarray(big[oy:oy + 96, ox:ox + 128]))
    return np.stack(frames)
