"""What the luma pipeline's tests share: tests/tracker_clip.py's 6-frame 128 x 96 clip g made colour as B = 255 - g, G = g, R = g -- the
channels differ, luma ~ 0.772 g + 29, and reading it red-first changes the result --, its 16-bit, BGRA and P010 forms, and the tests' model
pipeline on a stack of pairs (tests/track_model.py corners and LK -> model RANSAC -> model fit), as tests/test_gpu_scores.py builds its own."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homography_model as hm  # noqa: E402
import ransac_model as rm  # noqa: E402
import tracker_clip  # noqa: E402
from tracker_clip import MAX_PER, model_corners, model_lk  # noqa: E402

W, H = 128, 96


def _noise(shape, top, seed):
    from meshflow_amd import synthetic
    return (synthetic.hash32(np.arange(int(np.prod(shape))), seed) % top).reshape(shape)


def grey():
    return tracker_clip.clip()


def bgr(g):
    return np.ascontiguousarray(np.stack([255 - g, g, g], axis=-1))


def bgra(g):
    return np.ascontiguousarray(np.concatenate([bgr(g), _noise(g.shape + (1,), 256, 31).astype(np.uint8)], axis=-1))


def bgr16(g):
    return bgr(g).astype(np.uint16) * 257


def p010(g):
    """(d_y, d_uv): the clip's levels in the high byte, hashed noise in the six bits under the ten, hashed 10-bit chroma."""
    y = (g.astype(np.uint16) << 8) | (_noise(g.shape, 64, 32).astype(np.uint16))
    uv = (_noise((len(g), H // 2, W // 2, 2), 1024, 33).astype(np.uint16)) << 6
    return y, uv


def reversed_channels(frames):
    out = frames.copy()
    out[..., 0], out[..., 2] = frames[..., 2], frames[..., 0]
    return out


def model_fit_records(early_stack, late_stack):
    """The model pipeline's fit record (status, ...) of every pair (early_stack[t], late_stack[t])."""
    from meshflow_amd import ops
    grid = ops.track_subframe_grid(W, H, 2, 2)
    records = []
    for early, late in zip(early_stack, late_stack):
        points, counts, _ = model_corners(early, 2, 2, MAX_PER)
        moved, found = model_lk(early, late, 2, 2, points, counts)
        inlier, info = rm.ransac_inliers(points[None], counts[None], moved[None], found[None], 4)
        e, l, _, _ = rm.gather(points[None], moved[None], inlier, info, grid, 4)
        records.append(hm.fit_pair(e, l)[1])
    return np.stack(records)
