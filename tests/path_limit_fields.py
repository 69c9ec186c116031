"""The motion fields the path limiter's tests share (tests/test_path_limit_model.py proves on the CPU that the model's limited paths are
covered; tests/test_gpu_path_limit.py runs the same set through the kernels): 128 x 96 frames, per frame a correction d = p - c made of a
global shift of up to 25 px per axis, an affine part of up to +-8 % and up to 0.3 px of noise per vertex, on a wandering unstabilized path."""
import math

import numpy as np

import path_limit_model as pm

W, H = 128, 96
STEPS, GUARD, RISE = 32, 2.0, 2
MESHES = ((1, 1), (1, 2), (3, 1), (16, 16))
MARGINS = (0.08, 0.15)
FRAMES = 24
SHIFT, AFFINE, NOISE = 25.0, 0.08, 0.3


def rectangle(margin):
    left, top = math.floor(margin * (W - 1)), math.floor(margin * (H - 1))
    return left, top, (W - 1) - left, (H - 1) - top


def field(R, C, seed, frames=FRAMES):
    """(c, p): (frames, S) float64 each."""
    rng = np.random.default_rng(seed)
    xs, ys = pm.grid(W, H, R, C)
    gx, gy = np.meshgrid(xs - (W - 1) / 2, ys - (H - 1) / 2)                 # (R+1, C+1)
    c = np.cumsum(rng.uniform(-3, 3, (frames, 1, 1, 2)), axis=0) + rng.uniform(-0.5, 0.5, (frames, R + 1, C + 1, 2))
    shift = rng.uniform(-SHIFT, SHIFT, (frames, 2))
    shift[::3] *= 0.2                                                       # a third of the frames near the rectangle's reach
    a = rng.uniform(-AFFINE, AFFINE, (frames, 2, 2))
    d = np.empty((frames, R + 1, C + 1, 2))
    d[..., 0] = shift[:, 0, None, None] + a[:, 0, 0, None, None] * gx + a[:, 0, 1, None, None] * gy
    d[..., 1] = shift[:, 1, None, None] + a[:, 1, 0, None, None] * gx + a[:, 1, 1, None, None] * gy
    d += rng.uniform(-NOISE, NOISE, d.shape)
    S = (R + 1) * (C + 1) * 2
    return c.reshape(frames, S), (c + d).reshape(frames, S)


def cases():
    """[(R, C, margin, rectangle, c, p)] of the whole set."""
    out = []
    for i, (R, C) in enumerate(MESHES):
        for j, margin in enumerate(MARGINS):
            c, p = field(R, C, 100 + 10 * i + j)
            out.append((R, C, margin, rectangle(margin), c, p))
    return out


def covered(crop, rect):
    """(n,) bool from (n, 4) crop values {left, top, right, bottom}: the session's `covered`."""
    crop = np.asarray(crop)
    return (crop[:, 0] <= rect[0]) & (crop[:, 1] <= rect[1]) & (crop[:, 2] >= rect[2]) & (crop[:, 3] >= rect[3])
