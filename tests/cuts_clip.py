"""What the scene-cut tests share: scene A, the ten 128 x 96 frames of tests/online_clips.py's `grey_clip()` (canvas seed 21); scene B, the same
ten offsets cut from another canvas (seed 77) made darker by 60 levels; and the clips with cuts made of the two."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracker_clip  # noqa: E402
from online_clips import H, W, cut_from as _cut_from, grey_clip  # noqa: E402,F401


def scene_a():
    return grey_clip()


def scene_b():
    big = tracker_clip.canvas(140, 170, 77, boxes=160).astype(np.int64) - 60
    return _cut_from(np.clip(big, 0, 255).astype(np.uint8))


def one_cut():
    """M = A[:5] + B[5:]: a cut at frame 5."""
    a, b = scene_a(), scene_b()
    return np.concatenate([a[:5], b[5:]])


def two_cuts():
    """M2 = A[:3] + B[3:7] + A[7:]: cuts at frames 3 and 7."""
    a, b = scene_a(), scene_b()
    return np.concatenate([a[:3], b[3:7], a[7:]])
