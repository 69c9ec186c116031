"""The case table of the P210 crop-resize tests (tests/test_p210_model.py on the CPU, tests/test_gpu_p210_crop.py on the GPU): the frames,
rectangles and output sizes of tests/nv16_crop_cases.py -- chroma width 33, odd H, n = 9 for frame strides, 2x2, 2x35, and 640x95 to 1280x189
across three 256-sample tiles -- with random uint16 planes over 0 .. 65535.  `class_counts` says, from the model alone, how many chroma
samples of the whole table are low-clamped, high-clamped and interior in x and in y."""
import functools

import numpy as np

import nv16_crop_cases
import p210_model as model

FRAMES, NAMES = nv16_crop_cases.FRAMES, nv16_crop_cases.NAMES
rectangles, sizes = nv16_crop_cases.rectangles, nv16_crop_cases.sizes


@functools.lru_cache(maxsize=None)
def frame(name):
    """{'W', 'H', 'n', 'y', 'uv', 'cases': [(rect, size), ...]} with read-only random planes."""
    W, H, n, extra = FRAMES[NAMES.index(name)]
    rng = np.random.default_rng(2100 + NAMES.index(name))
    y = rng.integers(0, 65536, (n, H, W), dtype=np.uint16)
    uv = rng.integers(0, 65536, (n, H, W // 2, 2), dtype=np.uint16)
    y.setflags(write=False)
    uv.setflags(write=False)
    cases = [(r, s) for r in rectangles(W, H) for s in sizes(W, H, r, extra)]
    return dict(W=W, H=H, n=n, y=y, uv=uv, cases=cases)


@functools.lru_cache(maxsize=None)
def want(name, rect, size):
    """The model's (out_y, out_uv) of the whole clip for one case: computed once, shared, read-only."""
    c = frame(name)
    oy, ouv = model.crop_resize_clip(c['y'], c['uv'], rect, size)
    oy.setflags(write=False)
    ouv.setflags(write=False)
    return oy, ouv


def is_exact_2x(rect, size):
    return rect[2] - rect[0] + 1 == 2 * size[0] and rect[3] - rect[1] + 1 == 2 * size[1]


@functools.lru_cache(maxsize=None)
def class_counts():
    """{'x': (low, high, interior), 'y': (...)} summed over every case of the table."""
    tot = {'x': np.zeros(3, dtype=np.int64), 'y': np.zeros(3, dtype=np.int64)}
    for name in NAMES:
        for rect, size in frame(name)['cases']:
            tot['x'] += model.x_classes(rect[0], rect[2], size[0])
            tot['y'] += model.y_classes(rect[1], rect[3], size[1])
    return {k: tuple(int(v) for v in t) for k, t in tot.items()}
