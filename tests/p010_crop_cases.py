"""The case table of the P010 crop-resize tests (tests/test_p010_crop_model.py on the CPU, tests/test_gpu_p010_crop.py on the GPU): the geometry
of tests/nv12_crop_cases.py -- its frames, rectangles and output sizes -- with uint16 random planes over the full 0 .. 65,535 range.
`class_counts` says, from the model alone, how many chroma samples of the whole table are low-clamped, high-clamped and interior in x and in
y; the classes depend only on the geometry, so they are the NV12 table's."""
import functools

import numpy as np

import nv12_crop_cases as geometry
import nv12_crop_model as sites
import p010_crop_model as model

FRAMES = geometry.FRAMES
NAMES = geometry.NAMES
rectangles = geometry.rectangles
sizes = geometry.sizes


@functools.lru_cache(maxsize=None)
def frame(name):
    """{'W', 'H', 'n', 'y', 'uv', 'cases': [(rect, size), ...]} with read-only random planes."""
    W, H, n, extra = FRAMES[NAMES.index(name)]
    rng = np.random.default_rng(2000 + NAMES.index(name))
    y = rng.integers(0, 65536, (n, H, W), dtype=np.uint16)
    uv = rng.integers(0, 65536, (n, H // 2, W // 2, 2), dtype=np.uint16)
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


@functools.lru_cache(maxsize=None)
def class_counts():
    """{'x': (low, high, interior), 'y': (...)} summed over every case of the table."""
    tot = {'x': np.zeros(3, dtype=np.int64), 'y': np.zeros(3, dtype=np.int64)}
    for name in NAMES:
        for rect, size in frame(name)['cases']:
            tot['x'] += sites.axis_classes(rect[0], rect[2], size[0])
            tot['y'] += sites.axis_classes(rect[1], rect[3], size[1])
    return {k: tuple(int(v) for v in t) for k, t in tot.items()}
