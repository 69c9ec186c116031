"""The case table of the NV16 crop-resize tests (tests/test_nv16_crop_model.py on the CPU, tests/test_gpu_nv16_crop.py on the GPU): frames of
random planes, and for each its rectangles and output sizes.  `class_counts` says, from the model alone, how many chroma samples of the whole
table are low-clamped, high-clamped and interior in x and in y."""
import functools

import numpy as np

import nv16_crop_model as model

# (W, H, n, extra output sizes): chroma width 33 (a row end narrower than a lane) and an odd H; frame offsets beyond the first; a plain one with
# an odd H; chroma 1 x 2; a frame two pixels wide; and 640 x 95 to 1280 x 189: chroma rows of 640 samples spanning three 256-sample tiles
FRAMES = [(66, 49, 2, ()), (64, 48, 9, ()), (100, 71, 2, ()), (2, 2, 2, ()), (2, 35, 2, ()), (640, 95, 2, ((1280, 189),))]
NAMES = ['%dx%d' % (W, H) for W, H, _, _ in FRAMES]


def even(v):
    return max(2, int(v) // 2 * 2)


def odd(v):
    return max(3, int(v) // 2 * 2 + 1)


def rectangles(W, H):
    """The full frame; all four parities of (left, top) crossed with even and odd right / bottom; one pixel at an odd position; one pixel at
    the frame's last column and row; rectangles ending on the last column and row.  Only those that lie in the frame, each once."""
    rects = [(0, 0, W - 1, H - 1)]
    for left in (2, 3):
        for top in (2, 3):
            for right in (W - 4, W - 3):
                for bottom in (H - 4, H - 3):
                    rects.append((left, top, right, bottom))
    rects += [(5, 7, 5, 7), (1, 1, 1, 1), (W - 1, H - 1, W - 1, H - 1), (3, 2, W - 1, H - 1), (1, 1, W - 1, H - 1), (0, 1, W - 1, H - 2)]
    seen = []
    for r in rects:
        if 0 <= r[0] <= r[2] < W and 0 <= r[1] <= r[3] < H and r not in seen:
            seen.append(r)
    return seen


def sizes(W, H, rect, extra=()):
    """The frame's size; the crop's own where its width is even; an odd height; up, non-integer; exactly 2x down where the crop allows it;
    more than 4x down; 2 x 2; 2 x 3."""
    cw, ch = rect[2] - rect[0] + 1, rect[3] - rect[1] + 1
    out = [(W, H)]
    if cw % 2 == 0 and ch >= 2:
        out.append((cw, ch))
    out.append((even(cw * 0.8 + 2), odd(ch * 1.2)))
    out.append((even(cw * 1.37 + 2), int(ch * 1.61 + 2)))
    if cw % 4 == 0 and ch % 2 == 0 and ch >= 4:
        out.append((cw // 2, ch // 2))
    out += [(even(cw / 4.6), max(2, int(ch / 5.3))), (2, 2), (2, 3)]
    out += list(extra)
    seen = []
    for s in out:
        if s not in seen:
            seen.append(s)
    return seen


@functools.lru_cache(maxsize=None)
def frame(name):
    """{'W', 'H', 'n', 'y', 'uv', 'cases': [(rect, size), ...]} with read-only random planes."""
    W, H, n, extra = FRAMES[NAMES.index(name)]
    rng = np.random.default_rng(1600 + NAMES.index(name))
    y = rng.integers(0, 256, (n, H, W), dtype=np.uint8)
    uv = rng.integers(0, 256, (n, H, W // 2, 2), dtype=np.uint8)
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
            tot['x'] += model.x_classes(rect[0], rect[2], size[0])
            tot['y'] += model.y_classes(rect[1], rect[3], size[1])
    return {k: tuple(int(v) for v in t) for k, t in tot.items()}
