"""The P210 warp test cases, made on the CPU after tests/nv16_cases.py, whose geometries they reuse: the synthetic ones, the three odd-H twins,
every golden with an even W and the tiny 2x2, 4x3 and 2x33 frames -- motion, the reference's maps (C oracle), random uint16 planes over
0 .. 65535, the model's result (tests/p210_model.py) -- computed once per case, shared, never changed.  Before any kernel result is looked at,
every non-tiny case is checked to hold all three classes of chroma taps under the 4:2:2 definition: border, partly outside and deep interior."""
import os

import numpy as np

import cv16_model
import nv12_cases
import nv16_cases
import p210_model

HERE = os.path.dirname(os.path.abspath(__file__))
BORDER = (4660, 51966, 300)          # no default anywhere: Y, U and V all differ, in both bytes

SYNTHETIC, TINY, NAMES = nv16_cases.SYNTHETIC, nv16_cases.TINY, nv16_cases.NAMES
_CASES = {}


def case_for(name):
    if name in _CASES:
        return _CASES[name]
    tiny = name in TINY
    if name.startswith('golden_'):
        with np.load(os.path.join(HERE, 'golden', 'warp_' + name[len('golden_'):] + '.npz')) as z:
            F, W, H, R, C = int(z['F']), int(z['width']), int(z['height']), int(z['R']), int(z['C'])
            disp, stab, seed = np.array(z['unstab'], np.float64), np.array(z['stab'], np.float64), 2100 + int(z['seed'])
    else:
        F, W, H, R, C, kind, jitter, seed = (TINY if tiny else SYNTHETIC)[name]
        disp, stab = nv12_cases._motion(F, W, H, R, C, kind, jitter, seed)
    mx, my = np.empty((F, H, W), np.float32), np.empty((F, H, W), np.float32)
    crop = np.empty((F, 4), np.int32)
    for f in range(F):
        mx[f], my[f], crop[f], bad = cv16_model.warp_maps(W, H, R, C, disp[f], stab[f])
        assert bad == 0, (name, f, bad)
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 65536, (F, H, W), dtype=np.uint16)
    uv = rng.integers(0, 65536, (F, H, W // 2, 2), dtype=np.uint16)
    cmx, cmy = p210_model.chroma_maps(mx, my)                           # (the leading frame axis passes through)
    border, partly, deep = p210_model.tap_classes(cmx, cmy, W // 2, H)
    classes = dict(border=int(border.sum()), partly=int(partly.sum()), deep=int(deep.sum()), of=int(border.size))
    if not tiny:
        assert border.any() and partly.any() and deep.any(), (name, classes, 'the case cannot fail in every class: choose another seed')
    want_y = np.stack([p210_model.remap_luma(y[f], mx[f], my[f], BORDER[0]) for f in range(F)])
    want_uv = np.stack([p210_model.remap_chroma(uv[f], cmx[f], cmy[f], BORDER[1:]) for f in range(F)])
    if not tiny:
        is_border = (want_uv == np.asarray(BORDER[1:], np.uint16)).all(axis=-1)
        assert is_border[border].all() and not is_border[partly].all()
    c = dict(name=name, tiny=tiny, F=F, W=W, H=H, R=R, C=C, disp=disp, stab=stab, mx=mx, my=my, cmx=cmx, cmy=cmy, crop=crop, y=y, uv=uv,
             want_y=want_y, want_uv=want_uv, classes=classes)
    for a in (disp, stab, mx, my, cmx, cmy, crop, y, uv, want_y, want_uv):
        a.setflags(write=False)
    _CASES[name] = c
    return c
