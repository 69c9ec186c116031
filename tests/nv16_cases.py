"""The NV16 test cases, made on the CPU after tests/nv12_cases.py: geometry, motion, the reference's maps (C oracle), random planes, the model's
result (tests/nv16_model.py) and the luma reference -- computed once per case, shared, never changed.  Before any kernel result is looked at,
every non-tiny case is checked to hold all three classes of chroma samples under the 4:2:2 definition: border, partly outside and deep
interior.

The geometries: nv12_cases.SYNTHETIC with its seeds, three twins of them with an ODD height (4:2:2 has no rule about H), every golden with an
even W, and tiny frames (H = 1 is refused by the map oracle as degenerate: 2 is the smallest height).  The classes are classes of TAPS; the
kernel's footprint paths are counted in tests/test_gpu_nv16_paths.py."""
import glob
import os

import numpy as np

import cv16_model
import nv12_cases
import nv16_model

HERE = os.path.dirname(os.path.abspath(__file__))
BORDER = nv12_cases.BORDER         # no default anywhere: Y, U and V all differ

SYNTHETIC = dict(nv12_cases.SYNTHETIC)
SYNTHETIC.update({
    '100x71_3x5_jitter': (2, 100, 71, 3, 5, 'jitter', 6.0, 75),        # odd H; the right-edge footprint overhangs by 4 luma pixels
    '66x49_2x2_shift': (2, 66, 49, 2, 2, 'shift', 3.0, 32),            # odd H and W % 4 == 2: every chroma row starts 2-byte aligned only
    '66x49_2x2_jitter': (2, 66, 49, 2, 2, 'jitter', 5.0, 31),
})
TINY = {
    '2x2_tiny': (2, 2, 2, 1, 1, 'jitter', 0.2, 12),                    # chroma is 1 x 2: every tap's + 1 column is outside
    '4x3_tiny': (2, 4, 3, 1, 2, 'jitter', 0.2, 13),
    '2x33_tiny': (2, 2, 33, 3, 1, 'jitter', 0.3, 14),
}


def golden_names():
    """Every tests/golden/warp_*.npz geometry with an even W."""
    out = []
    for p in sorted(glob.glob(os.path.join(HERE, 'golden', 'warp_*.npz'))):
        with np.load(p) as z:
            if int(z['width']) % 2 == 0:
                out.append('golden_' + os.path.basename(p)[len('warp_'):-len('.npz')])
    return out


NAMES = list(SYNTHETIC) + golden_names() + list(TINY)
_CASES = {}


def case_for(name):
    if name in _CASES:
        return _CASES[name]
    tiny = name in TINY
    if name.startswith('golden_'):
        with np.load(os.path.join(HERE, 'golden', 'warp_' + name[len('golden_'):] + '.npz')) as z:
            F, W, H, R, C = int(z['F']), int(z['width']), int(z['height']), int(z['R']), int(z['C'])
            disp, stab, seed = np.array(z['unstab'], np.float64), np.array(z['stab'], np.float64), 1600 + int(z['seed'])
    else:
        F, W, H, R, C, kind, jitter, seed = (TINY if tiny else SYNTHETIC)[name]
        disp, stab = nv12_cases._motion(F, W, H, R, C, kind, jitter, seed)
    mx, my = np.empty((F, H, W), np.float32), np.empty((F, H, W), np.float32)
    crop = np.empty((F, 4), np.int32)
    for f in range(F):
        mx[f], my[f], crop[f], bad = cv16_model.warp_maps(W, H, R, C, disp[f], stab[f])
        assert bad == 0, (name, f, bad)
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 256, (F, H, W), dtype=np.uint8)
    uv = rng.integers(0, 256, (F, H, W // 2, 2), dtype=np.uint8)
    cmx, cmy = nv16_model.chroma_maps(mx, my)                           # (the leading frame axis passes through)
    border, partly, deep = nv16_model.tap_classes(cmx, cmy, W // 2, H)
    classes = dict(border=int(border.sum()), partly=int(partly.sum()), deep=int(deep.sum()), of=int(border.size))
    if not tiny:
        assert border.any() and partly.any() and deep.any(), (name, classes, 'the case cannot fail in every class: choose another seed')
    want_y = np.stack([nv16_model.remap_luma(y[f], mx[f], my[f], BORDER[0]) for f in range(F)])
    want_uv = np.stack([nv16_model.remap_chroma(uv[f], cmx[f], cmy[f], BORDER[1:]) for f in range(F)])
    if not tiny:
        is_border = (want_uv == np.asarray(BORDER[1:], np.uint8)).all(axis=-1)
        assert is_border[border].all() and not is_border[partly].all()
    c = dict(name=name, tiny=tiny, F=F, W=W, H=H, R=R, C=C, disp=disp, stab=stab, mx=mx, my=my, cmx=cmx, cmy=cmy, crop=crop, y=y, uv=uv,
             want_y=want_y, want_uv=want_uv, classes=classes)
    for a in (disp, stab, mx, my, cmx, cmy, crop, y, uv, want_y, want_uv):
        a.setflags(write=False)
    _CASES[name] = c
    return c
