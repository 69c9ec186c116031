"""The NV12 test cases, made on the CPU: geometry, motion, the reference's maps (C oracle), random planes, the model's result
(tests/nv12_model.py) and the luma reference -- computed once per case, shared, never changed.  Before any kernel result is looked at, every
non-tiny case is checked to hold all three classes of chroma samples: border, partly outside and deep interior.

Those are classes of TAPS.  They say nothing about which footprint path of the kernel produced a sample: the frames stop at 128 x 96 with cells
of 20 to 33 pixels under a 32-pixel footprint, so hot and pair footprints are few or absent here.  The plan classes and the tail's two forms
are counted and compared in tests/test_gpu_footprint_paths.py on tests/footprint_cases.py's geometries."""
import glob
import os

import numpy as np

import cv16_model
import nv12_model

HERE = os.path.dirname(os.path.abspath(__file__))
BORDER = (19, 203, 77)             # no default anywhere: Y, U and V all differ

# name -> (F, W, H, R, C, kind, jitter_sigma, seed); kind 'jitter': synthetic.motion's defaults plus vertex jitter, 'shift':
# translation_sigma=12 (wide border rings).  The seeds were chosen on the CPU so that the class check below holds.
SYNTHETIC = {
    '100x72_3x5_jitter': (2, 100, 72, 3, 5, 'jitter', 6.0, 75),        # the right-edge footprint overhangs by 4 luma pixels; chroma width 50
    '100x72_3x5_shift': (2, 100, 72, 3, 5, 'shift', 3.0, 76),
    '66x50_2x2_jitter': (2, 66, 50, 2, 2, 'jitter', 5.0, 31),          # W % 4 == 2: the last lane of a row holds one chroma sample
    '66x50_2x2_shift': (2, 66, 50, 2, 2, 'shift', 3.0, 32),
    '64x48_4x6_jitter': (2, 64, 48, 4, 6, 'jitter', 4.0, 51),
    '64x48_4x6_shift': (2, 64, 48, 4, 6, 'shift', 3.0, 52),
    '64x48_4x6_nine_frames': (9, 64, 48, 4, 6, 'shift', 2.0, 53),      # frame offsets beyond the first
    '128x96_32x32': (2, 128, 96, 32, 32, 'jitter', 0.3, 61),           # 4 x 3 pixel cells: the multi class, long candidate lists
}
TINY = {
    '2x2_tiny': (2, 2, 2, 1, 1, 'jitter', 0.2, 12),                    # chroma is 1 x 1: every tap's + 1 neighbour is outside
    '4x2_tiny': (2, 4, 2, 1, 2, 'jitter', 0.2, 13),
    '2x34_tiny': (2, 2, 34, 3, 1, 'jitter', 0.3, 14),
}


def golden_names():
    """Every tests/golden/warp_*.npz geometry with an even W and H."""
    out = []
    for p in sorted(glob.glob(os.path.join(HERE, 'golden', 'warp_*.npz'))):
        with np.load(p) as z:
            if int(z['width']) % 2 == 0 and int(z['height']) % 2 == 0:
                out.append('golden_' + os.path.basename(p)[len('warp_'):-len('.npz')])
    return out


NAMES = list(SYNTHETIC) + golden_names() + list(TINY)
_CASES = {}


def _motion(F, W, H, R, C, kind, jitter, seed):
    from meshflow_amd import synthetic
    from oracle import meshflow_oracle as mo
    kw = dict(translation_sigma=12.0) if kind == 'shift' else {}
    disp, hom = synthetic.motion(F, R, C, seed=seed, jitter_sigma=jitter, **kw)
    return disp, mo.stabilized_vertex_displacements(W, H, 0, disp, hom, 3, 10)


def case_for(name):
    if name in _CASES:
        return _CASES[name]
    tiny = name in TINY
    if name.startswith('golden_'):
        with np.load(os.path.join(HERE, 'golden', 'warp_' + name[len('golden_'):] + '.npz')) as z:
            F, W, H, R, C = int(z['F']), int(z['width']), int(z['height']), int(z['R']), int(z['C'])
            disp, stab, seed = np.array(z['unstab'], np.float64), np.array(z['stab'], np.float64), 900 + int(z['seed'])
    else:
        F, W, H, R, C, kind, jitter, seed = (TINY if tiny else SYNTHETIC)[name]
        disp, stab = _motion(F, W, H, R, C, kind, jitter, seed)
    mx, my = np.empty((F, H, W), np.float32), np.empty((F, H, W), np.float32)
    crop = np.empty((F, 4), np.int32)
    for f in range(F):
        mx[f], my[f], crop[f], bad = cv16_model.warp_maps(W, H, R, C, disp[f], stab[f])
        assert bad == 0, (name, f, bad)
    rng = np.random.default_rng(seed)
    y = rng.integers(0, 256, (F, H, W), dtype=np.uint8)
    uv = rng.integers(0, 256, (F, H // 2, W // 2, 2), dtype=np.uint8)
    cmaps = [nv12_model.chroma_maps(mx[f], my[f]) for f in range(F)]
    cmx, cmy = np.stack([m[0] for m in cmaps]), np.stack([m[1] for m in cmaps])
    border, partly, deep = nv12_model.tap_classes(cmx, cmy, W // 2, H // 2)
    classes = dict(border=int(border.sum()), partly=int(partly.sum()), deep=int(deep.sum()), of=int(border.size))
    if not tiny:
        assert border.any() and partly.any() and deep.any(), (name, classes, 'the case cannot fail in every class: choose another seed')
    want_y = np.stack([nv12_model.remap_luma(y[f], mx[f], my[f], BORDER[0]) for f in range(F)])
    want_uv = np.stack([nv12_model.remap_chroma(uv[f], cmx[f], cmy[f], BORDER[1:]) for f in range(F)])
    if not tiny:
        is_border = (want_uv == np.asarray(BORDER[1:], np.uint8)).all(axis=-1)
        assert is_border[border].all() and not is_border[partly].all()
    c = dict(name=name, tiny=tiny, F=F, W=W, H=H, R=R, C=C, disp=disp, stab=stab, mx=mx, my=my, cmx=cmx, cmy=cmy, crop=crop, y=y, uv=uv,
             want_y=want_y, want_uv=want_uv, classes=classes)
    for a in (disp, stab, mx, my, cmx, cmy, crop, y, uv, want_y, want_uv):
        a.setflags(write=False)
    _CASES[name] = c
    return c
