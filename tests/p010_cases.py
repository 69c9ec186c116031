"""The P010 test cases, made on the CPU: tests/nv12_cases.py's geometry, motion, maps, chroma maps and chroma classes (its seeds were chosen so
that every non-tiny case holds border, partly-outside and deep-interior chroma samples), with uint16 planes drawn over the whole 0 .. 65535
range -- products of 16-bit samples and 10-bit weights need 26 bits and must round; 8-bit-sized samples would hide a fused or reordered chain
-- and the model's result (tests/p010_model.py), computed once per case, shared, never changed.  Before any kernel result is looked at, every
non-tiny case is also checked to hold all three classes of LUMA samples.  (Classes of taps, as in tests/nv12_cases.py: which footprint path
produced a sample -- hot, pair, the general code; the fast or the clamped tail -- is tests/test_gpu_footprint_paths.py's business.)"""
import zlib

import numpy as np

import nv12_cases
import p010_model

BORDER = (4660, 51966, 300)         # no default anywhere: Y, U and V all differ and exceed 255
NAMES = list(nv12_cases.NAMES)
_CASES = {}


def case_for(name):
    if name in _CASES:
        return _CASES[name]
    g = nv12_cases.case_for(name)                                      # (the chroma class check is in there)
    F, W, H = g['F'], g['W'], g['H']
    border, partly, deep = p010_model.tap_classes(g['mx'], g['my'], W, H)
    luma_classes = dict(border=int(border.sum()), partly=int(partly.sum()), deep=int(deep.sum()), of=int(border.size))
    if not g['tiny']:                                                  # (every case of nv12_cases holds them: none is dropped)
        assert border.any() and partly.any() and deep.any(), (name, luma_classes, 'the case cannot fail in every luma class')
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    y = rng.integers(0, 65536, (F, H, W), dtype=np.uint16)
    uv = rng.integers(0, 65536, (F, H // 2, W // 2, 2), dtype=np.uint16)
    want_y = np.stack([p010_model.remap_luma(y[f], g['mx'][f], g['my'][f], BORDER[0]) for f in range(F)])
    want_uv = np.stack([p010_model.remap_chroma(uv[f], g['cmx'][f], g['cmy'][f], BORDER[1:]) for f in range(F)])
    cborder, cpartly, cdeep = p010_model.tap_classes(g['cmx'], g['cmy'], W // 2, H // 2)
    if not g['tiny']:
        assert (want_y[border] == BORDER[0]).all() and (want_uv[cborder] == np.asarray(BORDER[1:], np.uint16)).all()
        assert not (want_uv[cpartly] == np.asarray(BORDER[1:], np.uint16)).all()
    c = dict(g, y=y, uv=uv, want_y=want_y, want_uv=want_uv, luma_classes=luma_classes,
             luma_class=dict(border=border, partly=partly, deep=deep, other=~(border | partly | deep)),
             chroma_class=dict(border=cborder, partly=cpartly, deep=cdeep, other=~(cborder | cpartly | cdeep)))
    for a in (y, uv, want_y, want_uv, border, partly, deep, cborder, cpartly, cdeep):
        a.setflags(write=False)
    _CASES[name] = c
    return c
