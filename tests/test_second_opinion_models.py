"""The oracle and the uint16 models before the independent torch reference of tests/second_opinion.py, on the CPU: every true model inside
the envelope with the constants of that module, and every deliberately wrong model rejected with the same constants.  The HIP kernels equal
these models bit for bit (the -m gpu suites), so a bound the models meet here is a bound the kernels meet; tests/test_gpu_torch_crosscheck.py
runs the same judge on the kernels.

Models: u8c3 through the C oracle (oracle.clib.warp_clip) and oracle.meshflow_oracle.resize_linear_u8; u16c3 through tests/cv16_model.py and
tests/cv16_area.py; u8c1 as channel 0 of the u8c3 result of the frame repeated three times; u8c4 as the u8c3 result of B G R beside the
u8c1 result of the alpha plane -- the derivations of the GPU suites.  The chroma planes of NV12 and P010 (second half of this file) through
tests/nv12_model.py, p010_model.py, nv12_crop_model.py and p010_crop_model.py, judged at positions second_opinion.py computes for itself.

The wrong models are the NumPy models themselves with one statement changed (a patched function or a changed argument): nothing here
touches a kernel."""
import numpy as np
import pytest

import cv16_area
import cv16_model
import second_opinion as so
from oracle import clib
from oracle import meshflow_oracle as mo

torch = pytest.importorskip('torch')

PLANES = {'smooth': so.smooth_planes, 'noise': so.noise_planes}


# ---- the true models ------------------------------------------------------------------------------------------------------------------

def _alpha_of(border):
    return border[3] if len(border) > 3 else 0


def model_warp(fmt, fr, R, C, unstab, stab, border):
    if fmt == 'u16c3':
        return cv16_model.warp_clip_u16(fr, R, C, unstab, stab, border)[0]
    if fmt == 'u8c3':
        out, _, bad = clib.warp_clip(fr, R, C, unstab, stab, border)
    elif fmt == 'u8c1':
        out, _, bad = clib.warp_clip(np.repeat(fr[..., None], 3, axis=-1), R, C, unstab, stab, (border[0],) * 3)
        out = out[..., 0]
    else:
        out, _, bad = clib.warp_clip(np.ascontiguousarray(fr[..., :3]), R, C, unstab, stab, tuple(border[:3]))
        alpha = clib.warp_clip(np.repeat(fr[..., 3:], 3, axis=-1), R, C, unstab, stab, (_alpha_of(border),) * 3)[0]
        out = np.concatenate([out, alpha[..., :1]], axis=-1)
    assert bad == 0
    return out


def numpy_warp(fmt, fr, R, C, unstab, stab, border, map_shift=0.0):
    """The same results from the NumPy remap models on the C oracle's float32 maps -- the form the wrong models below are made from."""
    H, W = fr.shape[1:3]
    out = []
    for f in range(fr.shape[0]):
        mx, my, _, bad = cv16_model.warp_maps(W, H, R, C, unstab[f], stab[f])
        assert bad == 0
        mx, my = mx + np.float32(map_shift), my + np.float32(map_shift)
        if fmt == 'u16c3':
            out.append(cv16_model.remap_bilinear_u16c3(fr[f], mx, my, border))
        elif fmt == 'u8c3':
            out.append(mo.remap_bilinear_u8c3(fr[f], mx, my, border))
        elif fmt == 'u8c1':
            out.append(mo.remap_bilinear_u8c3(np.repeat(fr[f][..., None], 3, axis=-1), mx, my, (border[0],) * 3)[..., 0])
        else:
            alpha = mo.remap_bilinear_u8c3(np.repeat(fr[f][..., 3:], 3, axis=-1), mx, my, (_alpha_of(border),) * 3)
            out.append(np.concatenate([mo.remap_bilinear_u8c3(fr[f][..., :3], mx, my, tuple(border[:3])), alpha[..., :1]], axis=-1))
    return np.stack(out)


def model_resize(fmt, fr, rect, ow, oh):
    l, t, r, b = rect
    out = []
    for f in fr:
        crop = f[t:b + 1, l:r + 1]
        if fmt == 'u8c3':
            out.append(mo.resize_linear_u8(crop, ow, oh))
        elif fmt == 'u8c1':
            out.append(mo.resize_linear_u8(np.repeat(crop[..., None], 3, axis=2), ow, oh)[..., 0])
        elif fmt == 'u8c4':
            alpha = mo.resize_linear_u8(np.repeat(crop[..., 3:], 3, axis=2), ow, oh)[..., :1]
            out.append(np.concatenate([mo.resize_linear_u8(np.ascontiguousarray(crop[..., :3]), ow, oh), alpha], axis=-1))
        else:
            out.append(cv16_area.resize_u16(crop, ow, oh))
    return np.stack(out)


def warp_case_findings(fmt, case, kind, warp=model_warp, border=(0, 0, 0), eps=None, allow=None):
    """[(findings, violations)] of every setup of one case, the result computed by `warp`."""
    planes = PLANES[kind](fmt, case.n, case.H, case.W, case.seed)
    out = []
    for setup in so.warp_setups(case):
        got = so.to_planes(warp(fmt, so.to_numpy(fmt, planes), case.R, case.C, setup.unstab, setup.stab, border))
        f = so.warp_findings(fmt, got, planes, setup, border, eps, allow)
        out.append((f, so.warp_violations(fmt, f, setup, kind == 'smooth')))
    return out


def resize_case_findings(fmt, case, kind, resize=model_resize, eps=None, allow=None):
    n, H, W, rect, (ow, oh) = case
    planes = PLANES[kind](fmt, n, H, W, 9)
    got = so.to_planes(resize(fmt, so.to_numpy(fmt, planes), rect, ow, oh))
    assert tuple(got.shape[:3]) == (n, oh, ow)
    f = so.resize_findings(fmt, got, planes, rect, ow, oh, eps, allow)
    return f, so.resize_violations(fmt, f, rect, ow, oh, kind == 'smooth')


def _violations(found):
    return [v for _, vs in found for v in vs]


# ---- every true model is inside -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['smooth', 'noise'])
@pytest.mark.parametrize('fmt', so.FORMATS)
@pytest.mark.parametrize('case', so.WARP_CASES, ids=lambda c: f'{c.kind}-{c.H}x{c.W}')
def test_warp_models_are_inside(case, fmt, kind):
    """Identity and integer shifts exact; one global homography within the envelope on all but the border ring (>= 97 % judged); real mesh
    motion on cell interiors (>= 60 %); on smooth uint16 frames shifted by multiples of 1/32 px the mean signed difference within 3
    standard errors of zero."""
    found = warp_case_findings(fmt, case, kind)
    assert not _violations(found), found


@pytest.mark.parametrize('fmt', so.FORMATS)
def test_borders(fmt):
    """A non-black border per format on a wide uncovered band: far outside the mesh the output is the border exactly, everywhere else the
    shifted frame exactly.  uint16 with (0, 0, 255) gives 255, not 65,535; u8c4 with a 3-component border gives alpha 0, with 4 components
    that alpha."""
    case = next(c for c in so.WARP_CASES if c.kind == 'far')
    borders = [so.BORDERS[fmt]] + ([so.BORDERS['u8c4'][:3]] if fmt == 'u8c4' else [])
    for border in borders:
        found = warp_case_findings(fmt, case, 'smooth', border=border)
        assert not _violations(found), found
        assert found[0][0]['far_pixels'] > 1000
    planes = so.smooth_planes(fmt, case.n, case.H, case.W, case.seed)
    setup = next(so.warp_setups(case))
    out = model_warp(fmt, so.to_numpy(fmt, planes), case.R, case.C, setup.unstab, setup.stab, borders[-1])
    corner = out[0, -1, 0]                                               # FAR_SHIFT uncovers the bottom left corner
    want = {'u8c3': [11, 122, 233], 'u16c3': [0, 0, 255], 'u8c1': 77, 'u8c4': [11, 122, 233, 0]}[fmt]
    assert np.array_equal(corner, want), corner
    # a homography, so that border taps are blended into the judged pixels next to the ring as well
    hom = next(c for c in so.WARP_CASES if c.kind == 'homography')
    found = warp_case_findings(fmt, hom, 'smooth', border=so.BORDERS[fmt])
    assert not _violations(found), found


@pytest.mark.parametrize('kind', ['smooth', 'noise'])
@pytest.mark.parametrize('fmt', so.FORMATS)
@pytest.mark.parametrize('case', range(len(so.RESIZE_CASES)))
def test_resize_models_are_inside(case, fmt, kind):
    f, violations = resize_case_findings(fmt, so.RESIZE_CASES[case], kind)
    assert not violations, (f, violations)


@pytest.mark.parametrize('fmt', so.FORMATS)
def test_same_size_resize_models_are_inside(fmt):
    for n, H, W, rect in so.SAME_SIZE_CASES:
        for kind in ('smooth', 'noise'):
            f, violations = resize_case_findings(fmt, (n, H, W, rect, (W, H)), kind)
            assert not violations, (f, violations)


LARGE = [c for c in so.WARP_CASES_1080P if c.kind == 'homography']


@pytest.mark.parametrize('case,fmt,kind', [(c, 'u16c3', k) for c in LARGE for k in ('smooth', 'noise')] + [(LARGE[0], 'u8c3', 'noise')],
                         ids=lambda v: f'{v.R}x{v.C}' if isinstance(v, so.WarpCase) else v)
def test_warp_models_are_inside_at_1080p(case, fmt, kind):
    """The float32 coordinate error grows with the coordinates, so the bounds are proven at the largest size the device suite judges, here,
    before any kernel is: uint16 (the one format with a slack) on both meshes, and the 8-bit warp on noise (u8c1 and u8c4 are made of it)."""
    found = warp_case_findings(fmt, case, kind)
    assert not _violations(found), found


@pytest.mark.parametrize('fmt', ['u16c3', 'u8c4'])
@pytest.mark.parametrize('case', range(len(so.RESIZE_CASES_1080P)))
def test_resize_models_are_inside_at_1080p(case, fmt):
    f, violations = resize_case_findings(fmt, so.RESIZE_CASES_1080P[case], 'noise')
    assert not violations, (f, violations)
    n, H, W, rect = so.SAME_SIZE_CASES_1080P[0]
    if case == 0:
        f, violations = resize_case_findings(fmt, (n, H, W, rect, (W, H)), 'noise')
        assert not violations, (f, violations)


def test_the_resize_case_list_is_the_device_suite_s():
    """RESIZE_CASES restates tests/test_gpu_crop_resize_to.py's CASES (that module cannot be imported without the built package)."""
    import ast
    import os
    with open(os.path.join(os.path.dirname(__file__), 'test_gpu_crop_resize_to.py')) as fh:
        tree = ast.parse(fh.read())
    cases = next(n.value for n in tree.body if isinstance(n, ast.Assign) and getattr(n.targets[0], 'id', None) == 'CASES')
    assert ast.literal_eval(cases) == so.RESIZE_CASES


# ---- proof that the judge can fail: wrong models, the same constants ----------------------------------------------------------------------

HOMOGRAPHY = next(c for c in so.WARP_CASES if c.kind == 'homography')
THIRTYSECONDS = next(c for c in so.WARP_CASES if c.kind == 'thirtyseconds')
FAR = next(c for c in so.WARP_CASES if c.kind == 'far')
UP, DOWN = so.RESIZE_CASES[0], so.RESIZE_CASES[1]
# the frames on which each format resolves a coordinate error: uint8 smooth frames move 3 levels per pixel, so 1/64 px is 0.05 LSB -- only
# noise shows it; uint16 smooth frames move 800 LSB per pixel
SHARP = {'u8c3': 'noise', 'u16c3': 'smooth', 'u8c1': 'noise', 'u8c4': 'noise'}


@pytest.mark.parametrize('fmt', so.FORMATS)
def test_the_numpy_form_is_the_model(fmt):
    """The control of the wrong models below: unchanged, the NumPy form gives the model's result, sample for sample."""
    planes = so.noise_planes(fmt, HOMOGRAPHY.n, HOMOGRAPHY.H, HOMOGRAPHY.W, 1)
    s = next(so.warp_setups(HOMOGRAPHY))
    args = (fmt, so.to_numpy(fmt, planes), HOMOGRAPHY.R, HOMOGRAPHY.C, s.unstab, s.stab, so.BORDERS[fmt])
    assert np.array_equal(numpy_warp(*args), model_warp(*args))


@pytest.mark.parametrize('fmt', so.FORMATS)
def test_rejects_a_half_pixel_shift_of_the_warp_map(fmt):
    for kind in ('smooth', 'noise'):
        wrong = lambda *a: numpy_warp(*a, map_shift=0.5)                 # noqa: E731
        assert _violations(warp_case_findings(fmt, HOMOGRAPHY, kind, wrong)), kind


@pytest.mark.parametrize('fmt', so.FORMATS)
def test_rejects_the_inverted_map_direction(fmt):
    """Sampling at G x instead of G^-1 x: the model with its two vertex sets exchanged."""
    wrong = lambda fmt, fr, R, C, unstab, stab, border: numpy_warp(fmt, fr, R, C, stab, unstab, border)      # noqa: E731
    for kind in ('smooth', 'noise'):
        assert _violations(warp_case_findings(fmt, HOMOGRAPHY, kind, wrong)), kind


@pytest.mark.parametrize('fmt', so.FORMATS)
def test_rejects_the_coordinate_bucket_by_floor(fmt, monkeypatch):
    """floor(32 x) instead of round(32 x): a mean shift of 1/64 px, at most 1/32."""
    monkeypatch.setattr(mo, '_cv_round_f32', lambda v: np.floor(v.astype(np.float64)).astype(np.int64))
    assert _violations(warp_case_findings(fmt, HOMOGRAPHY, SHARP[fmt], numpy_warp))


@pytest.mark.parametrize('fmt', so.FORMATS)
def test_rejects_align_corners_resize(fmt, monkeypatch):
    """Pixel centres at the corners: source position d (src - 1) / (dst - 1) instead of (d + 0.5) src / dst - 0.5."""
    def tables(src_len, dst_len):
        f = (np.arange(dst_len, dtype=np.float64) * ((src_len - 1) / max(dst_len - 1, 1))).astype(np.float32)
        s = np.floor(f).astype(np.int64)
        return s, (f - s.astype(np.float32)).astype(np.float32)
    monkeypatch.setattr(mo, 'resize_linear_tables', tables)
    for case in (UP, DOWN):
        for kind in ('smooth', 'noise'):
            assert resize_case_findings(fmt, case, kind)[1], (case, kind)


def test_rejects_uint16_truncation_by_the_mean(monkeypatch):
    """saturate_cast by truncation: the mean half an LSB low.  The mean signed difference catches it in the warp and in the resize, wherever
    the frame moves enough per pixel that the envelope alone would not."""
    monkeypatch.setattr(cv16_model, 'saturate_u16', lambda t: np.clip(np.floor(t.astype(np.float64)), 0, 65535).astype(np.uint16))
    (f, violations), = warp_case_findings('u16c3', THIRTYSECONDS, 'smooth', numpy_warp)
    assert -0.55 < f['mean_signed'] < -0.45 and any('mean signed' in v for v in violations), (f, violations)
    f, violations = resize_case_findings('u16c3', so.RESIZE_CASES[11], 'smooth')
    assert -0.55 < f['mean_signed'] < -0.45 and any('mean signed' in v for v in violations), (f, violations)


def test_rejects_the_uint16_border_scaled_to_16_bits():
    wrong = lambda fmt, fr, R, C, unstab, stab, border: numpy_warp(fmt, fr, R, C, unstab, stab, tuple(257 * b for b in border))   # noqa: E731
    (f, violations), = warp_case_findings('u16c3', FAR, 'smooth', wrong, border=so.BORDERS['u16c3'])
    assert f['far_bad'] > 0 and violations, f


@pytest.mark.parametrize('op', ['warp', 'resize'])
def test_rejects_wrong_channels(op):
    """Channel 3 of u8c4 taken from channel 0; channels 0 and 2 exchanged (every multi-channel format)."""
    def alpha_from_blue(a):
        a = a.copy()
        a[..., 3] = a[..., 0]
        return a
    wrongs = [('u8c4', alpha_from_blue)] + [(fmt, lambda a: np.ascontiguousarray(a[..., [2, 1, 0] + [3] * (a.shape[-1] - 3)])) for fmt in ('u8c3', 'u16c3', 'u8c4')]
    for fmt, wrong in wrongs:
        if op == 'warp':
            assert _violations(warp_case_findings(fmt, HOMOGRAPHY, 'smooth', lambda *a: wrong(model_warp(*a)))), fmt
        else:
            assert resize_case_findings(fmt, DOWN, 'smooth', lambda *a: wrong(model_resize(*a)))[1], fmt


# ---- 4:2:0: the chroma planes of the NV12 and P010 models -------------------------------------------------------------------------------
# Luma needs no proof of its own: NV12 luma is the u8c1 model above and P010 luma channel 0 of the u16c3 model, bit for bit (the device
# suites assert both).  The wrong models are again the true ones with one statement changed.

import nv12_crop_model  # noqa: E402
import nv12_model  # noqa: E402
import p010_crop_model  # noqa: E402
import p010_model  # noqa: E402

WARP_420 = {'nv12': nv12_model, 'p010': p010_model}
CROP_420 = {'nv12': nv12_crop_model, 'p010': p010_crop_model}
_MAPS = {}


def _maps(case, setup, f):
    """The reference's float32 maps of one frame of one setup, computed once."""
    key = (case, setup.label, f)
    if key not in _MAPS:
        mx, my, _, bad = cv16_model.warp_maps(case.W, case.H, case.R, case.C, setup.unstab[f], setup.stab[f])
        assert bad == 0
        _MAPS[key] = (mx, my)
    return _MAPS[key]


def model_warp_420(fmt, y, uv, case, setup, border, chroma_maps=nv12_model.chroma_maps, chroma_border=lambda b: b[1:3]):
    """(out_y or None, out_uv) of the model; y None: chroma alone."""
    m = WARP_420[fmt]
    out_y, out_uv = [], []
    for f in range(case.n):
        mx, my = _maps(case, setup, f)
        if y is not None:
            out_y.append(m.remap_luma(y[f], mx, my, border[0]))
        out_uv.append(m.remap_chroma(uv[f], *chroma_maps(mx, my), chroma_border(border)))
    return (np.stack(out_y) if out_y else None), np.stack(out_uv)


def model_resize_420(fmt, y, uv, rect, size):
    return CROP_420[fmt].crop_resize_clip(y, uv, rect, size)


def chroma_warp_findings(fmt, case, kind, border=None, wrong=lambda a: a, **model_args):
    """[(findings, violations)] of the model's warped chroma plane for every setup of one case."""
    cf = so.CHROMA_OF[fmt]
    border = so.BORDERS_YUV[fmt] if border is None else border
    _, uv = so.planes_420(fmt, kind, case.n, case.H, case.W, case.seed)
    out = []
    for setup in so.warp_setups(case):
        cs = so.chroma_setup(setup, case.H, case.W)
        got = so.to_planes(wrong(model_warp_420(fmt, None, so.to_numpy(cf, uv), case, setup, border, **model_args)[1]))
        f = so.warp_findings(cf, got, uv, cs, border[1:])
        out.append((f, so.warp_violations(cf, f, cs, kind == 'smooth')))
    return out


def chroma_resize_findings(fmt, case, kind, resize=None):
    cf = so.CHROMA_OF[fmt]
    n, H, W, rect, (ow, oh) = case
    _, uv = so.planes_420(fmt, kind, n, H, W, 9)
    resize = resize or (lambda a, rect, size: np.stack([CROP_420[fmt].crop_resize_chroma(p, rect, size) for p in a]))
    got = so.to_planes(resize(so.to_numpy(cf, uv), rect, (ow, oh)))
    assert tuple(got.shape) == (n, oh // 2, ow // 2, 2)
    f = so.resize_chroma_findings(cf, got, uv, rect, ow, oh)
    return f, so.resize_violations(cf, f, rect, ow, oh, kind == 'smooth')


@pytest.mark.parametrize('kind', ['smooth', 'noise'])
@pytest.mark.parametrize('fmt', so.FORMATS_420)
@pytest.mark.parametrize('case', so.WARP_CASES_420, ids=lambda c: f'{c.kind}-{c.H}x{c.W}')
def test_warp_chroma_models_are_inside(case, fmt, kind):
    """Identity and shifts even in both axes exact; odd shifts (half a chroma pixel), a global homography and mesh motion inside the
    envelope of the chroma plane, with a (Y, U, V) border whose components all differ; P010 chroma shifted by sixteenths of a luma pixel
    has a mean signed difference within 3 standard errors of zero."""
    found = chroma_warp_findings(fmt, case, kind)
    assert not _violations(found), found
    labels = {f['label']: s for (f, _), s in zip(found, (so.chroma_setup(s, case.H, case.W) for s in so.warp_setups(case)))}
    if case.kind == 'shift':
        assert [labels[f'shift{s}'].exact for s in so.INTEGER_SHIFTS] == [False, True]
    if case.kind == 'far':
        assert found[0][0]['far_pixels'] > 250 and not labels[f'far{so.FAR_SHIFT}'].exact


@pytest.mark.parametrize('fmt', so.FORMATS_420)
def test_the_thirtyseconds_shift_is_a_rounding_tie_for_chroma(fmt):
    """Why chroma has a mean-signed case of its own: (5 7/32, -3 11/32) halves to odd multiples of 1/64 chroma px, every one on a tie of
    the 1/32 bucket, and the TRUE P010 model's chroma mean is a quarter LSB off; the sixteenths shift halves to multiples of 1/32."""
    assert all((64 * s / 2) % 2 == 1 for s in so.THIRTYSECONDS_SHIFT) and all((32 * s / 2) % 1 == 0 for s in so.SIXTEENTHS_SHIFT)
    if fmt == 'p010':
        (f, violations), = chroma_warp_findings(fmt, THIRTYSECONDS, 'smooth')
        assert not violations and abs(f['mean_signed']) > 0.1, f


@pytest.mark.parametrize('case,fmt,kind', [(LARGE[0], 'p010', 'smooth'), (LARGE[0], 'p010', 'noise'), (LARGE[1], 'p010', 'noise'), (LARGE[0], 'nv12', 'noise')],
                         ids=lambda v: f'{v.R}x{v.C}' if isinstance(v, so.WarpCase) else v)
def test_warp_chroma_models_are_inside_at_1080p(case, fmt, kind):
    """P010 is the format with a slack: both 1080p meshes, where the float32 coordinate error is largest; NV12 on noise."""
    found = chroma_warp_findings(fmt, case, kind)
    assert not _violations(found), found


@pytest.mark.parametrize('kind', ['smooth', 'noise'])
@pytest.mark.parametrize('fmt', so.FORMATS_420)
@pytest.mark.parametrize('case', range(len(so.RESIZE_CASES_420)))
def test_resize_chroma_models_are_inside(case, fmt, kind):
    f, violations = chroma_resize_findings(fmt, so.RESIZE_CASES_420[case], kind)
    assert not violations, (f, violations)


@pytest.mark.parametrize('fmt', so.FORMATS_420)
def test_resize_chroma_models_are_inside_at_1080p_and_same_size(fmt):
    cases = so.RESIZE_CASES_1080P + [(n, H, W, rect, (W, H)) for n, H, W, rect in so.SAME_SIZE_CASES + so.SAME_SIZE_CASES_1080P]
    for case in cases:
        for kind in ('smooth', 'noise'):
            f, violations = chroma_resize_findings(fmt, case, kind)
            assert not violations, (case, kind, f, violations)


def test_the_420_resize_table_crosses_every_parity():
    rects = [c[3] for c in so.RESIZE_CASES_420 if c[1:3] == (72, 100)]
    assert {tuple(v % 2 for v in r) for r in rects if r[2] - r[0] > 1} >= {(a, b, c, d) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)}
    assert (37, 21, 37, 21) in rects and (99, 71, 99, 71) in rects
    assert all(H % 2 == 0 and W % 2 == 0 and ow % 2 == 0 and oh % 2 == 0 for _, H, W, _, (ow, oh) in so.RESIZE_CASES_420)
    assert len(so.RESIZE_CASES_420) == len(so.RESIZE_CASES) + 20


# ---- wrong 4:2:0 models, the same constants --------------------------------------------------------------------------------------------

SHARP_420 = {'nv12': 'noise', 'p010': 'smooth'}
HALF = np.float32(0.5)


def odd_sited_maps(mx, my):
    return mx[1::2, 1::2] * HALF, my[1::2, 1::2] * HALF


def quarter_pixel_maps(mx, my):
    cmx, cmy = nv12_model.chroma_maps(mx, my)
    return cmx + np.float32(0.25), cmy + np.float32(0.25)


def unhalved_maps(mx, my):
    return np.ascontiguousarray(mx[::2, ::2]), np.ascontiguousarray(my[::2, ::2])


@pytest.mark.parametrize('fmt', so.FORMATS_420)
@pytest.mark.parametrize('maps', [odd_sited_maps, quarter_pixel_maps, unhalved_maps], ids=lambda m: m.__name__)
def test_rejects_wrong_chroma_maps(fmt, maps):
    """Chroma sited at the odd luma sample (half a chroma pixel off), a quarter-pixel correction, maps not halved."""
    for kind in ('smooth', 'noise'):
        found = chroma_warp_findings(fmt, HOMOGRAPHY, kind, chroma_maps=maps)
        assert _violations(found), (kind, found)


@pytest.mark.parametrize('fmt', so.FORMATS_420)
def test_rejects_u_and_v_exchanged(fmt):
    for kind in ('smooth', 'noise'):
        assert _violations(chroma_warp_findings(fmt, HOMOGRAPHY, kind, wrong=lambda a: np.ascontiguousarray(a[..., ::-1]))), kind
        n, H, W, rect, size = DOWN
        f, violations = chroma_resize_findings(fmt, (n, H, W, rect, (so._even(size[0]), so._even(size[1]))), kind,
                                               lambda a, rect, size: np.stack([CROP_420[fmt].crop_resize_chroma(p, rect, size)[..., ::-1] for p in a]))
        assert violations, (kind, f)


@pytest.mark.parametrize('fmt', so.FORMATS_420)
def test_rejects_the_chroma_bucket_by_floor(fmt, monkeypatch):
    monkeypatch.setattr(mo, '_cv_round_f32', lambda v: np.floor(v.astype(np.float64)).astype(np.int64))
    assert _violations(chroma_warp_findings(fmt, HOMOGRAPHY, SHARP_420[fmt]))


def test_rejects_p010_chroma_truncation_by_the_mean(monkeypatch):
    monkeypatch.setattr(cv16_model, 'saturate_u16', lambda t: np.clip(np.floor(t.astype(np.float64)), 0, 65535).astype(np.uint16))
    (f, violations), = chroma_warp_findings('p010', so.WARP_CASES_420[-1], 'smooth')
    assert -0.55 < f['mean_signed'] < -0.45 and any('mean signed' in v for v in violations), (f, violations)


@pytest.mark.parametrize('fmt', so.FORMATS_420)
def test_rejects_the_chroma_border_taken_from_y(fmt):
    found = chroma_warp_findings(fmt, FAR, 'smooth', chroma_border=lambda b: (b[0], b[0]))
    assert found[0][0]['far_bad'] > 0 and _violations(found), found
    # and blended into the edge samples of a homography
    assert _violations(chroma_warp_findings(fmt, HOMOGRAPHY, 'smooth', chroma_border=lambda b: (b[0], b[0])))


def plain_resize_of_the_halved_crop(fmt):
    """The plane cropped at left >> 1 .. right >> 1 and resized plainly: parity ignored."""
    def resize(a, rect, size):
        l, t, r, b = (v >> 1 for v in rect)
        crop = a[:, t:b + 1, l:r + 1]
        if fmt == 'nv12':
            three = np.concatenate([crop, crop[..., :1]], axis=-1)
            return np.stack([mo.resize_linear_u8(p, size[0] // 2, size[1] // 2)[..., :2] for p in three])
        return np.stack([cv16_model.resize_linear_u16(p, size[0] // 2, size[1] // 2) for p in crop])
    return resize


@pytest.mark.parametrize('fmt', so.FORMATS_420)
def test_rejects_the_crop_that_ignores_parity(fmt):
    assert so.PARITY_CASE_420[3][0] % 2 == 1 and so.PARITY_CASE_420[3][1] % 2 == 1
    f, violations = chroma_resize_findings(fmt, so.PARITY_CASE_420, SHARP_420[fmt], plain_resize_of_the_halved_crop(fmt))
    assert violations, f


@pytest.mark.parametrize('fmt', so.FORMATS_420)
def test_rejects_align_corners_chroma_resize(fmt, monkeypatch):
    def positions(lo, hi, out_len):
        c0, c1 = nv12_crop_model.axis_range(lo, hi)
        fc = (c0 + np.arange(out_len // 2, dtype=np.float64) * ((c1 - c0) / max(out_len // 2 - 1, 1))).astype(np.float32)
        s = np.floor(fc).astype(np.int64)
        return s, (fc - s.astype(np.float32)).astype(np.float32)
    monkeypatch.setattr(nv12_crop_model, 'axis_positions', positions)
    for case in (so.RESIZE_CASES_420[0], so.RESIZE_CASES_420[1]):
        assert chroma_resize_findings(fmt, case, SHARP_420[fmt])[1], case


@pytest.mark.parametrize('fmt', so.FORMATS_420)
def test_rejects_a_chroma_clamp_range_one_sample_too_wide(fmt, monkeypatch):
    true_range = nv12_crop_model.axis_range
    monkeypatch.setattr(nv12_crop_model, 'axis_range', lambda lo, hi: (max(true_range(lo, hi)[0] - 1, 0), true_range(lo, hi)[1] + 1))
    assert chroma_resize_findings(fmt, so.PARITY_CASE_420, 'noise')[1]


# ---- registration of chroma on luma: the ramp ----------------------------------------------------------------------------------------------

def ramp_warp_gap(fmt, **model_args):
    case = so.REGISTRATION_WARP[fmt]
    y, uv = so.ramp_420(fmt, case.n, case.H, case.W)
    setup = next(so.warp_setups(case))
    got_y, got_uv = model_warp_420(fmt, so.to_numpy(so.LUMA_OF[fmt], y), so.to_numpy(so.CHROMA_OF[fmt], uv), case, setup, so.BORDERS_YUV[fmt],
                                   **model_args)
    return so.registration_warp(fmt, so.to_planes(got_y), so.to_planes(got_uv), setup)


@pytest.mark.parametrize('fmt', so.FORMATS_420)
def test_ramp_registration_of_the_models(fmt):
    """On a linear ramp chroma and the luma of its even pixel are the same number whatever the warp or the crop: the true models within
    the derived bound; chroma sited at the odd sample or corrected by a quarter pixel outside it, in both formats."""
    worst, compared, bound = ramp_warp_gap(fmt)
    print(fmt, 'warp', worst, compared, bound)
    assert worst <= bound and compared > 0.8 * so.REGISTRATION_WARP[fmt].n * so.REGISTRATION_WARP[fmt].H * so.REGISTRATION_WARP[fmt].W / 4
    for maps in (odd_sited_maps, quarter_pixel_maps):
        wrong, _, _ = ramp_warp_gap(fmt, chroma_maps=maps)
        print(fmt, maps.__name__, wrong)
        assert wrong > bound, maps.__name__
    n, H, W, rect, (ow, oh) = so.REGISTRATION_RESIZE[fmt]
    assert rect[0] % 2 == 1 and rect[1] % 2 == 1
    y, uv = so.ramp_420(fmt, n, H, W)
    y_np, uv_np = so.to_numpy(so.LUMA_OF[fmt], y), so.to_numpy(so.CHROMA_OF[fmt], uv)
    got_y, got_uv = model_resize_420(fmt, y_np, uv_np, rect, (ow, oh))
    worst, compared, bound = so.registration_resize(fmt, so.to_planes(got_y), so.to_planes(got_uv), H, W, rect, ow, oh)
    print(fmt, 'resize', worst, compared, bound)
    assert worst <= bound and compared >= n * (ow // 2 - 2) * (oh // 2 - 2)         # (at most the first and last sample of an axis clamp)
    wrong_uv = plain_resize_of_the_halved_crop(fmt)(uv_np, rect, (ow, oh))
    wrong, _, _ = so.registration_resize(fmt, so.to_planes(got_y), so.to_planes(wrong_uv), H, W, rect, ow, oh)
    print(fmt, 'resize ignoring parity', wrong)
    assert wrong > bound
