"""-m gpu: the float32 side planes on the values depth, disparity, flow and confidence planes really carry -- NaN, infinities, -0.0,
subnormals, values near FLT_MAX (tests/planes_values.py) -- through `ops.warp_planes` and `ops.crop_resize_planes`, host and device rectangle.

The rule (planes_values.mismatches): uint32 bits wherever tests/planes_model.py's value is not NaN; where it is NaN the kernel's must be a NaN
of any payload (x86 and gfx950 generate different default NaNs).  So that the rule cannot hide a failure, every test first asserts FROM THE
MODEL ALONE that NaN is at most 5 % of the compared array and that NaN, +Inf, -Inf, -0.0, a nonzero subnormal and a finite value above 1e38
all occur in it, that some pixel has a non-finite tap with weight 0, and (warp) that some partly-outside pixel has `fill` as a tap.  The three
edge rectangles of the crop-resize (1 pixel wide, 1 pixel high, the last 2 x 2) give 9 x 7 outputs whose columns or rows repeat: one NaN
sample would be 7 or 9 of 126 results, above the cap.  They carry hand-placed pairs of every other class instead, and the only NaNs the model gives there are the
four of the 1-pixel-high crop's middle output row, where fy is exactly 0 and the vertical pass forms Inf * 0 (under the cap).  Exactly 2x down no finite result can exceed FLT_MAX / 4, so "above 1e38" is "above 2e37"
there.  With a NaN fill the unowned and wholly-outside
pixels are NaN by definition; they are checked on their own and the 5 % cap is taken over the other pixels.

Also here, found by the same reading: output widths above 256 (more than one tile per row), nine frames (all eight workgroup rotations of
plane_footprint and the wrap), rectangles on the plane's last column, row and element from a view that ends with its buffer, and the nearest
paths as bit copies of NaN payloads."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv16_model  # noqa: E402
import planes_model  # noqa: E402
import planes_values as pv  # noqa: E402
from test_gpu_planes import (FILL, FILL_F32, RECT, RECT_H, RECT_W, SIZES, UINT, case_for, dev, dev64, motion, raw, table_for,  # noqa: E402,F401
                             to_dev)
from oracle import meshflow_oracle as mo  # noqa: E402

F32 = np.float32
GEOMS = ['100x72_3x5', '131x97_4x6_oddW']
FILLS = {'finite': F32(FILL_F32), 'negzero': F32(-0.0), 'inf': F32(np.inf), 'nan': pv.QNAN}
_SEEDED = {}


def quantised(mx, my):
    """remapBilinear's integer positions and 5-bit fractions of float32 maps (moderate coordinates)."""
    sx, sy = np.rint(mx * F32(32)).astype(np.int64), np.rint(my * F32(32)).astype(np.int64)
    return sx >> 5, sy >> 5, sx & 31, sy & 31


def regions(mx, my, W, H):
    """(unowned, wholly outside, partly outside, deep) masks of a map pair."""
    ix, iy, _, _ = quantised(mx, my)
    unowned = (mx == F32(W + 1)) & (my == F32(H + 1))
    whole = (ix >= W) | (ix + 1 < 0) | (iy >= H) | (iy + 1 < 0)
    partly = ~whole & ((ix < 0) | (ix + 1 >= W) | (iy < 0) | (iy + 1 >= H))
    deep = ~whole & (ix >= pv.BLOCK) & (ix + 1 < W - pv.BLOCK) & (iy >= pv.BLOCK) & (iy + 1 < H - pv.BLOCK)
    return unowned, whole, partly, deep


def block_corners(mx, my, W, H):
    """Three source positions, far apart, each the footprint of a deep-interior output pixel: the top-left corners of the three blocks."""
    ix, iy, _, _ = quantised(mx, my)
    deep = regions(mx, my, W, H)[3]
    got = {}
    for kind, (ty, tx) in zip(('sub', 'huge', 'zero'), ((H // 4, W // 4), (H // 2, 3 * W // 4), (3 * H // 4, W // 3))):
        ys, xs = np.nonzero(deep)
        k = np.argmin((ys - ty) ** 2 + (xs - tx) ** 2)
        got[kind] = (iy[ys[k], xs[k]] - 3, ix[ys[k], xs[k]] - 3)
    return got


def seeded_case(name):
    """case_for(name)'s geometry and N(0, 1000) planes with the specials written in, and the model's result for each fill: once, shared."""
    if name in _SEEDED:
        return _SEEDED[name]
    c = case_for(name)
    rng = np.random.default_rng(2024)
    planes = c['planes'].copy()
    for f in range(c['F']):
        pv.seed(planes[f], rng, block_corners(c['mx'][f], c['my'][f], c['W'], c['H']))
    s = dict(c=c, planes=planes, linear={k: np.stack([planes_model.remap_linear_f32(planes[f], c['mx'][f], c['my'][f], v) for f in range(c['F'])])
                                         for k, v in FILLS.items()})
    for a in (planes, *s['linear'].values()):
        a.setflags(write=False)
    _SEEDED[name] = s
    return s


def zero_weight_nonfinite_taps(planes, mx, my, fill):
    """How many pixels that are not wholly outside have a tap of weight 0 that is not finite (a sample, or `fill` outside the plane)."""
    F, H, W = planes.shape
    ix, iy, fx, fy = quantised(mx, my)
    whole = regions(mx, my, W, H)[1]
    hit = np.zeros(planes.shape, bool)
    for dy, dx, zero in ((0, 0, np.zeros_like(hit)), (0, 1, fx == 0), (1, 0, fy == 0), (1, 1, (fx == 0) | (fy == 0))):
        tx, ty = ix + dx, iy + dy
        inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
        tap = np.where(inside, planes[np.arange(F)[:, None, None], np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)], F32(fill))
        hit |= zero & ~np.isfinite(tap)
    return int((hit & ~whole).sum())


def warp_conditions(name, fill):
    """What the model alone must show before a kernel's result is looked at; returns (the model's result, the pixels that are `fill` itself)."""
    s = seeded_case(name)
    c, want, fv = s['c'], s['linear'][fill], FILLS[fill]
    W, H = c['W'], c['H']
    unowned, whole, partly, deep = regions(c['mx'], c['my'], W, H)
    is_fill = unowned | whole
    counted = want[~is_fill] if fill == 'nan' else want
    pv.assert_covers(counted, '%s fill=%s' % (name, fill))
    zw = zero_weight_nonfinite_taps(s['planes'], c['mx'], c['my'], fv)
    print('zero-weight non-finite taps', zw, 'partly outside', int(partly.sum()), 'fill pixels', int(is_fill.sum()), 'deep', int(deep.sum()))
    assert zw >= 1 and partly.any() and unowned.any() and deep.any()
    if fill == 'nan':
        assert np.isnan(want[is_fill]).all() and np.isnan(want[partly]).all()
    else:
        assert np.all(want[is_fill].view(np.uint32) == np.array([fv]).view(np.uint32)[0])
    if fill == 'inf':                                              # a +Inf fill with weight 0 is NaN, with a positive weight +Inf
        assert np.isnan(want[partly]).any() and np.isposinf(want[partly]).any()
    if fill == 'finite':
        assert np.any(want[partly] != fv)
    return want, is_fill


@pytest.mark.parametrize('fill', list(FILLS))
@pytest.mark.parametrize('name', GEOMS)
def test_linear_warp_on_special_values(dev, name, fill):
    from meshflow_amd import ops
    want, is_fill = warp_conditions(name, fill)
    s = seeded_case(name)
    c, fv = s['c'], FILLS[fill]
    got = ops.warp_planes(to_dev(s['planes'], dev), table_for(dev, c), 'linear', fill=float(fv))
    torch.cuda.synchronize()
    bits = raw(got)
    if fill == 'nan':
        assert np.isnan(bits.view(F32)[is_fill]).all()
    else:
        assert np.all(bits[is_fill] == np.array([fv]).view(np.uint32)[0])
    bad = pv.mismatches(bits, want)
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist(), bits[bad][:5].tolist(), want.view(np.uint32)[bad][:5].tolist())


PAYLOADS = np.array([0x7FA00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000001, 0x807FFFFF, 0x7FC00000, 0xFF800000], np.uint32)


def payload_planes(shape, rng):
    """float32 planes whose bits are N(0, 1000) samples with one in eight replaced by NaNs of distinct payloads (one signalling), -0.0,
    subnormals and -Inf: data a float operation would change and a copy must not."""
    bits = rng.normal(0, 1000.0, shape).astype(F32).view(np.uint32).copy()
    pick = rng.random(shape) < 0.125
    bits[pick] = PAYLOADS[rng.integers(0, len(PAYLOADS), int(pick.sum()))]
    bits.reshape(-1)[:len(PAYLOADS)] = PAYLOADS
    return bits


@pytest.mark.parametrize('name', GEOMS)
def test_nearest_is_a_bit_copy_of_float_planes(dev, name):
    from meshflow_amd import ops
    c = case_for(name)
    bits = payload_planes(c['planes'].shape, np.random.default_rng(5))
    fill_bits = 0x7FB00BAD                                         # a signalling NaN no sample holds
    want = np.stack([planes_model.remap_nearest(bits[f], c['mx'][f], c['my'][f], fill_bits) for f in range(c['F'])])
    for p in PAYLOADS:
        assert (want == p).any(), hex(p)
    assert (want == fill_bits).any() and not (bits == fill_bits).any()
    table = table_for(dev, c)
    got = ops.warp_planes(to_dev(bits, dev), table, 'nearest', fill=int(np.array([fill_bits], np.uint32).view(np.int32)[0]))
    assert np.array_equal(raw(got), want)
    # the same bytes as a float32 tensor: still a copy, NaN payloads and the signalling bit included
    as_f32 = to_dev(bits, dev).view(torch.float32)
    got = ops.warp_planes(as_f32, table, 'nearest', fill=-0.0)
    assert got.dtype == torch.float32
    assert np.array_equal(raw(got), np.where(want == fill_bits, np.uint32(0x80000000), want))
    rect = (2, 1, c['W'] - 4, c['H'] - 3)
    d_rect = torch.tensor(rect, dtype=torch.int32, device=dev)
    for size in (None, (c['W'] + 9, c['H'] - 5), (c['W'] - 5, c['H'] - 3)):          # the last one: the crop's own size
        want_r = planes_model.crop_planes(bits, rect, 'nearest', size)
        assert sum((want_r == p).any() for p in PAYLOADS) == len(PAYLOADS)
        for t in (to_dev(bits, dev), as_f32):
            got = ops.crop_resize_planes(t, rect, 'nearest', size=size)
            got_dev, status = ops.crop_resize_planes(t, d_rect, 'nearest', size=size)
            assert got.dtype == t.dtype and np.array_equal(raw(got), want_r) and np.array_equal(raw(got_dev), want_r) and int(status.item()) == 0


# ---- crop-resize ----------------------------------------------------------------------------------------------------------------------------
WHOLE = (0, 0, RECT_W - 1, RECT_H - 1)
# name: (rectangle, size, which checks).  'classes': all six classes and the 5 % cap; 'edge': hand-placed specials on the plane's last column,
# row and 2 x 2
CROPS = {**{'rect_' + k: (RECT, v, 'classes') for k, v in SIZES.items()},
         'rect_256x9': (RECT, (256, 9), 'classes'), 'rect_257x9': (RECT, (257, 9), 'classes'), 'rect_600x9': (RECT, (600, 9), 'classes'),
         'whole_identity': (WHOLE, None, 'classes'), 'whole_2x_up': (WHOLE, (154, 100), 'classes'),
         'down_2x': ((1, 2, 76, 49), (38, 24), 'classes'),
         'last_column': ((76, 0, 76, 49), (9, 7), 'edge'), 'last_row': ((0, 49, 76, 49), (9, 7), 'edge'),
         'last_2x2': ((75, 48, 76, 49), (9, 7), 'edge')}
_CROP_PLANES = []
EDGE_PAIRS = ((-0.0, -0.0), (np.inf, 1.0), (-np.inf, -np.inf), (-1e-40, -1e-40), (3e38, 3e38))


def crop_planes_seeded():
    """Two 77 x 50 planes of N(0, 1000) with the specials, the blocks inside RECT on rows that every output height used here samples as a
    pair, and hand-placed values on the last column, the last row and the last 2 x 2."""
    if _CROP_PLANES:
        return _CROP_PLANES[0]
    rng = np.random.default_rng(17)
    planes = rng.normal(0, 1000.0, (2, RECT_H, RECT_W)).astype(F32)
    for p, corners in zip(planes, ({'sub': (6, 8), 'huge': (20, 30), 'zero': (34, 52)}, {'sub': (30, 10), 'huge': (8, 50), 'zero': (18, 28)})):
        pv.seed(p, rng, corners)
        p[10, RECT[0] + 1] = p[12, 1] = np.inf                      # the left-clamped columns' zero-weight tap, for RECT and for the whole plane
        # the last column and the last row at the sample pairs a (9, 7) output takes from them: one class per pair, and no NaN (see the docstring)
        for line, length, out_len in ((p[:, RECT_W - 1], RECT_H, 7), (p[RECT_H - 1, :], RECT_W, 9)):
            at = np.clip(mo.resize_linear_tables(length, out_len)[0], 0, length - 2)
            line[~np.isfinite(line)] = 7.0
            for k, pair in enumerate(EDGE_PAIRS):
                line[at[k]:at[k] + 2] = pair
    planes[0, RECT_H - 2:, RECT_W - 2:] = [[np.inf, 3.0], [-0.0, -0.0]]
    planes[1, RECT_H - 2:, RECT_W - 2:] = [[pv.FLT_MAX, pv.FLT_MAX], [-np.inf, 5.0]]
    planes.setflags(write=False)
    _CROP_PLANES.append(planes)
    return planes


def zero_weight_nonfinite_resize(crop, oW, oH):
    """Pixels of the linear route (neither copy nor area) with a non-finite tap of weight 0 -- S[sx + 1] where f = 0 below xmax, row sy1 where
    fy = 0 -- and how many columns and rows have such a weight at all."""
    n, ch, cw = crop.shape
    sx, fx = mo.resize_linear_tables(cw, oW)
    fx = np.where(sx < 0, F32(0), fx)
    sx = np.maximum(sx, 0)
    two = sx + 1 < cw
    cols = np.nonzero(two & (fx == 0))[0]
    sy, fy = mo.resize_linear_tables(ch, oH)
    rows = np.nonzero(fy == 0)[0]
    hits = 0
    exist = len(cols) + len(rows)
    if len(cols):
        hits += int((~np.isfinite(crop[:, :, sx[cols] + 1])).any(axis=0).sum())
    if len(rows):
        hits += int((~np.isfinite(crop[:, np.clip(sy[rows] + 1, 0, ch - 1), :])).any(axis=0).sum())
    return hits, exist


def end_view(dev, a):
    """`a` on the device as a view that starts one element into its buffer and ends exactly where the buffer ends: no byte behind the last
    sample belongs to the tensor's storage."""
    a = np.ascontiguousarray(a)
    buf = torch.full((a.size + 1,), 12345.0, dtype=torch.float32, device=dev)
    view = buf[1:].view(a.shape)
    view.copy_(torch.from_numpy(a))
    assert view.data_ptr() + 4 * a.size == buf.data_ptr() + 4 * buf.numel()
    return view


def crop_conditions(crop):
    """What the model alone must show before a kernel's result is looked at; returns the model's result."""
    rect, size, checks = CROPS[crop]
    planes = crop_planes_seeded()
    n, H, W = planes.shape
    oW, oH = size or (W, H)
    cw, ch = rect[2] - rect[0] + 1, rect[3] - rect[1] + 1
    want = planes_model.crop_planes(planes, rect, 'linear', size)
    assert want.shape == (n, oH, oW)
    src = planes[:, rect[1]:rect[3] + 1, rect[0]:rect[2] + 1]
    copy, area = (cw, ch) == (oW, oH), (cw, ch) == (2 * oW, 2 * oH)
    if checks == 'classes':
        # exactly 2x down every finite result is a finite sum times 0.25f, at most FLT_MAX / 4 = 8.5e37: "above 1e38" cannot occur there, and the
        # class is a finite magnitude above 2e37 instead (a sum above 8e37, which only the block of huge values reaches)
        pv.assert_covers(want, crop, huge_above=2e37 if area else 1e38)
        if copy:
            assert np.array_equal(want.view(np.uint32), src.view(np.uint32))
        elif not area:
            zw, exist = zero_weight_nonfinite_resize(src, oW, oH)
            print('zero-weight taps at', exist, 'columns and rows; non-finite ones at', zw)
            assert zw >= 1 or exist == 0                            # ('down' has no column or row with a fraction of exactly 0)
            assert exist >= 1 or crop == 'rect_down'
    else:
        c = pv.census(want)
        print(crop, c)
        assert c['nan'] <= 0.05 * c['size'] and c['+inf'] >= 1 and c['-inf'] >= 1 and c['-0.0'] >= 1 and c['huge'] >= 1
        assert c['subnormal'] >= 1 or crop == 'last_2x2'
    if crop == 'down_2x':
        assert area
    return want


@pytest.mark.parametrize('crop', list(CROPS))
def test_crop_resize_on_special_values(dev, crop):
    from meshflow_amd import ops
    rect, size, _ = CROPS[crop]
    planes = crop_planes_seeded()
    n, H, W = planes.shape
    oW, oH = size or (W, H)
    want = crop_conditions(crop)
    # ---- the kernels: the rectangle by value and from device memory
    d_planes = end_view(dev, planes)
    got = ops.crop_resize_planes(d_planes, rect, 'linear', size=size)
    got_dev, status = ops.crop_resize_planes(d_planes, torch.tensor(rect, dtype=torch.int32, device=dev), 'linear', size=size)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (n, oH, oW) and int(status.item()) == 0
    for which, g in (('host', got), ('device', got_dev)):
        bits = raw(g)
        bad = pv.mismatches(bits, want)
        assert not bad.any(), (which, int(bad.sum()), np.argwhere(bad)[:5].tolist(), bits[bad][:5].tolist(), want.view(np.uint32)[bad][:5].tolist())
    # nearest on the same bytes: a bit copy
    want_n = planes_model.crop_planes(planes.view(np.uint32), rect, 'nearest', size)
    as_i32 = d_planes.view(torch.int32)
    got = ops.crop_resize_planes(as_i32, rect, 'nearest', size=size)
    got_dev, status = ops.crop_resize_planes(as_i32, torch.tensor(rect, dtype=torch.int32, device=dev), 'nearest', size=size)
    assert np.array_equal(raw(got), want_n) and np.array_equal(raw(got_dev), want_n) and int(status.item()) == 0


# ---- nine frames: every rotation of plane_footprint's workgroup placement, and the wrap --------------------------------------------------
_NINE = []


def nine_frames():
    if _NINE:
        return _NINE[0]
    F, H, W, R, C = 9, 48, 64, 2, 2
    disp, hom, stab = motion(F, H, W, R, C, 50, 3.0, 'shift')
    mx, my = np.empty((F, H, W), F32), np.empty((F, H, W), F32)
    for f in range(F):
        mx[f], my[f], _, bad = cv16_model.warp_maps(W, H, R, C, disp[f], stab[f])
        assert bad == 0
    rng = np.random.default_rng(9)
    planes = rng.normal(0, 1000.0, (F, H, W)).astype(F32)
    for f in range(F):
        pv.seed(planes[f], rng, block_corners(mx[f], my[f], W, H))
    labels = {es: rng.integers(0, 200, (F, H, W), dtype=np.uint64).astype(UINT[es]) for es in (1, 8)}
    c = dict(F=F, H=H, W=W, R=R, C=C, disp=disp, stab=stab, mx=mx, my=my, planes=planes, labels=labels)
    c['linear'] = np.stack([planes_model.remap_linear_f32(planes[f], mx[f], my[f], FILL_F32) for f in range(F)])
    c['nearest'] = {es: np.stack([planes_model.remap_nearest(labels[es][f], mx[f], my[f], FILL[es][1]) for f in range(F)]) for es in (1, 8)}
    _NINE.append(c)
    return c


def test_nine_frames(dev):
    from meshflow_amd import ops
    c = nine_frames()
    pv.assert_covers(c['linear'], 'nine frames')
    for f in range(c['F']):                                            # every frame can fail on its own: data, border and interior
        unowned, whole, partly, deep = regions(c['mx'][f], c['my'][f], c['W'], c['H'])
        assert (unowned | whole).any() and deep.any() and len(np.unique(c['linear'][f].view(np.uint32))) > 100, f
    scan = table_for(dev, c)
    ops.crop_scan(scan)
    table = table_for(dev, c)
    got = ops.warp_planes(to_dev(c['planes'], dev), table, 'linear', fill=FILL_F32)
    torch.cuda.synchronize()
    table.check()
    bad = pv.mismatches(raw(got), c['linear'])
    assert not bad.any(), (int(bad.sum()), np.argwhere(bad)[:5].tolist())
    assert torch.equal(table.crop, scan.crop) and torch.equal(table.clip_bounds, scan.clip_bounds)
    defaults = torch.tensor([0, 0, c['W'] - 1, c['H'] - 1], dtype=torch.int32, device=dev)
    assert not torch.equal(scan.crop, defaults.expand(c['F'], 4)), 'the geometry sets no crop value: nothing compared'
    for es in (1, 8):
        fresh = table_for(dev, c)
        got = ops.warp_planes(to_dev(c['labels'][es], dev), fresh, 'nearest', fill=FILL[es][0])
        diff = raw(got) != c['nearest'][es]
        assert not diff.any(), (es, int(diff.sum()), np.argwhere(diff)[:5].tolist())
        assert torch.equal(fresh.crop, scan.crop) and torch.equal(fresh.clip_bounds, scan.clip_bounds)
