"""No GPU: tests/planes_model.py tied to code that is already merged -- the uint16 models of tests/cv16_model.py, INTEGRATION.md's gather
recipe for labels -- and to itself at the identity; and, on NaN, infinities, signed zeros, subnormals and values near FLT_MAX
(tests/planes_values.py), to a scalar restatement that shares no helper with it and to a table of cases worked out by hand."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv16_model  # noqa: E402
import planes_model  # noqa: E402
import planes_values as pv  # noqa: E402

F32 = np.float32
DTYPES = (np.uint8, np.int16, np.float32, np.int64)


def random_maps(rng, H, W):
    """Float32 maps around the identity with everything a warp produces: interior positions on the 1/64 grid (so that cvRound's ties in
    32 u and in u occur), positions up to 12 pixels outside every edge, a block of unowned pixels at (W + 1, H + 1), and a few far-away ones."""
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing='ij')
    mx = xs + np.round(rng.normal(0, 6.0, (H, W)) * 64) / 64
    my = ys + np.round(rng.normal(0, 6.0, (H, W)) * 64) / 64
    mx[:3, :5], my[:3, :5] = W + 1, H + 1
    mx[-1, -4:], my[-1, -4:] = [-40000.0, 70000.0, 1e9, -3e9], [5.0, 5.0, 5.0, 5.0]
    return mx.astype(F32), my.astype(F32)


@pytest.mark.parametrize('H,W,fill', [(37, 53, 40000), (9, 6, 7), (5, 7, 65535)])
def test_linear_warp_is_the_uint16_warp_before_saturation(H, W, fill):
    """For integer-valued planes in 0 .. 65,535: saturate_u16(linear model) == channel 0 of remap_bilinear_u16c3 on the plane repeated three
    times, border included."""
    rng = np.random.default_rng(H * W)
    plane = rng.integers(0, 65536, (H, W)).astype(np.uint16)
    mx, my = random_maps(rng, H, W)
    got = planes_model.remap_linear_f32(plane.astype(F32), mx, my, float(fill))
    want = cv16_model.remap_bilinear_u16c3(np.repeat(plane[..., None], 3, axis=2), mx, my, (fill, fill, fill))[..., 0]
    assert got.dtype == F32 and np.array_equal(cv16_model.saturate_u16(got), want)
    assert (want == fill).any() and (want != fill).any()
    # wholly outside and unowned pixels are the fill value itself, as a float32
    assert np.all(got[:3, :5].view(np.uint32) == np.asarray(fill, F32).view(np.uint32))


@pytest.mark.parametrize('sh,sw,dh,dw', [(37, 53, 37, 53), (20, 31, 45, 64), (45, 64, 20, 31), (40, 60, 21, 30), (1, 1, 5, 4), (7, 1, 3, 9)])
def test_linear_resize_is_the_uint16_resize_before_saturation(sh, sw, dh, dw):
    assert not (sw == 2 * dw and sh == 2 * dh)
    src = np.random.default_rng(sh + sw).integers(0, 65536, (sh, sw)).astype(np.uint16)
    got = planes_model.resize_linear_f32(src.astype(F32), dw, dh)
    want = cv16_model.resize_linear_u16(src[..., None], dw, dh)[..., 0]
    assert got.shape == (dh, dw) and got.dtype == F32 and np.array_equal(cv16_model.saturate_u16(got), want)


def test_linear_resize_exact_2x_is_the_scalar_area_sum():
    src = np.random.default_rng(5).normal(0, 100.0, (24, 34)).astype(F32)
    got = planes_model.resize_linear_f32(src, 17, 12)
    want = np.empty((12, 17), F32)
    for y in range(12):
        for x in range(17):
            want[y, x] = F32(F32(F32(F32(src[2 * y, 2 * x] + src[2 * y, 2 * x + 1]) + src[2 * y + 1, 2 * x]) + src[2 * y + 1, 2 * x + 1]) * F32(0.25))
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # the float path at f = 0.5 pairs the taps row by row: not the same bits everywhere, which is why the branch is modelled
    assert got.shape == (12, 17)


@pytest.mark.parametrize('dtype', DTYPES)
def test_nearest_warp_is_the_documented_gather(dtype):
    """The nearest model equals INTEGRATION.md's recipe on the same maps: maps.round(), inside test, gather, fill."""
    torch = pytest.importorskip('torch')
    H, W, fill = 29, 41, 77
    rng = np.random.default_rng(11)
    labels = rng.integers(0, 60, (H, W)).astype(dtype)
    mx, my = random_maps(rng, H, W)
    mx[-1, -4:] = [-4000.0, 7000.0, 2.5, 3.5]                  # (the recipe's .long() is undefined beyond int64: moderate values only)
    got = planes_model.remap_nearest(labels, mx, my, fill)
    maps = torch.from_numpy(np.stack([mx, my], axis=-1))[None]
    lab = torch.from_numpy(labels)[None]
    idx = maps.round().long(); ix, iy = idx[..., 0], idx[..., 1]
    inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    flat = (iy.clamp(0, H - 1) * W + ix.clamp(0, W - 1)).view(1, -1)
    want = torch.where(inside, lab.view(1, -1).gather(1, flat).view(1, H, W), torch.full_like(lab, fill))[0].numpy()
    assert got.dtype == np.dtype(dtype) and np.array_equal(got, want)
    assert (got == fill).any() and (got != fill).any()
    # ties round to even: 2.5 -> 2, 3.5 -> 4
    assert planes_model.nearest_indices(np.array([2.5, 3.5, -0.5, 0.5], F32), np.zeros(4, F32))[0].tolist() == [2, 4, 0, 0]


@pytest.mark.parametrize('dtype', DTYPES)
def test_nearest_resize_identity_and_integer_factors(dtype):
    src = np.random.default_rng(2).integers(0, 100, (13, 22)).astype(dtype)
    assert np.array_equal(planes_model.resize_nearest(src, 22, 13), src)
    assert np.array_equal(planes_model.crop_planes(src[None], (0, 0, 21, 12), 'nearest'), src[None])
    assert np.array_equal(planes_model.resize_nearest(src, 44, 26), np.repeat(np.repeat(src, 2, axis=0), 2, axis=1))
    assert np.array_equal(planes_model.resize_nearest(src[:12], 11, 6), src[:12][0::2, 0::2])
    with pytest.raises(ValueError):
        planes_model.resize_nearest(src[:0], 4, 4)


# ---- special values: a scalar restatement, one output element at a time, every operation a np.float32 operation ---------------------------
def scalar_remap_linear(src, mx, my, fill):
    """remapBilinear on CV_32FC1 after RemapInvoker's conversion of float32 maps, BORDER_CONSTANT; moderate coordinates (no int16 saturation)."""
    H, W = src.shape
    fill = F32(fill)
    out = np.empty(mx.shape, F32)
    for y in range(mx.shape[0]):
        for x in range(mx.shape[1]):
            sx = round(float(F32(mx[y, x]) * F32(32)))                  # cvRound: Python's round() is half to even too
            sy = round(float(F32(my[y, x]) * F32(32)))
            ix, iy, fx, fy = sx >> 5, sy >> 5, sx & 31, sy & 31
            if ix >= W or ix + 1 < 0 or iy >= H or iy + 1 < 0:
                out[y, x] = fill
                continue
            ax, ay = F32(F32(fx) * F32(0.03125)), F32(F32(fy) * F32(0.03125))          # initInterTab1D: 1.f - i * scale, i * scale
            ax0, ay0 = F32(F32(1) - ax), F32(F32(1) - ay)
            w = (F32(ay0 * ax0), F32(ay0 * ax), F32(ay * ax0), F32(ay * ax))
            tap = [src[iy + dy, ix + dx] if 0 <= ix + dx < W and 0 <= iy + dy < H else fill for dy in (0, 1) for dx in (0, 1)]
            out[y, x] = F32(F32(F32(F32(tap[0] * w[0]) + F32(tap[1] * w[1])) + F32(tap[2] * w[2])) + F32(tap[3] * w[3]))
    return out


def scalar_resize_linear(src, dw, dh):
    """cv::resize INTER_LINEAR on CV_32FC1: the dsize == ssize copy, INTER_AREA's scalar fast path at exactly 2x, else HResizeLinear (two taps
    below xmax, S * 1.0f from xmax on) and VResizeLinear (always two taps)."""
    sh, sw = src.shape
    out = np.empty((dh, dw), F32)
    if (dw, dh) == (sw, sh):
        for y in range(dh):
            for x in range(dw):
                out.view(np.uint32)[y, x] = src.view(np.uint32)[y, x]
        return out
    if sw == 2 * dw and sh == 2 * dh:
        for y in range(dh):
            for x in range(dw):
                s = F32(src[2 * y, 2 * x] + src[2 * y, 2 * x + 1])
                s = F32(s + src[2 * y + 1, 2 * x])
                s = F32(s + src[2 * y + 1, 2 * x + 1])
                out[y, x] = F32(s * F32(0.25))
        return out
    scale_x, scale_y = 1.0 / (float(dw) / float(sw)), 1.0 / (float(dh) / float(sh))
    xofs, alpha, xmax = [], [], dw
    for dx in range(dw):
        fx = F32((dx + 0.5) * scale_x - 0.5)
        sx = int(np.floor(fx))
        fx = F32(fx - F32(sx))
        if sx < 0:
            fx, sx = F32(0), 0
        if sx + 1 >= sw:
            xmax = min(xmax, dx)
            if sx >= sw - 1:
                fx, sx = F32(0), sw - 1
        xofs.append(sx)
        alpha.append((F32(F32(1) - fx), fx))
    for dy in range(dh):
        fy = F32((dy + 0.5) * scale_y - 0.5)
        sy = int(np.floor(fy))
        fy = F32(fy - F32(sy))
        b0, b1 = F32(F32(1) - fy), fy
        rows = [min(max(sy + k, 0), sh - 1) for k in (0, 1)]
        for dx in range(dw):
            t = []
            for r in rows:
                S = src[r]
                if dx < xmax:
                    t.append(F32(F32(S[xofs[dx]] * alpha[dx][0]) + F32(S[xofs[dx] + 1] * alpha[dx][1])))
                else:
                    t.append(F32(S[xofs[dx]] * F32(1)))
            out[dy, dx] = F32(F32(t[0] * b0) + F32(t[1] * b1))
    return out


def seeded(H, W, seed, share=0.04):
    rng = np.random.default_rng(seed)
    plane = rng.normal(0, 1000.0, (H, W)).astype(F32)
    if H >= 2 * pv.BLOCK and W >= 3 * pv.BLOCK:
        pv.seed(plane, rng, {'sub': (1, 1), 'huge': (H - pv.BLOCK - 1, W // 3), 'zero': (H // 3, W - pv.BLOCK - 1)}, share)
    else:                                                                   # too small for the blocks: specials alone, densely
        k = max(H * W // 4, 1)
        plane.reshape(-1)[rng.choice(H * W, k, replace=False)] = pv.SPECIALS[rng.integers(0, len(pv.SPECIALS), k)]
    return plane


def assert_same(got, want, what):
    """uint32 bits where the scalar result is not NaN, NaN on both sides where it is."""
    assert got.dtype == F32 and got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), what
    diff = ~nan & (got.view(np.uint32) != want.view(np.uint32))
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:5].tolist())


@pytest.mark.parametrize('fill', [-777.25, -0.0, np.inf, np.nan])
def test_linear_warp_model_equals_its_scalar_restatement(fill):
    H, W = 26, 37
    plane = seeded(H, W, 31)
    mx, my = random_maps(np.random.default_rng(32), H, W)
    mx[-1, -4:] = [-400.0, 700.0, 2.5, W - 1.0]                              # (moderate: the restatement does not saturate to int16)
    with np.errstate(all='ignore'):
        want = scalar_remap_linear(plane, mx, my, fill)
    got = planes_model.remap_linear_f32(plane, mx, my, fill)
    assert_same(got, want, fill)
    c = pv.census(want)
    assert all(c[k] >= 1 for k in pv.CLASSES), c
    if not np.isnan(fill):
        assert np.all(got[:3, :5].view(np.uint32) == np.array([fill], F32).view(np.uint32)[0])


# sh, sw, dh, dw: up (both clamped ends), down, exactly 2x, identity, cw = 1, ch = 1, 1 x 1, one axis 2x only, one axis identity only
RESIZES = [(24, 37, 40, 61), (40, 61, 17, 23), (32, 50, 16, 25), (24, 37, 24, 37), (19, 1, 7, 9), (1, 23, 7, 9), (1, 1, 3, 4), (32, 50, 16, 31),
           (24, 37, 24, 50), (2, 2, 7, 9)]


@pytest.mark.parametrize('sh,sw,dh,dw', RESIZES)
def test_linear_resize_model_equals_its_scalar_restatement(sh, sw, dh, dw):
    src = seeded(sh, sw, sh * 100 + sw)
    if sw > 1:
        src[sh // 2, sw - 1], src[0, sw - 1], src[sh // 2, 1] = np.inf, -np.inf, np.inf       # both clamped ends see an infinity
    with np.errstate(all='ignore'):
        want = scalar_resize_linear(src, dw, dh)
    got = planes_model.resize_linear_f32(src, dw, dh)
    assert_same(got, want, (sh, sw, dh, dw))
    assert_same(planes_model.crop_planes(np.pad(src, ((2, 1), (3, 2)))[None], (3, 2, 3 + sw - 1, 2 + sh - 1), 'linear', (dw, dh))[0], want, 'crop')
    if min(sh, sw) >= 16:
        c = pv.census(want, 2e37 if (sw, sh) == (2 * dw, 2 * dh) else 1e38)     # (2x down: no finite result above FLT_MAX / 4)
        assert all(c[k] >= 1 for k in pv.CLASSES), c


def bits(*values):
    return np.array(values, F32).view(np.uint32).tolist()


def test_special_values_closed_form():
    """The semantics, case by case and by hand, so that they rest on something other than two programs agreeing."""
    inf, nan = F32(np.inf), F32(np.nan)
    plane = np.full((12, 12), 1000.0, F32)
    plane[5, 6] = inf
    one = lambda u, v, p=plane, fill=0.0: planes_model.remap_linear_f32(p, np.array([[u]], F32), np.array([[v]], F32), fill)[0, 0]  # noqa: E731
    # a deep-interior tap of +Inf with weight 0: 1000 * 1 + Inf * 0 + ... = NaN
    assert np.isnan(one(5.0, 5.0))
    # the same tap with a positive weight, beside finite taps (fx = 16/32, fy = 0: the lower row's products are 1000 * 0 = 0)
    assert one(5.5, 5.0) == inf
    assert one(5.5, 4.5) == inf                                             # all four weights 0.25
    # +Inf and -Inf in one footprint
    both = plane.copy(); both[5, 5] = -inf
    assert np.isnan(one(5.5, 5.0, both))
    # a footprint wholly outside: fill's own bits; partly outside: fill inside the sum
    assert bits(one(40.0, 3.0, fill=-0.0)) == bits(-0.0) and bits(one(40.0, 3.0, fill=inf)) == bits(inf) and np.isnan(one(40.0, 3.0, fill=nan))
    assert np.isnan(one(11.0, 3.0, fill=inf))                               # x = 11: S01 is outside, weight 0, Inf * 0
    assert one(11.5, 3.5, fill=inf) == inf                                  # every weight 0.25 (at v = 3.0 the lower fill tap has weight 0: NaN)
    assert np.isnan(one(11.5, 3.0, fill=inf))
    assert bits(one(11.0, 3.0, fill=-0.0)) == bits(1000.0)
    # -0.0 survives only if all four products are -0.0
    zeros = np.full((6, 6), -0.0, F32)
    assert bits(one(2.25, 2.5, zeros)) == bits(-0.0)
    zeros[2, 3] = 0.0
    assert bits(one(2.25, 2.5, zeros)) == bits(0.0)
    # the area path, exactly 2x down: S00 = S01 = 3e38 -- the first sum overflows whatever follows
    q = 2.0 ** 125                                                          # 4 q = 2^127 is finite
    a = np.array([[3e38, 3e38, q, q], [-3e38, -3e38, q, q]], F32)
    assert bits(*planes_model.resize_linear_f32(a, 2, 1)[0]) == bits(inf, q)
    # (another pairing, (S00 + S10) + (S01 + S11), would give 0 there)
    # four subnormals: bits 1, 2, 3, 5 sum to 11 units of 2^-149; a quarter is 2.75 units, to nearest 3.  1, 1, 1, 3: 1.5 units, to even 2
    sub = np.array([[1, 2, 1, 1], [3, 5, 1, 3]], np.uint32).view(F32)
    assert planes_model.resize_linear_f32(sub, 2, 1).view(np.uint32).tolist() == [[3, 2]]
    # identity size: the source's bits, -0.0 and a NaN payload included, next to an infinity
    ident = np.array([[0x80000000, 0x7F800000, 0x7FA00001], [0x3F800000, 0xFFC12345, 0x00000001]], np.uint32)
    assert np.array_equal(planes_model.resize_linear_f32(ident.view(F32), 3, 2).view(np.uint32), ident)
    assert np.array_equal(planes_model.crop_planes(np.pad(ident, 1).view(F32)[None], (1, 1, 3, 2), 'linear', (3, 2)).view(np.uint32)[0], ident)
    assert np.array_equal(planes_model.crop_planes(ident.view(F32)[None], (0, 0, 2, 1), 'linear').view(np.uint32)[0], ident)
    # last column +Inf on an upscale: +Inf in the clamped output columns (one tap, S * 1), NaN only where Inf is a zero-weight SECOND tap
    up = np.full((4, 5), 2.0, F32)
    up[:, 4] = inf
    got = planes_model.resize_linear_f32(up, 15, 6)                         # x = (dx + 0.5) / 3 - 0.5: 3 at dx = 10, 4 at dx = 13; no fy is 0
    assert np.all(got[:, 13:] == inf)                                       # xmax = 13: one tap
    assert np.all(got[:, 11:13] == inf) and np.isnan(got[:, 10]).all()      # two taps: weight 2/3 and 1/3 on Inf; then 2 * 1 + Inf * 0
    assert np.all(got[:, :10] == 2.0)
    big = planes_model.resize_linear_f32(np.pad(np.full((72, 99), 2.0, F32), ((0, 0), (0, 1)), constant_values=np.inf), 131, 90)
    assert np.all(big[:, -1] == inf) and not np.isnan(big).any()           # (100 x 72 -> 131 x 90: NaN before the one-tap tail was modelled)
    # the left-clamped columns stay two-tap: S[0] * 1 + S[1] * 0
    left = np.full((4, 5), 2.0, F32)
    left[:, 1] = inf
    assert np.isnan(planes_model.resize_linear_f32(left, 15, 6)[:, 0]).all()
    # the vertical pass is always two-tap: a clipped row pair is the same row twice, and fy = 0 multiplies the second row by 0
    col = np.array([[2.0], [inf]], F32)
    got = planes_model.resize_linear_f32(col, 1, 6)[:, 0]                   # y = (dy + 0.5) / 3 - 0.5: rows (0, 0) at dy = 0; y = 0 exactly at dy = 1
    assert got[0] == 2.0 and np.isnan(got[1]) and np.all(got[[2, 3, 5]] == inf)     # 2 (2/3) + 2 (1/3);  2 * 1 + Inf * 0;  Inf, positive weight
    assert np.isnan(got[4])                                                 # y = 1 exactly: rows (1, 1 clipped), Inf * 1 + Inf * 0
