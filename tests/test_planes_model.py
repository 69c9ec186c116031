"""No GPU: tests/planes_model.py tied to code that is already merged -- the uint16 models of tests/cv16_model.py, INTEGRATION.md's gather
recipe for labels -- and to itself at the identity."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv16_model  # noqa: E402
import planes_model  # noqa: E402

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
