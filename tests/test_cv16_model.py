"""Known answers of the uint16 remap / resize model (tests/cv16_model.py) that the uint16 GPU kernels are held to (tests/test_gpu_u16.py)."""
from fractions import Fraction

import numpy as np

import cv16_model as m
from oracle import meshflow_oracle as mo


def _maps(H, W, dx=0.0, dy=0.0):
    y, x = np.mgrid[0:H, 0:W]
    return (x + dx).astype(np.float32), (y + dy).astype(np.float32)


def test_identity_and_integer_shift_copy_the_frame():
    rng = np.random.default_rng(1)
    src = rng.integers(0, 65536, (9, 11, 3), dtype=np.uint16)
    np.testing.assert_array_equal(m.remap_bilinear_u16c3(src, *_maps(9, 11)), src)
    out = m.remap_bilinear_u16c3(src, *_maps(9, 11, 2.0, -1.0))
    np.testing.assert_array_equal(out[1:, :-2], src[:-1, 2:])
    np.testing.assert_array_equal(out[0], np.broadcast_to(np.array([0, 0, 255], np.uint16), (11, 3)))   # iy = -1: wholly outside


def test_half_pixel_rounds_half_to_even():
    src = np.zeros((1, 4, 3), np.uint16)
    src[0, :, 0] = [1, 2, 2, 3]
    mx = np.array([[0.5, 0.0, 2.5, 0.0]], np.float32)      # 1|2 -> 1.5 -> 2,  2|3 -> 2.5 -> 2
    my = np.zeros((1, 4), np.float32)
    out = m.remap_bilinear_u16c3(np.concatenate([src, src]), np.concatenate([mx, mx]), np.concatenate([my, my]))
    assert out[0, 0, 0] == 2 and out[0, 2, 0] == 2


def test_default_border_is_255_not_65535():
    src = np.full((4, 4, 3), 1000, np.uint16)
    out = m.remap_bilinear_u16c3(src, np.full((4, 4), 50.0, np.float32), np.full((4, 4), 50.0, np.float32))
    assert (out == np.array([0, 0, 255], np.uint16)).all()
    assert (m.border_u16((-3, 70000.4, 12.5)) == [0, 65535, 12]).all()


def test_outside_footprint_gives_cval_and_partly_outside_blends_it():
    src = np.full((4, 4, 3), 1000, np.uint16)
    border = (7, 40000, 255)
    out = m.remap_bilinear_u16c3(src, np.full((4, 4), -1.5, np.float32), np.zeros((4, 4), np.float32), border)
    assert (out == np.array(border, np.uint16)).all()      # ix = -2: ix + 1 < 0
    out = m.remap_bilinear_u16c3(src, np.full((4, 4), -0.5, np.float32), np.zeros((4, 4), np.float32), border)
    # ix = -1 (cval, weight 1/2) and ix = 0 (1000, weight 1/2): (7 + 1000) / 2 = 503.5 -> 504, (40000 + 1000) / 2, (255 + 1000) / 2 = 627.5 -> 628
    assert out[0, 0].tolist() == [504, 20500, 628]


def test_float32_order_rounds_where_exact_arithmetic_would_not():
    """Frozen case (seeded search): ((S00 w0 + S01 w1) + S10 w2) + S11 w3 in float32 is 34597.5 -> 34598; the exact sum is
    34597.499... -> 34597.  The model gives the float32 answer."""
    S = [6041, 57224, 44993, 25901]
    fx, fy = 17, 27
    src = np.zeros((2, 2, 3), np.uint16)
    src[0, 0, 0], src[0, 1, 0], src[1, 0, 0], src[1, 1, 0] = S
    mx = np.full((2, 2), fx / 32, np.float32)
    my = np.full((2, 2), fy / 32, np.float32)
    out = m.remap_bilinear_u16c3(src, mx, my)
    w = [Fraction(32 - fy, 32) * Fraction(32 - fx, 32), Fraction(32 - fy, 32) * Fraction(fx, 32),
         Fraction(fy, 32) * Fraction(32 - fx, 32), Fraction(fy, 32) * Fraction(fx, 32)]
    exact = sum(s * wk for s, wk in zip(S, w))
    assert round(exact) == 34597 and exact < Fraction(69195, 2)
    assert out[0, 0, 0] == 34598


def test_8bit_values_match_the_u8_remap_except_at_ties():
    rng = np.random.default_rng(5)
    H, W = 23, 31
    src8 = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    mx = (rng.uniform(-2, W + 1, (H, W)) * 32).round().astype(np.float32) / np.float32(32)
    my = (rng.uniform(-2, H + 1, (H, W)) * 32).round().astype(np.float32) / np.float32(32)
    mx[::3] = np.float32(0.5) + np.arange(W, dtype=np.float32)       # many exact ties
    a = m.remap_bilinear_u16c3(src8.astype(np.uint16), mx, my, (0, 0, 255)).astype(np.int64)
    b = mo.remap_bilinear_u8c3(src8, mx, my, (0, 0, 255)).astype(np.int64)
    d = a - b
    assert set(np.unique(d)) <= {0, -1}
    assert (d == -1).any() and (a[d == -1] % 2 == 0).all()
    # a difference only where the exact blend is a tie: 2 * (32 * 32 * t) is an odd multiple of 1024
    sx, sy = np.rint(mx * 32).astype(np.int64), np.rint(my * 32).astype(np.int64)
    fx, fy, ix, iy = sx & 31, sy & 31, sx >> 5, sy >> 5
    acc = np.zeros((H, W, 3), np.int64)
    for ddy in (0, 1):
        for ddx in (0, 1):
            tx, ty = ix + ddx, iy + ddy
            inside = (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            tap = np.where(inside[..., None], src8[np.clip(ty, 0, H - 1), np.clip(tx, 0, W - 1)].astype(np.int64), [0, 0, 255])
            acc += ((fx if ddx else 32 - fx) * (fy if ddy else 32 - fy))[..., None] * tap
    assert ((acc[d == -1] % 1024) == 512).all()


def test_resize_identity_and_2x_upscale():
    rng = np.random.default_rng(3)
    src = rng.integers(0, 65536, (7, 5, 3), dtype=np.uint16)
    np.testing.assert_array_equal(m.resize_linear_u16(src, 5, 7), src)
    up = np.zeros((2, 2, 3), np.uint16)
    up[:, 1] = 1000
    out = m.resize_linear_u16(up, 4, 2)
    assert out[:, :, 0].tolist() == [[0, 250, 750, 1000]] * 2
    col = np.zeros((2, 1, 3), np.uint16)
    col[1] = 65535
    out = m.resize_linear_u16(col, 1, 4)
    assert out[:, 0, 2].tolist() == [0, 16384, 49151, 65535]       # 0.25 * 65535 = 16383.75, 0.75 * 65535 = 49151.25
    np.testing.assert_array_equal(m.crop_frames_u16(src[None], (0, 0, 4, 6))[0], src)


def test_fast_blend_rounds_inside_its_samples():
    """The premise of the unclamped fast blend in warp_tails.h's remap_store_u16: the float32 chain ((s00 w0 + s01 w1) + s10 w2) + s11 w3
    rounds (half to even) into [min, max] of its four samples, so saturate_cast's clamp to 65535 never acts there.  Every (fx, fy) of
    the 32 x 32 weight table, every quadruple of samples from {0, 1, 65533, 65534, 65535}; a change of the blend order that breaks the
    premise fails here first."""
    import itertools
    vals = np.array([0, 1, 65533, 65534, 65535])
    quads = np.array(list(itertools.product(vals, repeat=4)), np.float32)            # (625, 4)
    fx, fy = np.meshgrid(np.arange(32), np.arange(32), indexing='ij')
    w = [wk.reshape(-1, 1) for wk in m.weights_f32(fx.reshape(-1), fy.reshape(-1))]   # (1024, 1) each
    s = [quads[:, k].reshape(1, -1) for k in range(4)]
    t = ((s[0] * w[0] + s[1] * w[1]) + s[2] * w[2]) + s[3] * w[3]
    assert t.dtype == np.float32 and t.shape == (1024, 625)
    r = np.rint(t.astype(np.float64))
    assert (r >= quads.min(1)[None, :]).all() and (r <= quads.max(1)[None, :]).all()
    assert (m.saturate_u16(t) == r).all()
