"""No GPU: tests/nv12_model.py pinned on maps whose answer is known without it, before any kernel is judged against it -- identity, even and
odd luma shifts, an unowned pixel, and the independence of U and V."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nv12_model  # noqa: E402

H, W = 24, 40
HC, WC = H // 2, W // 2
BORDER = (7, 201, 33)


@pytest.fixture(scope='module')
def frame():
    rng = np.random.default_rng(5)
    y = rng.integers(0, 256, (H, W), dtype=np.uint8)
    uv = rng.integers(0, 256, (HC, WC, 2), dtype=np.uint8)
    y.setflags(write=False)
    uv.setflags(write=False)
    return y, uv


def shift_maps(dx, dy):
    """Output luma pixel (x, y) samples (x - dx, y - dy): the picture moves by (dx, dy)."""
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    return (xs - np.float32(dx)).astype(np.float32), (ys - np.float32(dy)).astype(np.float32)


def shifted(uv, k, m, border_uv):
    """uv moved by (k, m) whole chroma samples, the uncovered strip in the border colour."""
    out = np.empty_like(uv)
    out[...] = np.asarray(border_uv, np.uint8)
    ys, xs = np.arange(HC), np.arange(WC)
    sy, sx = ys - m, xs - k
    oky, okx = (sy >= 0) & (sy < HC), (sx >= 0) & (sx < WC)
    out[np.ix_(ys[oky], xs[okx])] = uv[np.ix_(sy[oky], sx[okx])]
    return out


def test_identity_returns_the_planes(frame):
    y, uv = frame
    oy, ouv = nv12_model.warp_frame(y, uv, *shift_maps(0, 0), BORDER)
    assert oy.dtype == np.uint8 and ouv.dtype == np.uint8 and ouv.shape == uv.shape
    assert np.array_equal(oy, y) and np.array_equal(ouv, uv)


@pytest.mark.parametrize('dx,dy', [(4, -2), (-6, 8)])
def test_even_luma_shift_moves_chroma_by_half(frame, dx, dy):
    y, uv = frame
    _, ouv = nv12_model.warp_frame(y, uv, *shift_maps(dx, dy), BORDER)
    want = shifted(uv, dx // 2, dy // 2, BORDER[1:])
    assert np.array_equal(ouv, want)
    assert (want == np.asarray(BORDER[1:], np.uint8)).all(axis=-1).sum() >= WC * abs(dy // 2)      # the strip is there


def test_one_luma_pixel_is_the_half_pixel_blend(frame):
    y, uv = frame
    _, ouv = nv12_model.warp_frame(y, uv, *shift_maps(1, 0), BORDER)
    # cmx = cx - 0.5: ix = cx - 1, fx = 16 -- (a + b + 1) >> 1 of samples cx - 1 and cx, the border standing in for sample -1
    left = shifted(uv, 1, 0, BORDER[1:]).astype(np.int64)
    want = (left + uv.astype(np.int64) + 1) >> 1
    assert np.array_equal(ouv, want.astype(np.uint8))


def test_three_luma_rows_blend_at_fy_16(frame):
    y, uv = frame
    _, ouv = nv12_model.warp_frame(y, uv, *shift_maps(0, 3), BORDER)
    # cmy = cy - 1.5: iy = cy - 2, fy = 16 -- (a + b + 1) >> 1 of rows cy - 2 and cy - 1
    a, b = shifted(uv, 0, 2, BORDER[1:]).astype(np.int64), shifted(uv, 0, 1, BORDER[1:]).astype(np.int64)
    assert np.array_equal(ouv, ((a + b + 1) >> 1).astype(np.uint8))


def test_unowned_pixel_gives_the_border(frame):
    y, uv = frame
    mx, my = shift_maps(0, 0)
    mx, my = mx.copy(), my.copy()
    holes = [(0, 0), (6, 10), (H - 2, W - 2)]
    for (r, c) in holes:
        mx[r, c], my[r, c] = W + 1, H + 1                           # the map template of an unowned pixel
    mx[1, 1], my[1, 1] = W + 1, H + 1                               # an odd luma pixel: chroma does not look at it
    oy, ouv = nv12_model.warp_frame(y, uv, mx, my, BORDER)
    want = uv.copy()
    for (r, c) in holes:
        want[r // 2, c // 2] = BORDER[1:]
        assert oy[r, c] == BORDER[0]
    assert np.array_equal(ouv, want)
    cmx, cmy = nv12_model.chroma_maps(mx, my)
    border, partly, deep = nv12_model.tap_classes(cmx, cmy, WC, HC)
    assert int(border.sum()) == len(holes) and deep.any() and partly.any()


@pytest.mark.parametrize('channel', [0, 1])
def test_u_and_v_never_mix(frame, channel):
    y, uv = frame
    zeroed = uv.copy()
    zeroed[..., channel] = 0
    border = [9, 77, 77]
    border[1 + channel] = 0
    rng = np.random.default_rng(11)
    mx, my = shift_maps(0, 0)
    mx = (mx + rng.uniform(-9, 9, mx.shape)).astype(np.float32)     # every fraction, taps inside and outside
    my = (my + rng.uniform(-9, 9, my.shape)).astype(np.float32)
    _, ouv = nv12_model.warp_frame(y, zeroed, mx, my, border)
    _, full = nv12_model.warp_frame(y, uv, mx, my, border)
    assert not ouv[..., channel].any() and ouv[..., 1 - channel].any()
    assert np.array_equal(ouv[..., 1 - channel], full[..., 1 - channel])
