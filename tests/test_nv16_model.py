"""No GPU: tests/nv16_model.py pinned on maps whose answer is known without it, before any kernel is judged against it -- identity, horizontal
and vertical luma shifts (a row of luma is a row of chroma: where 4:2:2 differs from NV12), the half-pixel blend, an unowned pixel, the
independence of U and V, and the packed byte orders."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nv16_model  # noqa: E402

H, W = 23, 40                       # an odd height: 4:2:2 has no rule about it
HC, WC = H, W // 2
BORDER = (7, 201, 33)


@pytest.fixture(scope='module')
def frame():
    rng = np.random.default_rng(6)
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
    oy, ouv = nv16_model.warp_frame(y, uv, *shift_maps(0, 0), BORDER)
    assert oy.dtype == np.uint8 and ouv.dtype == np.uint8 and ouv.shape == uv.shape
    assert np.array_equal(oy, y) and np.array_equal(ouv, uv)


@pytest.mark.parametrize('dx', [2, -6])
def test_two_luma_columns_move_chroma_by_one_column(frame, dx):
    y, uv = frame
    _, ouv = nv16_model.warp_frame(y, uv, *shift_maps(dx, 0), BORDER)
    want = shifted(uv, dx // 2, 0, BORDER[1:])
    assert np.array_equal(ouv, want)
    assert (want == np.asarray(BORDER[1:], np.uint8)).all(axis=-1).sum() >= HC * abs(dx // 2)      # the strip is there


@pytest.mark.parametrize('dy', [1, -3])
def test_one_luma_row_moves_chroma_by_one_row(frame, dy):
    """Where 4:2:2 differs from NV12, whose chroma would blend two rows here."""
    y, uv = frame
    _, ouv = nv16_model.warp_frame(y, uv, *shift_maps(0, dy), BORDER)
    want = shifted(uv, 0, dy, BORDER[1:])
    assert np.array_equal(ouv, want)
    assert (want == np.asarray(BORDER[1:], np.uint8)).all(axis=-1).sum() >= WC * abs(dy)


def test_one_luma_pixel_is_the_half_pixel_blend(frame):
    y, uv = frame
    _, ouv = nv16_model.warp_frame(y, uv, *shift_maps(1, 0), BORDER)
    # cmx = cx - 0.5: ix = cx - 1, fx = 16 -- (a + b + 1) >> 1 of samples cx - 1 and cx, the border standing in for sample -1
    left = shifted(uv, 1, 0, BORDER[1:]).astype(np.int64)
    want = (left + uv.astype(np.int64) + 1) >> 1
    assert np.array_equal(ouv, want.astype(np.uint8))


def test_unowned_pixel_gives_the_border(frame):
    y, uv = frame
    mx, my = shift_maps(0, 0)
    mx, my = mx.copy(), my.copy()
    holes = [(0, 0), (7, 10), (H - 1, W - 2)]                       # even columns, rows of either parity
    for (r, c) in holes:
        mx[r, c], my[r, c] = W + 1, H + 1                           # the map template of an unowned pixel
    mx[1, 1], my[1, 1] = W + 1, H + 1                               # an odd luma column: chroma does not look at it
    oy, ouv = nv16_model.warp_frame(y, uv, mx, my, BORDER)
    want = uv.copy()
    for (r, c) in holes:
        want[r, c // 2] = BORDER[1:]
        assert oy[r, c] == BORDER[0]
    assert np.array_equal(ouv, want)
    cmx, cmy = nv16_model.chroma_maps(mx, my)
    border, partly, deep = nv16_model.tap_classes(cmx, cmy, WC, HC)
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
    _, ouv = nv16_model.warp_frame(y, zeroed, mx, my, border)
    _, full = nv16_model.warp_frame(y, uv, mx, my, border)
    assert not ouv[..., channel].any() and ouv[..., 1 - channel].any()
    assert np.array_equal(ouv[..., 1 - channel], full[..., 1 - channel])


@pytest.mark.parametrize('order', nv16_model.ORDERS)
def test_pack_unpack_round_trip(frame, order):
    y, uv = frame
    packed = nv16_model.pack(y, uv, order)
    assert packed.shape == (H, W, 2) and packed.dtype == np.uint8
    y2, uv2 = nv16_model.unpack(packed, order)
    assert np.array_equal(y2, y) and np.array_equal(uv2, uv)
    rng = np.random.default_rng(12)
    clip = rng.integers(0, 256, (3, 5, 6, 2), dtype=np.uint8)       # leading axes; pack(unpack(x)) == x
    assert np.array_equal(nv16_model.pack(*nv16_model.unpack(clip, order), order), clip)
    other = [o for o in nv16_model.ORDERS if o != order][0]
    assert not np.array_equal(nv16_model.pack(y, uv, other), packed)


def test_known_frame_byte_by_byte():
    y = np.array([[10, 20]], np.uint8)                              # a 2 x 1 frame: one word
    uv = np.array([[[30, 40]]], np.uint8)
    assert nv16_model.pack(y, uv, 'yuyv').tobytes() == bytes([10, 30, 20, 40])          # YUY2: Y0 U Y1 V
    assert nv16_model.pack(y, uv, 'uyvy').tobytes() == bytes([30, 10, 40, 20])          # UYVY: U Y0 V Y1
    yy, cc = nv16_model.unpack(np.frombuffer(bytes([10, 30, 20, 40]), np.uint8).reshape(1, 2, 2), 'yuyv')
    assert yy.tolist() == [[10, 20]] and cc.tolist() == [[[30, 40]]]
