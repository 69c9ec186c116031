"""No GPU: tests/p010_model.py pinned before any kernel is judged against it -- luma is channel 0 of the uint16 BGR model on the stacked clip,
U and V are independent, a constant plane under a border of the same value warps to itself, and whole-sample shifts move the planes."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv16_model  # noqa: E402
import p010_cases  # noqa: E402
import p010_model  # noqa: E402

H, W = 24, 40
HC, WC = H // 2, W // 2
BORDER = (700, 60123, 3301)


@pytest.fixture(scope='module')
def frame():
    rng = np.random.default_rng(15)
    y = rng.integers(0, 65536, (H, W), dtype=np.uint16)
    uv = rng.integers(0, 65536, (HC, WC, 2), dtype=np.uint16)
    y.setflags(write=False)
    uv.setflags(write=False)
    return y, uv


def wobble_maps(seed=3):
    """Smooth maps with every fraction, reaching past all four frame edges."""
    rng = np.random.default_rng(seed)
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    mx = (xs * np.float32(1.13) - np.float32(3.3) + rng.uniform(-0.5, 0.5, (H, W)).astype(np.float32)).astype(np.float32)
    my = (ys * np.float32(1.21) - np.float32(2.6) + rng.uniform(-0.5, 0.5, (H, W)).astype(np.float32)).astype(np.float32)
    return mx, my


def test_luma_is_channel_0_of_the_u16c3_model(frame):
    y, uv = frame
    mx, my = wobble_maps()
    oy, _ = p010_model.warp_frame(y, uv, mx, my, BORDER)
    three = cv16_model.remap_bilinear_u16c3(np.stack([y, y, y], axis=-1), mx, my, (BORDER[0],) * 3)
    assert oy.dtype == np.uint16 and np.array_equal(oy, three[..., 0])
    assert np.array_equal(three[..., 0], three[..., 1]) and np.array_equal(three[..., 0], three[..., 2])
    border, partly, deep = p010_model.tap_classes(mx, my, W, H)
    assert border.any() and partly.any() and deep.any()
    assert (oy[border] == BORDER[0]).all()


def test_chroma_is_the_two_channel_model_at_half_the_even_maps(frame):
    y, uv = frame
    mx, my = wobble_maps(4)
    _, ouv = p010_model.warp_frame(y, uv, mx, my, BORDER)
    cmx, cmy = (mx[::2, ::2] * np.float32(0.5)).astype(np.float32), (my[::2, ::2] * np.float32(0.5)).astype(np.float32)
    for ch in (0, 1):
        plane = uv[..., ch]
        one = cv16_model.remap_bilinear_u16c3(np.stack([plane] * 3, axis=-1), cmx, cmy, (BORDER[1 + ch],) * 3)[..., 0]
        assert np.array_equal(ouv[..., ch], one)
    assert ouv.dtype == np.uint16 and ouv.shape == uv.shape


def test_u_and_v_are_independent(frame):
    y, uv = frame
    mx, my = wobble_maps(5)
    _, ouv = p010_model.warp_frame(y, uv, mx, my, BORDER)
    _, swapped = p010_model.warp_frame(y, np.ascontiguousarray(uv[..., ::-1]), mx, my, (BORDER[0], BORDER[2], BORDER[1]))
    assert np.array_equal(swapped, ouv[..., ::-1])
    other = uv.copy()
    other[..., 1] = 65535 - other[..., 1]
    _, changed = p010_model.warp_frame(y, other, mx, my, BORDER)
    assert np.array_equal(changed[..., 0], ouv[..., 0]) and not np.array_equal(changed[..., 1], ouv[..., 1])


@pytest.mark.parametrize('value', [0, 1, 255, 256, 1023, 40000, 65472, 65535])
def test_constant_planes_warp_to_themselves(value):
    mx, my = wobble_maps(6)
    y = np.full((H, W), value, np.uint16)
    uv = np.full((HC, WC, 2), value, np.uint16)
    oy, ouv = p010_model.warp_frame(y, uv, mx, my, (value, value, value))
    assert np.array_equal(oy, y) and np.array_equal(ouv, uv)


def test_identity_and_whole_sample_shifts(frame):
    y, uv = frame
    xs, ys = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    oy, ouv = p010_model.warp_frame(y, uv, xs, ys, BORDER)
    assert np.array_equal(oy, y) and np.array_equal(ouv, uv)
    oy, ouv = p010_model.warp_frame(y, uv, xs - np.float32(4), ys - np.float32(2), BORDER)         # 4 luma = 2 chroma samples right, 2 = 1 down
    assert np.array_equal(oy[2:, 4:], y[:-2, :-4]) and (oy[:2] == BORDER[0]).all() and (oy[:, :4] == BORDER[0]).all()
    assert np.array_equal(ouv[1:, 2:], uv[:-1, :-2]) and (ouv[:1] == np.asarray(BORDER[1:], np.uint16)).all()
    assert (ouv[:, :2] == np.asarray(BORDER[1:], np.uint16)).all()
    # an unowned pixel, at (W + 1, H + 1), is the border in both planes
    mx, my = xs.copy(), ys.copy()
    mx[6, 10], my[6, 10] = W + 1, H + 1
    oy, ouv = p010_model.warp_frame(y, uv, mx, my, BORDER)
    assert oy[6, 10] == BORDER[0] and tuple(ouv[3, 5]) == BORDER[1:]


def test_default_border():
    assert p010_model.BORDER_RED == (20736, 23040, 61440) == (81 << 8, 90 << 8, 240 << 8)


def test_cases_hold_every_class_and_full_range_samples():
    for name in ('66x50_2x2_jitter', '64x48_4x6_nine_frames', '2x34_tiny'):
        c = p010_cases.case_for(name)
        assert c['y'].dtype == np.uint16 and c['uv'].dtype == np.uint16 and int(c['y'].max()) > 60000 and int(c['uv'].max()) > 60000
        assert len(set(p010_cases.BORDER)) == 3 and min(p010_cases.BORDER) > 255
        if not c['tiny']:
            assert all(c['luma_classes'][k] > 0 and c['classes'][k] > 0 for k in ('border', 'partly', 'deep'))
