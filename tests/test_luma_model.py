"""tests/luma_model.py, the specification of the device luma, against what is known of it without a cv2: the values of the pure colours, greys
that stay what they are, the red-first order, the ignored alpha, the 16-bit truncation, and a condition that keeps a wrong constant from
passing: at most 1 away from round(0.114 b + 0.587 g + 0.299 r).  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import luma_model as lm  # noqa: E402


def noise(shape, dtype, seed):
    from meshflow_amd import synthetic
    top = np.iinfo(dtype).max + 1
    return (synthetic.hash32(np.arange(int(np.prod(shape))), seed) % top).astype(dtype).reshape(shape)


def test_the_pure_colours_at_255():
    bgr = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8).reshape(1, 1, 3, 3)
    assert lm.luma(bgr).tolist() == [[[29, 150, 76]]]
    assert lm.luma(bgr, red_first=True).tolist() == [[[76, 150, 29]]]
    assert lm.luma(bgr).dtype == np.uint8 and lm.luma(bgr).shape == (1, 1, 3)


def test_a_grey_pixel_stays_what_it_is():
    v = np.arange(256, dtype=np.uint8)
    for red_first in (False, True):
        assert np.array_equal(lm.luma(np.stack([v, v, v], -1).reshape(1, 16, 16, 3), red_first).reshape(-1), v)
        assert np.array_equal(lm.luma(np.stack([v, v, v, 255 - v], -1).reshape(1, 16, 16, 4), red_first).reshape(-1), v)
    v16 = np.unique(np.concatenate([np.arange(0, 65536, 251), [0, 255, 256, 257, 32767, 32768, 65279, 65280, 65535]])).astype(np.uint16)
    got = lm.luma(np.stack([v16, v16, v16], -1).reshape(1, 1, -1, 3)).reshape(-1)
    assert np.array_equal(got, (v16 >> 8).astype(np.uint8))
    assert np.array_equal(lm.luma(v16.reshape(1, 1, -1)).reshape(-1), (v16 >> 8).astype(np.uint8))


def test_sixteen_bit_values_are_truncated_not_rounded():
    assert lm.luma(np.array([255, 256, 511, 32767, 32768, 65535], np.uint16).reshape(1, 1, 6)).reshape(-1).tolist() == [0, 1, 1, 127, 128, 255]
    px = np.array([[65535, 0, 0], [0, 65535, 0], [0, 0, 65535], [255, 255, 255], [511, 511, 511]], np.uint16).reshape(1, 1, 5, 3)
    # 65535 * 1868 / 16384 = 7471.9 -> 7472 = 29 * 256 + 48; green 38467.9 -> 38468 = 150 * 256 + 68; red 19595.7 -> 19596 = 76 * 256 + 140
    assert lm.luma(px).reshape(-1).tolist() == [29, 150, 76, 0, 1]


@pytest.mark.parametrize('dtype, channels', [(np.uint8, 3), (np.uint8, 4), (np.uint16, 3)])
def test_red_first_is_the_model_on_the_reversed_channels(dtype, channels):
    a = noise((2, 9, 11, channels), dtype, 3)
    rev = a.copy()
    rev[..., :3] = a[..., 2::-1] if channels == 3 else a[..., [2, 1, 0]]
    assert np.array_equal(lm.luma(a, red_first=True), lm.luma(rev))
    assert not np.array_equal(lm.luma(a, red_first=True), lm.luma(a))


def test_alpha_never_matters():
    a = noise((2, 7, 13, 4), np.uint8, 5)
    for alpha in (0, 255, None):
        b = a.copy()
        b[..., 3] = noise((2, 7, 13), np.uint8, 6) if alpha is None else alpha
        for red_first in (False, True):
            assert np.array_equal(lm.luma(a, red_first), lm.luma(b, red_first))
            assert np.array_equal(lm.luma(a, red_first), lm.luma(np.ascontiguousarray(a[..., :3]), red_first))


def test_within_one_of_the_real_weights():
    a = noise((4, 64, 64, 3), np.uint8, 7).astype(np.float64)
    want = np.rint(0.114 * a[..., 0] + 0.587 * a[..., 1] + 0.299 * a[..., 2])
    assert np.abs(lm.luma(a.astype(np.uint8)).astype(np.float64) - want).max() <= 1
    want = np.rint(0.114 * a[..., 2] + 0.587 * a[..., 1] + 0.299 * a[..., 0])
    assert np.abs(lm.luma(a.astype(np.uint8), red_first=True).astype(np.float64) - want).max() <= 1
    b = noise((4, 64, 64, 3), np.uint16, 8)
    y16 = np.rint(0.114 * b[..., 0].astype(np.float64) + 0.587 * b[..., 1] + 0.299 * b[..., 2])
    # the 16-bit value is within 1 of the real weights' before the high byte is taken: its high byte is that value's, or that of a neighbour
    got = lm.luma(b).astype(np.int64)
    assert ((got == (y16.astype(np.int64) - 1) >> 8) | (got == y16.astype(np.int64) >> 8) | (got == np.minimum(y16.astype(np.int64) + 1, 65535) >> 8)).all()


def test_other_inputs_have_no_rule():
    for bad in (np.zeros((2, 4, 4), np.uint8), np.zeros((2, 4, 4, 4), np.uint16), np.zeros((2, 4, 4, 3), np.float32), np.zeros((2, 4, 4, 2), np.uint8),
                np.zeros((4, 4), np.uint16)):
        with pytest.raises(ValueError, match='no luma rule'):
            lm.luma(bad)
