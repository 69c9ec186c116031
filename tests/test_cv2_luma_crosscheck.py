"""tests/luma_model.py against cv2.cvtColor for the three colour sources -- the only place where the model's constants, restated from memory of
OpenCV's source, can be settled.  Skips without OpenCV.  The 16-bit source is compared before the high byte is taken: cv2 has no rule for
that step (its FAST takes no 16-bit image), the model's is truncation."""
import os
import sys

import numpy as np
import pytest

cv2 = pytest.importorskip('cv2')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import luma_model as lm  # noqa: E402


def noise(shape, dtype, seed):
    from meshflow_amd import synthetic
    return (synthetic.hash32(np.arange(int(np.prod(shape))), seed) % (np.iinfo(dtype).max + 1)).astype(dtype).reshape(shape)


def levels(dtype):
    """Every channel over its whole range (8-bit: every level) with the other two at both ends."""
    top = np.iinfo(dtype).max
    ramp = np.arange(256) if dtype == np.uint8 else np.concatenate([np.arange(0, 65536, 251), np.arange(255, 65536, 256), [32767, 32768, 65535]])
    px = np.zeros((3, 2, len(ramp), 3), dtype)
    for c in range(3):
        for k, other in enumerate((0, top)):
            px[c, k] = other
            px[c, k, :, c] = ramp
    return px.reshape(6, len(ramp), 3)


@pytest.mark.parametrize('red_first', [False, True])
def test_bgr_uint8(red_first):
    code = cv2.COLOR_RGB2GRAY if red_first else cv2.COLOR_BGR2GRAY
    for img in (noise((96, 128, 3), np.uint8, 1), levels(np.uint8)):
        assert np.array_equal(lm.luma(img[None], red_first)[0], cv2.cvtColor(img, code))


@pytest.mark.parametrize('red_first', [False, True])
def test_bgra_uint8(red_first):
    code = cv2.COLOR_RGBA2GRAY if red_first else cv2.COLOR_BGRA2GRAY
    img = noise((96, 128, 4), np.uint8, 2)
    assert np.array_equal(lm.luma(img[None], red_first)[0], cv2.cvtColor(img, code))


@pytest.mark.parametrize('red_first', [False, True])
def test_bgr_uint16(red_first):
    code = cv2.COLOR_RGB2GRAY if red_first else cv2.COLOR_BGR2GRAY
    for img in (noise((96, 128, 3), np.uint16, 3), levels(np.uint16)):
        y16 = cv2.cvtColor(img, code)
        assert y16.dtype == np.uint16
        assert np.array_equal(lm.luma(img[None], red_first)[0], (y16 >> 8).astype(np.uint8))
