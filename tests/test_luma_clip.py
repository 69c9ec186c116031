"""What tests/test_gpu_luma_pipeline.py relies on, checked without a GPU: the model luma (tests/luma_model.py) of tests/luma_clip.py's colour
clip, in both channel orders and from its 16-bit form, fits a homography for every adjacent pair in the tests' own model pipeline, and so do
the pairs (luma of the clip, luma of the colour clip cropped and scaled back by the oracle)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homography_model as hm  # noqa: E402
import luma_clip as lc  # noqa: E402
import luma_model as lm  # noqa: E402

RECTS = ((8, 6, 119, 89), (4, 3, 123, 92))          # inclusive (left, top, right, bottom), two of tests/test_gpu_scores.py's


def test_the_colour_clip_differs_by_channel_and_order():
    g = lc.grey()
    colour = lc.bgr(g)
    y, y_red_first = lm.luma(colour), lm.luma(colour, red_first=True)
    assert not np.array_equal(y, g) and not np.array_equal(y, y_red_first)
    assert np.abs(y.astype(np.float64) - (0.772 * g + 29)).max() <= 1.0           # 0.587 + 0.299 - 0.114 = 0.772, 255 * 0.114 = 29.07
    assert np.array_equal(lm.luma(lc.reversed_channels(colour), red_first=True), y)
    assert np.array_equal(lm.luma(lc.bgra(g)), y)
    d_y, d_uv = lc.p010(g)
    assert np.array_equal(lm.luma(d_y), g) and (d_y & 0x3F).any() and d_uv.shape == (6, 48, 64, 2)


def test_every_pair_of_the_model_luma_fits_a_homography():
    from oracle import meshflow_oracle as mo
    g = lc.grey()
    colour = lc.bgr(g)
    for red_first in (False, True):
        y = lm.luma(colour, red_first)
        assert (lc.model_fit_records(y[:-1], y[1:])[:, 0] == hm.OK).all(), red_first
        for rect in RECTS:
            cropped = lm.luma(np.stack(mo.crop_frames(list(colour), rect)), red_first)
            assert (lc.model_fit_records(y, cropped)[:, 0] == hm.OK).all(), (red_first, rect)
    y16 = lm.luma(lc.bgr16(g))
    assert (lc.model_fit_records(y16[:-1], y16[1:])[:, 0] == hm.OK).all()
