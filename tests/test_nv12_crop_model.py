"""No GPU: tests/nv12_crop_model.py pinned -- against a plain scalar-loop restatement of the definition (include/meshflow_hip.h,
mf_crop_resize_nv12), against the consequences the definition was prototyped to have, and with the check that every tap of every case of the
table lies in columns c0 .. c1 and rows r0 .. r1 of the chroma plane."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nv12_crop_cases as cases  # noqa: E402
import nv12_crop_model as model  # noqa: E402

F32 = np.float32


def cv_round(v):
    """cvRound of a non-negative float32: round half to even."""
    return int(np.rint(F32(v)))


def scalar_axis(lo, hi, out_len, c, clamp_weights):
    """One chroma sample of one axis, operation by operation: (s0, s1, w0, w1)."""
    cw = hi - lo + 1
    scale = 1.0 / (float(out_len) / float(cw))
    fc = F32((float(lo) + ((float(2 * c) + 0.5) * scale - 0.5)) * 0.5)
    s = int(math.floor(fc))
    f = F32(fc - F32(s))
    c1 = hi >> 1
    c0 = min((lo + 1) >> 1, c1)
    if clamp_weights:                                   # x, as cv2 clamps columns
        if s < c0:
            s, f = c0, F32(0)
        if s >= c1:
            s, f = c1, F32(0)
        s0, s1 = s, min(s + 1, c1)
    else:                                               # y: the rows clipped, the weights kept
        s0, s1 = min(max(s, c0), c1), min(max(s + 1, c0), c1)
    return s0, s1, cv_round((F32(1) - f) * F32(2048)), cv_round(f * F32(2048))


def scalar_chroma(uv, rect, size):
    left, top, right, bottom = rect
    oW, oH = size
    out = np.zeros((oH // 2, oW // 2, 2), dtype=np.uint8)
    for cy in range(oH // 2):
        sy0, sy1, b0, b1 = scalar_axis(top, bottom, oH, cy, False)
        for cx in range(oW // 2):
            sx0, sx1, a0, a1 = scalar_axis(left, right, oW, cx, True)
            for ch in range(2):
                t0 = int(uv[sy0, sx0, ch]) * a0 + int(uv[sy0, sx1, ch]) * a1
                t1 = int(uv[sy1, sx0, ch]) * a0 + int(uv[sy1, sx1, ch]) * a1
                v = (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2
                assert 0 <= v <= 255
                out[cy, cx, ch] = v
    return out


@pytest.mark.parametrize('name', ['66x50', '2x2', '2x34'])
def test_model_equals_the_scalar_restatement(name):
    c = cases.frame(name)
    picked = c['cases'] if c['W'] == 2 else c['cases'][::5]
    assert len(picked) >= 3
    for rect, size in picked:
        got = model.crop_resize_chroma(c['uv'][1], rect, size)
        assert np.array_equal(got, scalar_chroma(c['uv'][1], rect, size)), (rect, size)


def test_one_case_by_hand():
    """left = 3, right = 8 at the crop's own width 6: scale 1, fc = (3 + 2 cx) / 2 = 1.5, 2.5, 3.5; c0 = 2, c1 = 4: cx = 0 is clamped to a copy of
    column 2, the others average neighbours."""
    s0, s1, a0, a1 = model.x_table(3, 8, 6)
    assert s0.tolist() == [2, 2, 3] and s1.tolist() == [3, 3, 4]
    assert a0.tolist() == [2048, 1024, 1024] and a1.tolist() == [0, 1024, 1024]
    assert model.axis_range(5, 5) == (2, 2) and model.axis_range(4, 4) == (2, 2) and model.axis_range(3, 4) == (2, 2)
    assert model.axis_range(0, 9) == (0, 4) and model.axis_range(1, 8) == (1, 4)


def test_full_frame_at_its_own_size_is_a_copy():
    for name in cases.NAMES:
        c = cases.frame(name)
        W, H = c['W'], c['H']
        oy, ouv = model.crop_resize_frame(c['y'][0], c['uv'][0], (0, 0, W - 1, H - 1))
        assert np.array_equal(ouv, c['uv'][0]) and np.array_equal(oy, c['y'][0]), name


def test_even_corner_at_the_crop_s_own_size_is_a_copy_of_the_sub_plane():
    c = cases.frame('100x72')
    for rect in ((2, 4, 61, 51), (0, 0, 9, 9), (98, 70, 99, 71), (0, 0, 99, 71), (40, 2, 41, 71)):
        left, top, right, bottom = rect
        size = (right - left + 1, bottom - top + 1)
        assert size[0] % 2 == 0 and size[1] % 2 == 0 and left % 2 == 0 and top % 2 == 0
        ouv = model.crop_resize_chroma(c['uv'][0], rect, size)
        assert np.array_equal(ouv, c['uv'][0][top // 2:bottom // 2 + 1, left // 2:right // 2 + 1]), rect


def test_odd_left_at_scale_one_averages_horizontal_neighbours():
    c = cases.frame('100x72')
    uv = c['uv'][0].astype(np.int64)
    for rect in ((3, 4, 62, 51), (5, 0, 98, 71), (1, 2, 98, 71)):
        left, top, right, bottom = rect
        size = (right - left + 1, bottom - top + 1)
        assert size[0] % 2 == 0 and size[1] % 2 == 0 and left % 2 == 1 and top % 2 == 0
        got = model.crop_resize_chroma(c['uv'][0], rect, size).astype(np.int64)
        c0, c1 = model.axis_range(left, right)
        rows = uv[top // 2:bottom // 2 + 1]
        assert c0 == (left + 1) // 2 and got.shape[1] == c1 - c0 + 1
        assert np.array_equal(got[:, 0], rows[:, c0])                                  # the first column: clamped to a copy
        n = got.shape[1] - 1
        assert np.array_equal(got[:, 1:], (rows[:, c0:c0 + n] + rows[:, c0 + 1:c0 + 1 + n] + 1) >> 1)


def test_every_tap_lies_inside_the_crop_s_chroma_samples():
    checked = 0
    for name in cases.NAMES:
        c = cases.frame(name)
        for rect, size in c['cases']:
            left, top, right, bottom = rect
            (c0, c1), (r0, r1) = model.axis_range(left, right), model.axis_range(top, bottom)
            assert 0 <= c0 <= c1 < c['W'] // 2 and 0 <= r0 <= r1 < c['H'] // 2
            assert 2 * c1 <= right and 2 * r1 <= bottom and (2 * c0 >= left or c0 == c1) and (2 * r0 >= top or r0 == r1)
            sx0, sx1, a0, a1 = model.x_table(left, right, size[0])
            sy0, sy1, b0, b1 = model.y_table(top, bottom, size[1])
            for s, lo, hi in ((sx0, c0, c1), (sx1, c0, c1), (sy0, r0, r1), (sy1, r0, r1)):
                assert s.min() >= lo and s.max() <= hi, (name, rect, size)
            assert np.all(a0 + a1 >= 2047) and np.all(a0 + a1 <= 2049) and np.all(b0 + b1 >= 2047) and np.all(b0 + b1 <= 2049)
            assert np.all(a1[sx0 == c1] == 0)                                           # the crop's last column is read alone
            checked += 1
    assert checked > 300


def test_the_case_table_holds_every_class_of_sample():
    counts = cases.class_counts()
    print(counts)
    for axis in ('x', 'y'):
        low, high, interior = counts[axis]
        assert low > 0 and high > 0 and interior > 0, counts


def test_luma_is_the_grey_crop_resize():
    from oracle import meshflow_oracle as mo
    c = cases.frame('66x50')
    rect, size = (3, 2, 62, 47), (80, 70)
    oy, _ = model.crop_resize_frame(c['y'][0], c['uv'][0], rect, size)
    three = np.repeat(c['y'][0][2:48, 3:63, None], 3, axis=2)
    assert np.array_equal(oy, mo.resize_linear_u8(three, 80, 70)[..., 1])
