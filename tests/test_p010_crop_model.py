"""No GPU: tests/p010_crop_model.py pinned -- against a plain scalar-loop restatement of the definition (include/meshflow_hip.h,
mf_crop_resize_p010), against the consequences the definition has, and with the checks the GPU test relies on: that the case table
(tests/p010_crop_cases.py) holds every class of chroma sample, that its exact-2x luma cases tell INTER_AREA's form from the float path, and
that its chroma results tell float32 weights from NV12's 11-bit ones."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv16_area  # noqa: E402
import cv16_model  # noqa: E402
import nv12_crop_cases  # noqa: E402
import nv12_crop_model as sites  # noqa: E402
import p010_crop_cases as cases  # noqa: E402
import p010_crop_model as model  # noqa: E402

F32 = np.float32


def scalar_axis(lo, hi, out_len, c, clamp_weights):
    """One chroma sample of one axis, operation by operation: (s0, s1, w0, w1) with float32 weights."""
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
    else:                                               # y: the rows clipped, the fraction kept
        s0, s1 = min(max(s, c0), c1), min(max(s + 1, c0), c1)
    return s0, s1, F32(F32(1) - f), f


def scalar_chroma(uv, rect, size):
    left, top, right, bottom = rect
    oW, oH = size
    out = np.zeros((oH // 2, oW // 2, 2), dtype=np.uint16)
    for cy in range(oH // 2):
        sy0, sy1, b0, b1 = scalar_axis(top, bottom, oH, cy, False)
        for cx in range(oW // 2):
            sx0, sx1, a0, a1 = scalar_axis(left, right, oW, cx, True)
            for ch in range(2):
                t0 = F32(F32(F32(uv[sy0, sx0, ch]) * a0) + F32(F32(uv[sy0, sx1, ch]) * a1))
                t1 = F32(F32(F32(uv[sy1, sx0, ch]) * a0) + F32(F32(uv[sy1, sx1, ch]) * a1))
                v = F32(F32(t0 * b0) + F32(t1 * b1))
                out[cy, cx, ch] = min(int(np.rint(v)), 65535)
    return out


@pytest.mark.parametrize('name', ['66x50', '2x2', '2x34'])
def test_model_equals_the_scalar_restatement(name):
    c = cases.frame(name)
    picked = c['cases'] if c['W'] == 2 else c['cases'][::7]
    assert len(picked) >= 3
    for rect, size in picked:
        got = model.crop_resize_chroma(c['uv'][1], rect, size)
        assert np.array_equal(got, scalar_chroma(c['uv'][1], rect, size)), (rect, size)


def test_the_geometry_is_the_nv12_table_s():
    assert cases.NAMES == ['66x50', '64x48', '100x72', '2x2', '2x34', '640x96'] and cases.frame('64x48')['n'] == 9
    assert (1280, 190) in [s for _, s in cases.frame('640x96')['cases']]
    for name in cases.NAMES:
        c = cases.frame(name)
        assert c['cases'] == nv12_crop_cases.frame(name)['cases']
        assert c['y'].dtype == np.uint16 and c['uv'].dtype == np.uint16 and c['y'].shape == (c['n'], c['H'], c['W'])
    big = cases.frame('100x72')
    assert big['y'].max() > 65000 and big['y'].min() < 500 and big['uv'].max() > 65000 and big['uv'].min() < 500


def test_the_case_table_holds_every_class_of_sample():
    counts = cases.class_counts()
    print(counts)
    assert counts == {'x': (194, 3377, 37366), 'y': (206, 846, 9711)}
    for axis in ('x', 'y'):
        assert min(counts[axis]) > 0


def test_full_frame_at_its_own_size_is_a_copy():
    for name in cases.NAMES:
        c = cases.frame(name)
        W, H = c['W'], c['H']
        oy, ouv = model.crop_resize_frame(c['y'][0], c['uv'][0], (0, 0, W - 1, H - 1))
        assert np.array_equal(ouv, c['uv'][0]) and np.array_equal(oy, c['y'][0]), name


def test_even_corner_at_the_crop_s_own_size_is_a_copy_of_the_sub_planes():
    c = cases.frame('100x72')
    for rect in ((2, 4, 61, 51), (0, 0, 9, 9), (98, 70, 99, 71), (0, 0, 99, 71), (40, 2, 41, 71)):
        left, top, right, bottom = rect
        size = (right - left + 1, bottom - top + 1)
        assert size[0] % 2 == 0 and size[1] % 2 == 0 and left % 2 == 0 and top % 2 == 0
        oy, ouv = model.crop_resize_frame(c['y'][0], c['uv'][0], rect, size)
        assert np.array_equal(ouv, c['uv'][0][top // 2:bottom // 2 + 1, left // 2:right // 2 + 1]), rect
        assert np.array_equal(oy, c['y'][0][top:bottom + 1, left:right + 1]), rect


def test_odd_left_at_scale_one_is_the_neighbours_mean_rounded_half_to_even():
    c = cases.frame('100x72')
    uv = c['uv'][0].astype(np.int64)
    ties_to_even = 0
    for rect in ((3, 4, 62, 51), (5, 0, 98, 71), (1, 2, 98, 71)):
        left, top, right, bottom = rect
        size = (right - left + 1, bottom - top + 1)
        assert size[0] % 2 == 0 and size[1] % 2 == 0 and left % 2 == 1 and top % 2 == 0
        got = model.crop_resize_chroma(c['uv'][0], rect, size).astype(np.int64)
        c0, c1 = sites.axis_range(left, right)
        rows = uv[top // 2:bottom // 2 + 1]
        assert c0 == (left + 1) // 2 and got.shape[1] == c1 - c0 + 1
        assert np.array_equal(got[:, 0], rows[:, c0])                                  # the first column: clamped to a copy
        n = got.shape[1] - 1
        pair = rows[:, c0:c0 + n] + rows[:, c0 + 1:c0 + 1 + n]
        mean = (pair >> 1) + ((pair & 1) & ((pair >> 1) & 1))                           # half to even, in integers
        assert np.array_equal(got[:, 1:], mean)
        ties_to_even += int(((pair & 3) == 1).sum())                                    # .5 above an even number: rounded DOWN
    assert ties_to_even > 100


def test_chroma_at_exactly_2x_down_is_the_float_path_not_a_box():
    """Even left and top at exactly 2x down: f = 0.25 on both axes away from the clamps -- the float path, and not INTER_AREA's box."""
    c = cases.frame('100x72')
    rect, size = (4, 8, 67, 55), (32, 24)
    assert 2 * size[0] == rect[2] - rect[0] + 1 and 2 * size[1] == rect[3] - rect[1] + 1
    s, f = sites.axis_positions(rect[0], rect[2], size[0])
    assert f[:-1].tolist() == [0.25] * (len(f) - 1) and s.tolist() == list(range(2, 2 + 2 * len(s), 2))
    got = model.crop_resize_chroma(c['uv'][0], rect, size)
    assert np.array_equal(got, scalar_chroma(c['uv'][0], rect, size))
    sub = c['uv'][0][rect[1] // 2:rect[3] // 2 + 1, rect[0] // 2:rect[2] // 2 + 1]
    box = cv16_area.area_fast_u16(sub)
    assert box.shape == got.shape and int((box != got).sum()) > got.size // 2
    # and luma at the same case IS the area form, which differs from the float path somewhere
    oy = model.crop_resize_luma(c['y'][0], rect, size)
    crop = c['y'][0][rect[1]:rect[3] + 1, rect[0]:rect[2] + 1, None]
    assert np.array_equal(oy, cv16_area.area_fast_u16(crop)[..., 0])
    assert not np.array_equal(oy, cv16_model.resize_linear_u16(crop, *size)[..., 0])


def test_the_exact_2x_luma_cases_tell_the_area_form_from_the_float_path():
    cases_2x, differing = 0, 0
    for name in cases.NAMES:
        c = cases.frame(name)
        for rect, size in c['cases']:
            cw, ch = rect[2] - rect[0] + 1, rect[3] - rect[1] + 1
            if not cv16_area.is_area_fast(cw, ch, *size):
                continue
            cases_2x += 1
            crop = c['y'][0][rect[1]:rect[3] + 1, rect[0]:rect[2] + 1, None]
            differing += int((cv16_area.area_fast_u16(crop) != cv16_model.resize_linear_u16(crop, *size)).sum())
    print(cases_2x, 'exact-2x cases,', differing, 'luma samples where the two forms differ')
    assert cases_2x >= 6 and differing > 100


def test_chroma_tells_float32_weights_from_11_bit_weights():
    """The same positions through weights quantised to 1/2048 (cvRound(f 2048) / 2048, what a kernel that borrowed NV12's tables would
    apply) give other samples somewhere: the table can fail such a kernel."""
    def quantised(w):
        return (np.rint(w * F32(2048)) / F32(2048)).astype(F32)

    differing, compared = 0, 0
    for name in ('66x50', '100x72'):
        c = cases.frame(name)
        for rect, size in c['cases'][::3]:
            sx0, sx1, a0, a1 = model.x_table(rect[0], rect[2], size[0])
            sy0, sy1, b0, b1 = model.y_table(rect[1], rect[3], size[1])
            S = c['uv'][0].astype(F32)
            exact = model.blend(S, sx0, sx1, a0, a1, sy0, sy1, b0, b1)
            assert np.array_equal(exact, model.crop_resize_chroma(c['uv'][0], rect, size))
            coarse = model.blend(S, sx0, sx1, quantised(a0), quantised(a1), sy0, sy1, quantised(b0), quantised(b1))
            differing += int((exact != coarse).sum())
            compared += exact.size
    print(differing, 'of', compared, 'chroma samples differ under 11-bit weights')
    assert differing > 1000


def test_every_tap_lies_inside_the_crop_s_chroma_samples():
    checked = 0
    for name in cases.NAMES:
        c = cases.frame(name)
        for rect, size in c['cases']:
            left, top, right, bottom = rect
            (c0, c1), (r0, r1) = sites.axis_range(left, right), sites.axis_range(top, bottom)
            assert 0 <= c0 <= c1 < c['W'] // 2 and 0 <= r0 <= r1 < c['H'] // 2
            sx0, sx1, a0, a1 = model.x_table(left, right, size[0])
            sy0, sy1, b0, b1 = model.y_table(top, bottom, size[1])
            for s, lo, hi in ((sx0, c0, c1), (sx1, c0, c1), (sy0, r0, r1), (sy1, r0, r1)):
                assert s.min() >= lo and s.max() <= hi, (name, rect, size)
            assert np.all(a1[sx0 == c1] == 0)                                           # the crop's last column is read alone
            assert np.all((a1 >= 0) & (a1 < 1)) and np.all((b1 >= 0) & (b1 < 1))
            checked += 1
    assert checked > 300


def test_luma_is_channel_0_of_the_three_channel_resize():
    c = cases.frame('66x50')
    rect, size = (3, 2, 62, 47), (80, 70)
    oy, _ = model.crop_resize_frame(c['y'][0], c['uv'][0], rect, size)
    three = np.repeat(c['y'][0][2:48, 3:63, None], 3, axis=2)
    assert np.array_equal(oy, cv16_area.resize_u16(three, 80, 70)[..., 0])
