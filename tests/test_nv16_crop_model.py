"""CPU: tests/nv16_crop_model.py, the NumPy model of the NV16 crop-resize, against the consequences the contract names
(include/meshflow_hip.h, mf_crop_resize_nv16) -- the full frame at its own size is a copy, an even-left rectangle at its own size is a copy of
the sub-plane for any top, and at x identity the y axis is luma's byte for byte --, the case table's coverage, and four mutants of the model
that the table must tell from it: rows halved, rows not offset by top, c0 / c1 taken from the plane instead of the crop, U and V swapped."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nv12_crop_model as nv12  # noqa: E402
import nv16_crop_cases as cases  # noqa: E402
import nv16_crop_model as model  # noqa: E402
from oracle import meshflow_oracle as mo  # noqa: E402


def test_the_x_axis_is_the_nv12_model_s_own():
    assert model.x_table is nv12.x_table and model.axis_range is nv12.axis_range


@pytest.mark.parametrize('name', cases.NAMES)
def test_full_frame_at_its_own_size_is_a_copy(name):
    c = cases.frame(name)
    W, H = c['W'], c['H']
    oy, ouv = cases.want(name, (0, 0, W - 1, H - 1), (W, H))
    assert np.array_equal(oy, c['y']) and np.array_equal(ouv, c['uv'])


@pytest.mark.parametrize('name', ['66x49', '100x71', '2x35'])
def test_even_left_rectangle_at_its_own_size_is_a_copy_of_the_sub_plane(name):
    c = cases.frame(name)
    W, H = c['W'], c['H']
    n = 0
    for left in range(0, W - 1, 2):
        for right in sorted({left + 1, W - 1, min(left + 5, W - 1)}):
            if (right - left + 1) % 2:
                continue
            for top, bottom in ((0, H - 1), (1, H - 1), (2, H - 2), (3, 4), (H - 2, H - 1)):
                if not 0 <= top < bottom < H:
                    continue
                rect, size = (left, top, right, bottom), (right - left + 1, bottom - top + 1)
                got = model.crop_resize_chroma(c['uv'][0], rect, size)
                assert np.array_equal(got, c['uv'][0][top:bottom + 1, left // 2:right // 2 + 1]), rect
                n += 1
    assert n >= 3


@pytest.mark.parametrize('name', ['66x49', '100x71', '64x48'])
def test_at_x_identity_the_y_axis_is_luma_s(name):
    """left even and oW == cw: plant U into the even columns of a grey plane; out_u[:, cx] is then crop_resize(grey)[:, 2 cx]."""
    c = cases.frame(name)
    W, H = c['W'], c['H']
    uv = c['uv'][0]
    grey = np.array(c['y'][0], copy=True)
    grey[:, 0::2] = uv[..., 0]
    checked = 0
    for rect in ((0, 0, W - 1, H - 1), (2, 3, W - 3, H - 4), (4, 1, W - 1, H - 1), (6, 5, 9, 5), (2, 2, W - 3, H - 3)):
        left, top, right, bottom = rect
        cw, ch = right - left + 1, bottom - top + 1
        assert left % 2 == 0 and cw % 2 == 0
        for oH in (H, ch, 2 * ch + 1, max(2, ch // 2), max(2, ch // 5), 3):
            out = model.crop_resize_chroma(uv, rect, (cw, oH))
            lum = mo.resize_linear_u8(grey[top:bottom + 1, left:right + 1, None], cw, oH)[..., 0]
            assert np.array_equal(out[..., 0], lum[:, 0::2]), (rect, oH)
            checked += 1
    assert checked == 30


def test_the_table_holds_every_class_of_sample():
    counts = cases.class_counts()
    for axis in ('x', 'y'):
        assert min(counts[axis]) > 0, counts
    all_sizes = {s for name in cases.NAMES for _, s in cases.frame(name)['cases']}
    assert any(s[1] % 2 for s in all_sizes) and (2, 3) in all_sizes and (2, 2) in all_sizes and (1280, 189) in all_sizes
    for name in cases.NAMES:
        c = cases.frame(name)
        rects = {r for r, _ in c['cases']}
        assert (0, 0, c['W'] - 1, c['H'] - 1) in rects
        if min(c['W'], c['H']) > 16:
            assert {(r[0] % 2, r[1] % 2, r[2] % 2, r[3] % 2) for r in rects} >= {(a, b, p, q) for a in (0, 1) for b in (0, 1) for p in (0, 1) for q in (0, 1)}
            assert (5, 7, 5, 7) in rects and (c['W'] - 1, c['H'] - 1, c['W'] - 1, c['H'] - 1) in rects


def test_unclamped_rows_are_the_luma_table_s():
    for top, bottom, oH in ((0, 48, 49), (3, 45, 71), (7, 7, 5), (1, 34, 3), (2, 94, 189)):
        s0, s1, b0, b1 = model.y_table(top, bottom, oH)
        ch = bottom - top + 1
        sy, fy = mo.resize_linear_tables(ch, oH)
        w0, w1 = mo._coef(fy)
        assert np.array_equal(s0, top + np.clip(sy, 0, ch - 1)) and np.array_equal(s1, top + np.clip(sy + 1, 0, ch - 1))
        assert np.array_equal(b0, w0) and np.array_equal(b1, w1)
        assert s0.min() >= top and s1.max() <= bottom and len(s0) == oH


@pytest.mark.parametrize('mutant', ['halve_rows', 'forget_top', 'plane_range', 'swap_uv'])
def test_mutants_are_rejected_by_the_table(mutant):
    """Each mutant differs from the model on some case of the table (so a kernel with that mistake fails the GPU test), and the two small
    frames alone already tell."""
    rejected = 0
    for name in ('66x49', '100x71'):
        c = cases.frame(name)
        for rect, size in c['cases']:
            want = cases.want(name, rect, size)[1][0]
            got = model.crop_resize_chroma(c['uv'][0], rect, size, **{mutant: True})
            rejected += int(not np.array_equal(got, want))
    assert rejected > 0, mutant
    # and where the mutation is the identity the mutant IS the model: the check is not vacuous the other way round
    c = cases.frame('66x49')
    full = (0, 0, c['W'] - 1, c['H'] - 1)
    if mutant in ('forget_top', 'plane_range'):
        assert np.array_equal(model.crop_resize_chroma(c['uv'][0], full, (66, 49), **{mutant: True}), c['uv'][0])
