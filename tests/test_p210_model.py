"""CPU: tests/p210_model.py, the NumPy models of the P210 warp, the P210 crop-resize and the Y210 pack / unpack, against the consequences
the contract names (include/meshflow_hip.h) -- the models are compositions of the pinned ones, the full frame at its own size is a copy, luma
takes the box at exactly 2x and chroma does not --, the case tables' coverage, and six planted mutants of the crop model that the table must
tell from it: chroma rows halved, `top` forgotten, U and V swapped, x weights quantised to 2048ths, an area box for chroma at exactly 2x, the
clamp range taken from the plane instead of the crop."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv16_area  # noqa: E402
import cv16_model  # noqa: E402
import nv16_model  # noqa: E402
import p010_crop_model  # noqa: E402
import p010_model  # noqa: E402
import p210_cases  # noqa: E402
import p210_crop_cases as cases  # noqa: E402
import p210_model as model  # noqa: E402
from oracle import meshflow_oracle as mo  # noqa: E402

MUTANTS = ['halve_rows', 'forget_top', 'swap_uv', 'quantise_x', 'area_box', 'plane_range']


def test_the_models_are_compositions_of_the_pinned_ones():
    assert model.chroma_maps is nv16_model.chroma_maps and model.tap_classes is nv16_model.tap_classes
    assert model.remap_luma is p010_model.remap_luma and model.remap_chroma is p010_model.remap_chroma
    assert model.x_table is p010_crop_model.x_table and model.crop_resize_luma is p010_crop_model.crop_resize_luma


@pytest.mark.parametrize('name', ['2x2_tiny', '4x3_tiny', '66x49_2x2_shift'])
def test_warp_cases_hold_the_definition(name):
    """chroma of frame 0 is p010's remap at nv16's maps; a sample whose taps are all outside is the border word itself"""
    c = p210_cases.case_for(name)
    cmx, cmy = nv16_model.chroma_maps(c['mx'][0], c['my'][0])
    assert cmx.shape == (c['H'], c['W'] // 2)
    assert np.array_equal(cmx, c['mx'][0][:, 0::2] * np.float32(0.5)) and np.array_equal(cmy, c['my'][0][:, 0::2])
    got_y, got_uv = model.warp_frame(c['y'][0], c['uv'][0], c['mx'][0], c['my'][0], p210_cases.BORDER)
    assert np.array_equal(got_y, c['want_y'][0]) and np.array_equal(got_uv, c['want_uv'][0])
    assert got_uv.dtype == np.uint16 and got_uv.shape == c['uv'][0].shape
    border, _, _ = model.tap_classes(cmx, cmy, c['W'] // 2, c['H'])
    assert (got_uv[border] == np.asarray(p210_cases.BORDER[1:], np.uint16)).all()


def test_warp_case_names_are_nv16_s():
    import nv16_cases
    assert p210_cases.NAMES == nv16_cases.NAMES and {'2x2_tiny', '4x3_tiny', '2x33_tiny'} <= set(p210_cases.NAMES)
    assert sum(n.startswith('golden_') for n in p210_cases.NAMES) >= 1


@pytest.mark.parametrize('name', cases.NAMES)
def test_full_frame_at_its_own_size_is_a_copy(name):
    c = cases.frame(name)
    W, H = c['W'], c['H']
    oy, ouv = cases.want(name, (0, 0, W - 1, H - 1), (W, H))
    assert np.array_equal(oy, c['y']) and np.array_equal(ouv, c['uv'])


def test_rows_are_the_16_bit_luma_table_s():
    for top, bottom, oH in ((0, 48, 49), (3, 45, 71), (7, 7, 5), (1, 34, 3), (2, 94, 189)):
        s0, s1, b0, b1 = model.y_table(top, bottom, oH)
        ch = bottom - top + 1
        sy, fy = mo.resize_linear_tables(ch, oH)
        assert np.array_equal(s0, top + np.clip(sy, 0, ch - 1)) and np.array_equal(s1, top + np.clip(sy + 1, 0, ch - 1))
        assert b0.dtype == np.float32 and np.array_equal(b1, fy.astype(np.float32)) and np.array_equal(b0, np.float32(1) - b1)
        assert s0.min() >= top and s1.max() <= bottom and len(s0) == oH


@pytest.mark.parametrize('name', ['66x49', '100x71', '64x48'])
def test_at_x_identity_the_y_axis_is_the_16_bit_luma_resize(name):
    """left even and oW == cw, away from exactly 2x: plant U into the even columns of a grey plane; out_u[:, cx] is then the luma resize's
    column 2 cx."""
    c = cases.frame(name)
    W, H = c['W'], c['H']
    uv = c['uv'][0]
    grey = np.array(c['y'][0], copy=True)
    grey[:, 0::2] = uv[..., 0]
    checked = 0
    for rect in ((0, 0, W - 1, H - 1), (2, 3, W - 3, H - 4), (4, 1, W - 1, H - 1), (6, 5, 9, 5), (2, 2, W - 3, H - 3)):
        left, top, right, bottom = rect
        cw, ch = right - left + 1, bottom - top + 1
        for oH in (H, ch, 2 * ch + 1, max(2, ch // 2), max(2, ch // 5), 3):
            out = model.crop_resize_chroma(uv, rect, (cw, oH))
            lum = cv16_model.resize_linear_u16(grey[top:bottom + 1, left:right + 1, None], cw, oH)[..., 0]
            assert np.array_equal(out[..., 0], lum[:, 0::2]), (rect, oH)
            checked += 1
    assert checked == 30


def test_luma_takes_the_box_at_exactly_2x_and_chroma_does_not():
    seen = 0
    for name in ('64x48', '100x71'):
        c = cases.frame(name)
        for rect, size in c['cases']:
            if not cases.is_exact_2x(rect, size):
                continue
            left, top, right, bottom = rect
            oy, ouv = cases.want(name, rect, size)
            assert np.array_equal(oy[0], cv16_area.area_fast_u16(c['y'][0][top:bottom + 1, left:right + 1, None])[..., 0])
            assert not np.array_equal(oy[0], cv16_model.resize_linear_u16(c['y'][0][top:bottom + 1, left:right + 1, None], *size)[..., 0])
            assert np.array_equal(ouv[0], model.crop_resize_chroma(c['uv'][0], rect, size))
            seen += 1
    assert seen >= 2


def test_the_table_holds_every_class_of_sample():
    counts = cases.class_counts()
    for axis in ('x', 'y'):
        assert min(counts[axis]) > 0, counts
    all_sizes = {s for name in cases.NAMES for _, s in cases.frame(name)['cases']}
    assert any(s[1] % 2 for s in all_sizes) and (2, 3) in all_sizes and (2, 2) in all_sizes and (1280, 189) in all_sizes
    assert any(cases.is_exact_2x(r, s) for name in cases.NAMES for r, s in cases.frame(name)['cases'])
    assert [cases.frame(n)['n'] for n in cases.NAMES].count(9) == 1 and cases.frame('66x49')['uv'].shape[2] == 33
    for name in cases.NAMES:
        c = cases.frame(name)
        assert c['y'].dtype == np.uint16 and c['uv'].dtype == np.uint16 and int(c['uv'].max()) > 255      # (samples use both bytes)
        assert (0, 0, c['W'] - 1, c['H'] - 1) in {r for r, _ in c['cases']}


@pytest.mark.parametrize('mutant', MUTANTS)
def test_mutants_are_rejected_by_the_table(mutant):
    """Each mutant differs from the model on some case of the table (so a kernel with that mistake fails the GPU test), and the small frames
    alone already tell."""
    rejected = 0
    for name in ('66x49', '100x71', '64x48'):
        c = cases.frame(name)
        for rect, size in c['cases']:
            want = cases.want(name, rect, size)[1][0]
            got = model.crop_resize_chroma(c['uv'][0], rect, size, **{mutant: True})
            rejected += int(got.shape != want.shape or not np.array_equal(got, want))
    assert rejected > 0, mutant
    # and where the mutation is the identity the mutant IS the model: the check is not vacuous the other way round
    c = cases.frame('66x49')
    full = (0, 0, c['W'] - 1, c['H'] - 1)
    if mutant in ('forget_top', 'plane_range', 'area_box'):
        assert np.array_equal(model.crop_resize_chroma(c['uv'][0], full, (66, 49), **{mutant: True}), c['uv'][0])


def test_y210_models_by_round_trip_and_by_slicing():
    rng = np.random.default_rng(210)
    for shape in ((1, 1, 2), (2, 3, 6), (3, 5, 34)):
        n, H, W = shape
        packed = rng.integers(0, 65536, (n, H, W, 2), dtype=np.uint16)
        y, uv = model.unpack_y210(packed)
        assert y.shape == (n, H, W) and uv.shape == (n, H, W // 2, 2)
        flat = packed.reshape(-1, 4)                                  # the stream of words Y0 U Y1 V
        assert np.array_equal(y.reshape(-1, 2), flat[:, [0, 2]]) and np.array_equal(uv.reshape(-1, 2), flat[:, [1, 3]])
        assert np.array_equal(model.pack_y210(y, uv), packed)
        y2, uv2 = model.unpack_y210(model.pack_y210(y, uv))
        assert np.array_equal(y2, y) and np.array_equal(uv2, uv)
