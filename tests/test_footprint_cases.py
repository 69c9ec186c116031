"""No GPU: tests/footprint_cases.py before any kernel result is looked at -- every case holds border, partly-outside and deep-interior samples
in every model's output (luma-sized and chroma planes), the restated deep-interior rule agrees with nv12_model.tap_classes sample by sample,
and the per-footprint tail map is what that rule gives wavefront by wavefront."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint_cases as fc  # noqa: E402
import nv12_model  # noqa: E402


def test_the_table_s_own_rules():
    assert len(set(fc.NAMES)) == len(fc.CASES)
    for F, H, W, R, C, jitter, kind, seed in fc.CASES:
        assert W % 4 == 0 and H % 2 == 0 and W <= 512 and H <= 288 and F >= 2
    cells = [(W / C, H / R) for F, H, W, R, C, *_ in fc.CASES]
    assert any(cw >= 2 * 32 and ch >= 2 * 8 for cw, ch in cells), 'no case with cells well above a footprint'
    assert any(cw < 32 and ch < 8 for cw, ch in cells), 'no case with cells below a footprint'


@pytest.mark.parametrize('name', fc.NAMES)
def test_every_sample_class_in_every_output(name):
    c = fc.case_for(name)
    W, H, F = c['W'], c['H'], c['F']
    luma = nv12_model.tap_classes(c['mx'], c['my'], W, H)
    chroma = nv12_model.tap_classes(c['cmx'], c['cmy'], W // 2, H // 2)
    print(name, 'luma', [int(m.sum()) for m in luma], 'chroma', [int(m.sum()) for m in chroma], 'of', luma[0].size, chroma[0].size)
    for border, partly, deep in (luma, chroma):
        assert border.any() and partly.any() and deep.any(), (name, 'the case cannot fail in every class')
    border, partly, deep = luma
    # the float32 plane and P010 luma: the border value wherever the 2 x 2 taps lie wholly outside, something else among the partly-outside
    # and the deep samples -- and nothing but the plane's own samples where all four taps lie inside
    for fmt, fill in (('plane_f32', np.float32(fc.FILL_F32)), ('u16c1', fc.BORDER_P010[0]), ('nv12_y', fc.BORDER_NV12[0])):
        w = c['want'][fmt]
        assert (w[border] == fill).all() and (w[partly] != fill).any() and (w[deep] != fill).any(), (name, fmt)
    cborder, cpartly, cdeep = chroma
    for fmt, fill in (('nv12_uv', fc.BORDER_NV12[1:]), ('p010_uv', fc.BORDER_P010[1:])):
        w = c['want'][fmt]
        is_fill = (w == np.asarray(fill, w.dtype)).all(axis=-1)
        assert is_fill[cborder].all() and not is_fill[cpartly].all() and not is_fill[cdeep].all(), (name, fmt)
        assert np.array_equal(c['live'][fmt][:, ::2, ::2], ~is_fill) and not c['live'][fmt][:, 1::2, :].any() and not c['live'][fmt][:, :, 1::2].any()
    # nearest: the element under the rounded coordinate, the fill where that lies outside -- both occur, and an unowned pixel gives the fill
    unowned = ~c['live']['maps']
    assert unowned.any() and not unowned.all()
    for es in fc.UINT:
        w = c['want']['plane_n%d' % es]
        assert (w[unowned] == fc.FILL[es][1]).all() and (w == fc.FILL[es][1]).any() and (w != fc.FILL[es][1]).any()
        assert not (c['labels'][es] == fc.FILL[es][1]).any()
    assert np.array_equal(c['want']['maps'][..., 0], c['mx']) and c['want']['maps'].shape == (F, H, W, 2)
    for a in (c['mx'], c['planes'], c['want']['u16c1'], c['tail_fast']['luma']):
        assert not a.flags.writeable


@pytest.mark.parametrize('name', fc.NAMES)
def test_tail_map_agrees_with_tap_classes(name):
    """The deep-interior rule restated from warp_coords.h (raw float bits, unsigned compare) against nv12_model.tap_classes' (cvRound, shift,
    2 <= ix <= W - 3) on the chroma plane and on the luma plane, sample by sample; then the footprint map against a loop over footprints."""
    c = fc.case_for(name)
    W, H, F = c['W'], c['H'], c['F']
    Wc, Hc = W // 2, H // 2
    assert np.array_equal(fc.deep_interior(c['cmx'], c['cmy'], Wc, Hc), nv12_model.tap_classes(c['cmx'], c['cmy'], Wc, Hc)[2])
    assert np.array_equal(fc.deep_interior(c['mx'], c['my'], W, H), nv12_model.tap_classes(c['mx'], c['my'], W, H)[2])
    deep_l = nv12_model.tap_classes(c['mx'], c['my'], W, H)[2]
    deep_c = nv12_model.tap_classes(c['cmx'], c['cmy'], Wc, Hc)[2]
    fast_l, fast_c = c['tail_fast']['luma'], c['tail_fast']['chroma']
    assert fast_l.shape == fast_c.shape == c['whole'].shape == (F, (H + 7) // 8, (W + 31) // 32)
    for f in range(F):
        for ty in range(fast_l.shape[1]):
            for tx in range(fast_l.shape[2]):
                ys, xs = slice(8 * ty, min(8 * ty + 8, H)), slice(32 * tx, min(32 * tx + 32, W))
                assert fast_l[f, ty, tx] == deep_l[f, ys, xs].all()
                # the footprint's emitting chroma samples: rows 4 ty .. 4 ty + 3, columns 16 tx .. 16 tx + 15 of the chroma plane
                assert fast_c[f, ty, tx] == deep_c[f, 4 * ty:min(4 * ty + 4, Hc), 16 * tx:min(16 * tx + 16, Wc)].all()
    assert fast_l.any() and not fast_l.all() and fast_c.any() and not fast_c.all(), (name, 'one tail form only')
    # (neither map implies the other: a luma-deep source 2 to 4 pixels from the edge halves to a chroma position that is not deep, and only
    # the even pixels of the even rows count for chroma)
    for fmt, plane in fc.TWO_FORM_TAILS.items():
        names = fc.tail_names(c, fmt)
        assert np.array_equal(names == 'fast', c['tail_fast'][plane]) and set(np.unique(names)) == {'fast', 'clamped'}
    assert set(np.unique(fc.tail_names(c, 'maps'))) == {'one'}


def test_deep_interior_at_the_rule_s_edges():
    """The rule on hand-picked coordinates: the first and last deep position in 1/32 pixel steps, ties of the rounding (half to even), a plane
    too small to hold a deep sample, and values outside the fixed-point trick's range."""
    W, H = 40, 12
    v = np.float32(5.0)
    cases = [(2.0, True), (2.0 - 1 / 64, True), (2.0 - 3 / 64, False),       # 32 u = 63.5 -> 64 (even): deep; 62.5 -> 62: not
             (1.97, False), (W - 2 - 1 / 32, True), (W - 2 - 1 / 64, False),   # 32 u = 32 (W - 2) - 0.5 -> 32 (W - 2) (even): ix = W - 2
             (W - 2.0, False), (-0.25, False), (float(W + 1), False), (3e6, False), (-3e6, False), (np.inf, False), (np.nan, False)]
    for u, want in cases:
        assert bool(fc.deep_interior(np.float32(u), v, W, H)) == want, u
        assert bool(fc.deep_interior(v, np.float32(u), H, W)) == want, u   # the same rule for rows
    assert not fc.deep_interior(np.float32(2.0), np.float32(2.0), 4, 40) and not fc.deep_interior(np.float32(2.0), np.float32(2.0), 40, 4)
    assert fc.deep_interior(np.float32(2.0), np.float32(2.0), 5, 5)


def test_the_midpoint_case_sits_on_float32_midpoints():
    """Owned by the top-left cell, whose inverse homography is an exact shear, every footprint of columns 32 .. 63 above the mesh's middle row
    holds coordinates on which the cheap chain must refuse; a translation by a multiple of 1/32 pixel holds none anywhere."""
    c = fc.case_for(fc.MIDPOINT)
    hi = c['records'][:, 0, 9:18]
    for f, (bx, by) in enumerate(fc.BY_NAME[fc.MIDPOINT][6][1]):
        # (the u row and the denominator to the last bit; the v row's offset carries the solve's own 1e-14)
        assert hi[f, :3].tolist() == [1.0, 2.0 ** -18, bx + by * 2.0 ** -18] and hi[f, 6:].tolist() == [0.0, 0.0, 1.0]
        assert hi[f, 3:5].tolist() == [0.0, 1.0] and abs(hi[f, 5] - by) < 1e-13
    must = fc.cheap_chain_must_refuse(c['records'], np.zeros(c['whole'].shape, np.int64), c['H'], c['W'])
    assert must[:, :9, 1].all() and not must[:, :, 4:].any()            # (64 <= u: the midpoints are those of other rows' values, if any)
    plain = fc.case_for('256x144_2x2_translate_25')
    assert not fc.cheap_chain_must_refuse(plain['records'], np.zeros(plain['whole'].shape, np.int64), plain['H'], plain['W']).any()
