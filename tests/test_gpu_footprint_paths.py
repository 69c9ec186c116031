"""-m gpu: the warps that take the plan's hot and pair shortcuts without an LDS window (warp_body.h, NOWIN) -- `ops.warp_maps`,
`ops.warp_planes` (linear, and nearest at 1, 2, 4 and 8 bytes), `ops.warp_p010` (luma and chroma) and `ops.warp_nv12` (chroma) -- held to their
footprint paths on tests/footprint_cases.py's geometries.

Per case the table is built once, the device's plan decoded (tests/plan_words.footprint_class_map) and every format compared bit for bit with
its CPU model over the whole output; a mismatch is reported per plan class and tail form.  The census test then shows that the comparison is
not vacuous: per format, over the cases, the plan classes and tail forms listed below each hold a whole footprint whose expected samples are
not all border / fill.  What the code rules out is asserted to be empty.

The plan does not record whether cell_coords_fast kept its result on a HOT | FAST64 footprint or refused at run time (its midpoint guard) and
cell_coords<false> ran.  One case is built so that it must refuse (test_the_cheap_chain_refuses_at_run_time says how).  Unproven here: inside
a pair footprint, whether a pixel fell into the edge's float32 error band and the general code decided."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint_cases as fc  # noqa: E402
import plan_words as pw  # noqa: E402

SIGNED = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}          # what torch.from_numpy takes for the same bytes
CERTIFIED = ('hot_fast64', 'hot_plain', 'pair', 'multi', 'border')     # the classes cell_table.hip gives to whole footprints only
SHORTCUT = ('hot_fast64', 'hot_plain', 'pair')                         # ... and those whose region is DEEP: the shortcuts of the NOWIN warps


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def to_dev(a, dev):
    """A NumPy stack on the device, unsigned element types of 4 and 8 bytes as the signed torch dtype of the same bytes."""
    a = np.array(a, copy=True)                                          # (a writable copy: the cases' arrays are read-only)
    if a.dtype in (np.uint32, np.uint64):
        a = a.view(SIGNED[a.dtype.itemsize])
    return torch.from_numpy(a).to(dev)


def raw(t):
    """The tensor's bytes on the host, as unsigned integers of the element's size."""
    a = t.detach().cpu().contiguous()
    return a.view(torch.uint8).numpy().view(fc.UINT[t.element_size()]).reshape(tuple(t.shape))


_TABLES = {}


def device_case(dev, name):
    """(case, its table -- built once --, the plan's class per footprint and per luma pixel)."""
    if name not in _TABLES:
        from meshflow_amd import ops
        c = fc.case_for(name)
        d64 = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, copy=True)).to(dev)  # noqa: E731  (a copy: the case's arrays are read-only)
        table = ops.cell_table(d64(c['disp']), d64(c['stab']), c['W'], c['H'], c['R'], c['C'])
        torch.cuda.synchronize()
        table.check()
        cmap = pw.footprint_class_map(table)
        cmap.setflags(write=False)
        _TABLES[name] = (c, table, cmap, pw.per_pixel(cmap, c['H'], c['W']))
    return _TABLES[name]


def run_formats(dev, c, table, views=None):
    """Every format of the family on `table`: {format: the result as unsigned integers}, the chroma planes and the maps with their channels
    last.  views: {tensor name: function(tensor) -> the tensor to pass instead} for inputs ('planes', 'n1' .., 'y16', 'uv16', 'uv8') and
    outputs ('out_' + format)."""
    from meshflow_amd import ops
    views = views or {}

    def arg(key, t):
        return views[key](t) if key in views else t

    def out(key, like):
        return views[key](torch.empty_like(like)) if key in views else None

    got = {}
    m = ops.warp_maps(table, out=out('out_maps', torch.empty((c['F'], c['H'], c['W'], 2), dtype=torch.float32, device=dev)))
    got['maps'] = raw(m)
    p = to_dev(c['planes'], dev)
    got['plane_f32'] = raw(ops.warp_planes(arg('planes', p), table, 'linear', fill=fc.FILL_F32, out=out('out_plane_f32', p)))
    for es in fc.UINT:
        p = to_dev(c['labels'][es], dev)
        got['plane_n%d' % es] = raw(ops.warp_planes(arg('n%d' % es, p), table, 'nearest', fill=fc.FILL[es][0], out=out('out_plane_n%d' % es, p)))
    y, uv = to_dev(c['y16'], dev), to_dev(c['uv16'], dev)
    o = (out('out_u16c1', y), out('out_p010_uv', uv))
    oy, ouv = ops.warp_p010(arg('y16', y), arg('uv16', uv), table, fc.BORDER_P010, out=None if o[0] is None else o)
    got['u16c1'], got['p010_uv'] = raw(oy), raw(ouv)
    y, uv = to_dev(c['y8'], dev), to_dev(c['uv8'], dev)
    o = out('out_nv12_uv', uv)
    oy, ouv = ops.warp_nv12(y, arg('uv8', uv), table, fc.BORDER_NV12, out=None if o is None else (torch.empty_like(y), o))
    got['nv12_y'], got['nv12_uv'] = raw(oy), raw(ouv)
    torch.cuda.synchronize()
    table.check()
    return got


def want_bits(c, fmt):
    w = np.ascontiguousarray(c['want'][fmt])
    return w.view(fc.UINT[w.dtype.itemsize])


def luma_grid(c, diff):
    """A mismatch mask of any format's shape on the luma pixel grid (F, H, W): channels folded, a chroma sample at its pixel (2 cx, 2 cy)."""
    if diff.ndim == 4:
        diff = diff.any(axis=-1)
    if diff.shape == (c['F'], c['H'], c['W']):
        return diff
    out = np.zeros((c['F'], c['H'], c['W']), bool)
    out[:, ::2, ::2] = diff
    return out


def by_path(c, fmt, diff, class_px):
    """{(plan class, tail form): (mismatching samples, the first five as [frame, luma row, luma column])} of a mismatch mask."""
    d = luma_grid(c, diff)
    tail_px = pw.per_pixel(fc.tail_names(c, fmt), c['H'], c['W'])
    report = {}
    for k, cname in enumerate(pw.CLASS_NAMES):
        for tail in np.unique(tail_px):
            m = d & (class_px == k) & (tail_px == tail)
            if m.any():
                report[(cname, str(tail))] = (int(m.sum()), np.argwhere(m)[:5].tolist())
    return report


def census_of(c, cmap, fmt):
    """{(plan class, tail form): whole footprints of case c whose expected samples of `fmt` are not all border / fill}."""
    tails = fc.tail_names(c, fmt)
    live = c['live_footprints'][fmt]
    return {(cname, str(tail)): int((live & (cmap == k) & (tails == tail)).sum())
            for k, cname in enumerate(pw.CLASS_NAMES) for tail in np.unique(tails)}


@pytest.mark.parametrize('name', fc.NAMES)
def test_every_format_equals_its_model_on_every_path(dev, name):
    c, table, cmap, class_px = device_case(dev, name)
    got = run_formats(dev, c, table)
    print(name, 'footprints per class', {n: int((cmap == k).sum()) for k, n in enumerate(pw.CLASS_NAMES)})
    bad = {}
    for fmt in fc.FORMATS + ('nv12_y',):
        want = want_bits(c, fmt)
        assert got[fmt].shape == want.shape and got[fmt].dtype == want.dtype, fmt
        diff = got[fmt] != want
        if diff.any():
            # (nv12_y is the grey warp's launch, no member of the family: reported by class alone)
            bad[fmt] = by_path(c, fmt if fmt in fc.FORMATS else 'maps', diff, class_px)
    assert not bad, bad
    assert np.array_equal(raw(table.crop), c['crop'].view(np.uint32))   # the crop rows every launch folded are the oracle's


# Per format, the (plan class, tail form) combinations that must hold a live whole footprint somewhere in the table.  Every plan class, and
# for the four two-form tails both forms under every class, with one exception that is merely not required: a BORDER footprint is one the
# plan could NOT certify as interior (cell_table.hip: !(covered && inside)) -- its fast form needs a source within 1/16 pixel of the
# certificate's slack and no uncovered pixel, which no geometry here is built to hit.
def must_occur(fmt):
    tails = ('fast', 'clamped') if fmt in fc.TWO_FORM_TAILS else ('one',)
    return {(k, t) for k in pw.CLASS_NAMES for t in tails} - {('border', 'fast')}


# Candidate cells a list of each class holds (mf_common.h): HOT and BORDER sit in the unused second entry of a ONE-entry list, the pair's
# flag in the unused third entry of a list of exactly TWO cells, the multi flag on lists of two to four.  Counted from the valid bits alone,
# so a label that footprint_class_map takes from the wrong flag (hot and pair swapped, say) shows here.
ENTRIES = {'hot_fast64': (1, 1), 'hot_plain': (1, 1), 'pair': (2, 2), 'multi': (2, 4), 'border': (1, 1), 'overflow': (0, 0), 'other': (0, 8)}


def test_census(dev):
    total = {fmt: {} for fmt in fc.FORMATS}
    for name in fc.NAMES:
        c, table, cmap, _ = device_case(dev, name)
        entries = pw.entry_counts(pw.plan_and_regions(table.buf, table.n, table.W, table.H, table.R, table.C)[0]).reshape(cmap.shape)
        for k, cname in enumerate(pw.CLASS_NAMES):
            lo, hi = ENTRIES[cname]
            assert int(((cmap == k) & ((entries < lo) | (entries > hi))).sum()) == 0, (name, cname)
        per_case = {}
        for fmt in fc.FORMATS:
            for key, n in census_of(c, cmap, fmt).items():
                total[fmt][key] = total[fmt].get(key, 0) + n
                if fmt in ('plane_f32', 'nv12_uv') and n:
                    per_case[(fmt,) + key] = n
        print('census', name, {n: int((cmap == k).sum()) for k, n in enumerate(pw.CLASS_NAMES)}, per_case)
    for fmt in fc.FORMATS:
        print('census total', fmt, {'%s/%s' % key: n for key, n in sorted(total[fmt].items())})
    missing = {fmt: sorted(key for key in must_occur(fmt) if total[fmt].get(key, 0) == 0) for fmt in fc.FORMATS}
    assert not any(missing.values()), missing


def fixed_index(coord):
    """ix = rint(32 u) >> 5 of cv2.remap's fixed point, for coordinates inside the frame's neighbourhood."""
    return np.rint(np.asarray(coord, np.float32).astype(np.float64) * 32.0).astype(np.int64) >> 5


def test_combinations_the_code_rules_out(dev):
    shortcut_codes = [pw.CLASS_NAMES.index(k) for k in SHORTCUT]
    hot_clamped_luma = hot_fast_luma_clamped_chroma = 0
    for name in fc.NAMES:
        c, table, cmap, class_px = device_case(dev, name)
        W, H = c['W'], c['H']
        # 1. cell_table.hip gives HOT, PAIR, MULTI and BORDER to whole footprints only (`whole` is a premise of `interior`, of DEEP and of the
        #    border window): none on a footprint that overhangs the frame -- the shortcuts run with every lane active.
        certified = np.isin(cmap, [pw.CLASS_NAMES.index(k) for k in CERTIFIED])
        assert int((certified & ~c['whole']).sum()) == 0, name
        # 2. A hot or pair footprint's region is DEEP: covered (every pixel has an owner) and `inside` -- floor(umin - 1/16) >= 1 and
        #    floor(umax + 1/16) + 1 <= W - 2 over the corner values of every listed cell, the same in y --, so every pixel's taps are columns
        #    ix, ix + 1 with 1 <= ix <= W - 3 and rows 1 <= iy <= H - 3: no unowned pixel, no tap outside the plane, in no format.
        short_px = np.isin(class_px, shortcut_codes)
        ix, iy = fixed_index(c['mx']), fixed_index(c['my'])
        outside = (ix < 1) | (ix > W - 3) | (iy < 1) | (iy > H - 3)
        assert int((short_px & outside).sum()) == 0, name
        assert int((short_px & ~c['live']['maps']).sum()) == 0, name
        #    ... halved, a chroma sample's taps are columns 0 <= ix, ix + 1 <= W / 2 - 1 (rows alike): inside the chroma plane
        cix, ciy = fixed_index(c['cmx']), fixed_index(c['cmy'])
        c_outside = (cix < 0) | (cix + 1 > W // 2 - 1) | (ciy < 0) | (ciy + 1 > H // 2 - 1)
        assert int((short_px[:, ::2, ::2] & c_outside).sum()) == 0, name
        # 3. That certificate is ONE pixel weaker than the tails' deep-interior test on the low side (2 <= ix) and equal to it on the high
        #    side (ix <= W - 3).  So on the full-resolution planes a hot or pair footprint takes the clamped tail only through a source column
        #    or row 1: a clamped one whose sources all have ix >= 2 and iy >= 2 cannot exist ...
        short_fp = np.isin(cmap, shortcut_codes)
        low = fc.per_footprint_any((ix < 2) | (iy < 2))
        clamped_luma = ~c['tail_fast']['luma']
        assert int((short_fp & clamped_luma & ~low).sum()) == 0, name
        #    ... while through column or row 1 it can and does (asserted over the table below): hot x clamped is NOT ruled out on a
        #    full-resolution plane, whatever mf_common.h's "two pixels inside" suggests.
        hot_clamped_luma += int((short_fp & clamped_luma & c['live_footprints']['plane_f32']).sum())
        # 4. Chroma: a luma-deep hot footprint whose source lies 2 to 4 pixels from the left or top edge halves to chroma column or row 1,
        #    which is not deep on the chroma plane: fast on the luma-sized planes and clamped on both chroma planes.
        hot_fast_luma_clamped_chroma += int((short_fp & ~clamped_luma & ~c['tail_fast']['chroma'] & c['live_footprints']['nv12_uv']).sum())
    print('hot or pair footprints: clamped on the full-resolution planes', hot_clamped_luma,
          '-- fast there, clamped on the chroma planes', hot_fast_luma_clamped_chroma)
    assert hot_clamped_luma > 0 and hot_fast_luma_clamped_chroma > 0


def test_the_cheap_chain_refuses_at_run_time(dev):
    """HOT | FAST64 footprints on which cell_coords_fast must refuse, so that the hot shortcut's second chain, cell_coords<false>, produces
    what the equality test compares.  Shown from the case's construction, on the CPU: the mesh is sheared by 2^-18 per row, a shear's inverse
    is exact, so in every second row the source column u = x + 2^-18 (y + by) + bx lies, where 32 <= u < 64, exactly half way between two
    float32 numbers; the oracle's inverse homography of the footprint's owner (the cell the device's plan names) gives that value in
    float64 to the last bit, and the cheap chain's own value lies within its certified bound of it -- inside the guard's window
    (footprint_cases.cheap_chain_must_refuse).  The premise is the bound itself, which
    tests/test_gpu_parity.py measures with mf_selftest_fast64_margin."""
    c, table, cmap, _ = device_case(dev, fc.MIDPOINT)
    plan = pw.plan_and_regions(table.buf, table.n, table.W, table.H, table.R, table.C)[0]
    owner = (plan[:, 0] & 0xFFF).astype(np.int64).reshape(cmap.shape)
    fast64 = cmap == pw.CLASS_NAMES.index('hot_fast64')
    must = fc.cheap_chain_must_refuse(c['records'], np.where(fast64, owner, 0), c['H'], c['W']) & fast64
    print('hot_fast64 footprints', int(fast64.sum()), 'of which the cheap chain must refuse', int(must.sum()),
          'with the fast tail', int((must & c['tail_fast']['luma']).sum()), 'with the clamped tail', int((must & ~c['tail_fast']['luma']).sum()))
    assert int(must.sum()) > 0
    # the same footprints through every format: the equality of test_every_format_equals_its_model_on_every_path, restricted to them
    got = run_formats(dev, c, table)
    must_px = pw.per_pixel(must, c['H'], c['W'])
    for fmt in fc.FORMATS:
        diff = luma_grid(c, got[fmt] != want_bits(c, fmt))
        assert not (diff & must_px).any(), (fmt, int((diff & must_px).sum()), np.argwhere(diff & must_px)[:5].tolist())


# Unaligned stacks: the smallest step off the natural alignment each format allows, in bytes (the maps' `out` must stay 8-byte aligned)
OFFSET_BYTES = {'out_maps': 8, 'planes': 4, 'out_plane_f32': 4, 'n1': 1, 'out_plane_n1': 1, 'n2': 2, 'out_plane_n2': 2, 'n4': 4, 'out_plane_n4': 4,
                'n8': 8, 'out_plane_n8': 8, 'y16': 2, 'out_u16c1': 2, 'uv16': 2, 'out_p010_uv': 2, 'uv8': 2, 'out_nv12_uv': 2}
HOT_RICH = '256x144_2x2_translate_25'


def test_hot_footprints_from_and_into_unaligned_stacks(dev):
    """One case rich in hot footprints (asserted), every format from and into views that sit the smallest allowed step past a 16-byte
    boundary of a sentinel-filled buffer: the float32 plane's 16-byte store turns into the per-element loop, the 8-byte and 4-byte stores of
    the 16-bit and chroma planes become unaligned ones.  The same bits as the aligned call, the inputs unchanged, the guards intact."""
    c, table, cmap, _ = device_case(dev, HOT_RICH)
    hot = np.isin(cmap, [pw.CLASS_NAMES.index('hot_fast64'), pw.CLASS_NAMES.index('hot_plain')])
    assert hot.mean() > 0.5 and (cmap == pw.CLASS_NAMES.index('pair')).any(), 'the case is not rich in hot footprints any more'
    aligned = run_formats(dev, c, table)
    guards = []

    def guarded(key):
        def make(t):
            nbytes, lead = t.numel() * t.element_size(), 16 + OFFSET_BYTES[key]
            buf = torch.full((lead + nbytes + 32,), 0xA5, dtype=torch.uint8, device=dev)
            assert buf.data_ptr() % 16 == 0
            view = buf[lead:lead + nbytes].view(t.dtype).view(t.shape)
            if not key.startswith('out_'):
                buf[lead:lead + nbytes].copy_(t.contiguous().view(torch.uint8).view(-1))
            guards.append((key, buf, lead, nbytes, None if key.startswith('out_') else t))
            assert view.data_ptr() % 16 == OFFSET_BYTES[key] % 16 and view.is_contiguous()
            return view
        return make

    got = run_formats(dev, c, table, views={key: guarded(key) for key in OFFSET_BYTES})
    assert len(guards) == len(OFFSET_BYTES)
    for fmt in fc.FORMATS + ('nv12_y',):
        assert np.array_equal(got[fmt], aligned[fmt]), fmt
        assert np.array_equal(got[fmt], want_bits(c, fmt)), fmt
    for key, buf, lead, nbytes, source in guards:
        assert bool((buf[:lead] == 0xA5).all()) and bool((buf[lead + nbytes:] == 0xA5).all()), key
        if source is not None:
            assert torch.equal(buf[lead:lead + nbytes], source.contiguous().view(torch.uint8).view(-1)), key
