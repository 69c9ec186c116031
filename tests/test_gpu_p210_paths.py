"""-m gpu: the P210 chroma warp (p210_chroma_footprint; warp_body.h, NOWIN) held to its footprint paths on tests/footprint_cases.py's
geometries, after tests/test_gpu_nv16_paths.py: their motion, maps and uint16 luma, and a seeded (F, H, W/2, 2) uint16 chroma stack of this
file's own.

Per case the table is built once, the device's plan decoded (tests/plan_words.footprint_class_map) and the chroma compared bit for bit with
tests/p210_model.py over the whole output; a mismatch is reported per plan class and tail form.  The tail form of a footprint is 'fast' where
every emitting sample -- the even columns of EVERY row -- is deep interior by the tail's own test at (u / 2, v) on the (W / 2, H) plane
(footprint_cases.deep_interior).  The census test then shows that the comparison is not vacuous: over the cases, every plan class x {fast,
clamped} except (border, fast) -- the set the existing tests demand of nv12_uv and nv16_uv -- holds a whole footprint whose expected samples
are not all border."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import footprint_cases as fc  # noqa: E402
import p210_model  # noqa: E402
import plan_words as pw  # noqa: E402

F32 = np.float32
BORDER = fc.BORDER_P010
_CASES = {}


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def p210_case(name):
    """footprint_cases' case plus what P210 adds, made on the CPU once: the chroma stack, the model's result, the tail form and the live
    footprints."""
    if name in _CASES:
        return _CASES[name]
    c = fc.case_for(name)
    F, H, W = c['F'], c['H'], c['W']
    uv = np.random.default_rng(2100 + fc.BY_NAME[name][7]).integers(0, 65536, (F, H, W // 2, 2), dtype=np.uint16)
    cmx, cmy = p210_model.chroma_maps(c['mx'], c['my'])
    assert np.array_equal(cmx, c['mx'][:, :, ::2] * F32(0.5)) and np.array_equal(cmy, c['my'][:, :, ::2])
    want = np.stack([p210_model.remap_chroma(uv[f], cmx[f], cmy[f], BORDER[1:]) for f in range(F)])
    deep = np.ones((F, H, W), bool)                                     # (W % 4 == 0: every lane holds two samples)
    deep[:, :, ::2] = fc.deep_interior(cmx, cmy, W // 2, H)
    fast = fc.per_footprint_all(deep)
    live_px = np.zeros((F, H, W), bool)
    live_px[:, :, ::2] = (want != np.asarray(BORDER[1:], np.uint16)).any(axis=-1)
    live = fc.per_footprint_any(live_px) & c['whole']
    e = dict(uv=uv, want=want, tails=np.where(fast, 'fast', 'clamped'), fast=fast, live=live)
    for a in e.values():
        a.setflags(write=False)
    _CASES[name] = e
    return e


_TABLES = {}


def device_case(dev, name):
    if name not in _TABLES:
        from meshflow_amd import ops
        c = fc.case_for(name)
        d64 = lambda a: torch.from_numpy(np.array(a, dtype=np.float64, copy=True)).to(dev)  # noqa: E731  (a copy: the case's arrays are read-only)
        table = ops.cell_table(d64(c['disp']), d64(c['stab']), c['W'], c['H'], c['R'], c['C'])
        torch.cuda.synchronize()
        table.check()
        cmap = pw.footprint_class_map(table)
        cmap.setflags(write=False)
        _TABLES[name] = (c, table, cmap)
    return _TABLES[name]


def by_path(c, e, diff, cmap):
    """{(plan class, tail form): (mismatching samples, the first five as [frame, luma row, luma column])} of a chroma mismatch mask."""
    d = np.zeros((c['F'], c['H'], c['W']), bool)
    d[:, :, ::2] = diff.any(axis=-1)
    class_px, tail_px = pw.per_pixel(cmap, c['H'], c['W']), pw.per_pixel(e['tails'], c['H'], c['W'])
    report = {}
    for k, cname in enumerate(pw.CLASS_NAMES):
        for tail in ('fast', 'clamped'):
            m = d & (class_px == k) & (tail_px == tail)
            if m.any():
                report[(cname, tail)] = (int(m.sum()), np.argwhere(m)[:5].tolist())
    return report


@pytest.mark.parametrize('name', fc.NAMES)
def test_p210_chroma_equals_its_model_on_every_path(dev, name):
    from meshflow_amd import ops
    c, table, cmap = device_case(dev, name)
    e = p210_case(name)
    y = torch.from_numpy(np.array(c['y16'], copy=True)).to(dev)
    uv = torch.from_numpy(np.array(e['uv'], copy=True)).to(dev)
    out_y, out_uv = ops.warp_p210(y, uv, table, BORDER)
    torch.cuda.synchronize()
    table.check()
    got = out_uv.cpu().numpy()
    assert got.shape == e['want'].shape and got.dtype == np.uint16
    diff = got != e['want']
    assert not diff.any(), by_path(c, e, diff, cmap)
    assert np.array_equal(out_y.cpu().numpy(), c['want']['u16c1'])      # the 16-bit luma launch in front of it
    assert np.array_equal(table.crop.cpu().numpy(), c['crop'])


def must_occur():
    return {(k, t) for k in pw.CLASS_NAMES for t in ('fast', 'clamped')} - {('border', 'fast')}


def test_census(dev):
    total = {}
    for name in fc.NAMES:
        c, table, cmap = device_case(dev, name)
        e = p210_case(name)
        assert e['fast'].any() and not e['fast'].all(), name              # both tail forms in every geometry
        per_case = {}
        for k, cname in enumerate(pw.CLASS_NAMES):
            for tail in ('fast', 'clamped'):
                n = int((e['live'] & (cmap == k) & (e['tails'] == tail)).sum())
                total[(cname, tail)] = total.get((cname, tail), 0) + n
                if n:
                    per_case['%s/%s' % (cname, tail)] = n
        print('census', name, 'fast footprints', int(e['fast'].sum()), per_case)
    print('census total p210_uv', {'%s/%s' % key: n for key, n in sorted(total.items())})
    missing = sorted(key for key in must_occur() if total.get(key, 0) == 0)
    assert not missing, missing
