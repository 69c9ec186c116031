"""-m gpu: the warp's float32 coordinate maps -- mf_warp_maps_f32 / mf_warp_maps_bounds_f32 through `ops.warp_maps`, raw ctypes and
`MeshFlowStabilizer.stabilization_maps`.

The contract is the reference's own arrays: maps[f, y, x] = (u, v) is bit for bit what the C oracle's mfo_warp_frame(..., map_x, map_y)
returns (frame_stabilized_x_y of mfs.py:1054-1061; (W + 1, H + 1) where no cell owns the pixel, mfs.py:983-984), on every path of the
kernel -- hot, pair, and the general path that serves multi and border footprints here --, and the crop values / clip rectangle a maps
launch folds are those of the pixel warps."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import plan_words  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def dev64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def motion(F, H, W, R, C, seed, jitter, kind='jitter'):
    from meshflow_amd import synthetic
    from oracle import meshflow_oracle as mo
    if kind == 'shift':                            # large global translation: wide border rings, many uncovered pixels
        disp, hom = synthetic.motion(F, R, C, seed=seed, translation_sigma=12.0, jitter_sigma=jitter)
    elif kind == 'stress':                         # a strong smooth field on top: far-from-affine cells, long candidate lists
        disp, hom = synthetic.motion(F, R, C, seed=seed, translation_sigma=20.0, field_sigma=8.0, jitter_sigma=jitter)
    else:
        disp, hom = synthetic.motion(F, R, C, seed=seed, jitter_sigma=jitter)
    stab = mo.stabilized_vertex_displacements(W, H, 0, disp, hom, 3, 10)
    return disp, hom, stab


def oracle_maps(disp, stab, H, W, R, C):
    """(F, H, W, 2) float32 maps, x first, from the C oracle; fails on a degenerate mesh."""
    from oracle import clib
    F = disp.shape[0]
    out = np.empty((F, H, W, 2), dtype=np.float32)
    blank = np.zeros((H, W, 3), dtype=np.uint8)
    for f in range(F):
        tab, bad = clib.cell_table(W, H, R, C, disp[f], stab[f])
        assert bad == 0
        _, _, mx, my = clib.warp_frame(blank, R, C, tab, want_maps=True)
        out[f, ..., 0], out[f, ..., 1] = mx, my
    return out


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def unowned_mask(maps, W, H):
    return (maps[..., 0] == np.float32(W + 1)) & (maps[..., 1] == np.float32(H + 1))


def table_for(dev, disp, stab, H, W, R, C, bounds=None):
    from meshflow_amd import ops
    return ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C, bounds=bounds)


def class_counts(table):
    """Footprints per plan class: hot / pair / multi / border as tests/plan_words.py decodes them."""
    plan, region = plan_words.plan_and_regions(table.buf, table.n, table.W, table.H, table.R, table.C)
    k = plan_words.classes(plan, region)
    return {name: int(k[name].sum()) for name in ('hot', 'pair', 'multi', 'border')}


# F, H, W, R, C, jitter, kind, seed.  Every case leaves pixels no cell owns (asserted): the stabilised mesh never covers the whole frame here.
CASES = [
    # the geometries of test_gpu_u8c4.py::test_coverage_mask (F = 3, seed = H + R)
    (3, 72, 100, 3, 5, 6.0, 'jitter', 75),
    (3, 144, 256, 8, 8, 2.0, 'shift', 152),
    (3, 97, 131, 4, 6, 4.0, 'shift', 101),        # odd W: every other row of the maps is only 8-byte aligned
    # tiny frames: below one footprint in one or both directions
    (2, 2, 2, 1, 1, 0.3, 'jitter', 4),
    (3, 2, 9, 1, 2, 0.3, 'jitter', 12),
    (3, 9, 2, 2, 1, 0.3, 'jitter', 6),
    (3, 7, 33, 1, 3, 1.0, 'shift', 36),           # H < 8, W = 32 + 1: a footprint with one column
    (2, 31, 30, 2, 2, 2.0, 'shift', 32),          # W % 4 == 2
    # W not a multiple of 4 or 32, H not of 8
    (3, 131, 257, 5, 7, 1.0, 'jitter', 260),
    (3, 75, 101, 6, 4, 2.0, 'shift', 104),
    (2, 60, 56, 2, 3, 1.0, 'jitter', 58),
    (2, 97, 132, 8, 32, 0.8, 'jitter', 134),      # R != C
    # stress meshes
    (5, 100, 100, 3, 3, 1.0, 'stress', 7),
    (4, 144, 256, 16, 16, 4.0, 'stress', 11),
    (3, 128, 128, 64, 64, 0.05, 'jitter', 13),    # the largest mesh: cells of two pixels
    # a 32 x 32 mesh
    (2, 96, 128, 32, 32, 0.5, 'jitter', 130),
    (2, 288, 512, 32, 32, 1.0, 'shift', 514),
    # 1080p at 16 x 16
    (2, 1080, 1920, 16, 16, 1.5, 'jitter', 1923),
    (2, 1080, 1920, 16, 16, 1.5, 'shift', 1922),
]


@pytest.mark.parametrize('F,H,W,R,C,jitter,kind,seed', CASES)
def test_bit_identical_to_the_oracle(dev, F, H, W, R, C, jitter, kind, seed):
    from meshflow_amd import ops
    disp, _, stab = motion(F, H, W, R, C, seed=seed, jitter=jitter, kind=kind)
    want = oracle_maps(disp, stab, H, W, R, C)
    table = table_for(dev, disp, stab, H, W, R, C)
    maps = ops.warp_maps(table)
    torch.cuda.synchronize()
    table.check()
    assert maps.shape == (F, H, W, 2) and maps.dtype == torch.float32 and maps.is_contiguous()
    got = maps.cpu().numpy()
    diff = bits(got) != bits(want)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5].tolist(), class_counts(table))
    n_unowned = int(unowned_mask(want, W, H).sum())
    print('classes', class_counts(table), 'unowned', n_unowned, 'of', F * H * W)
    assert n_unowned > 0, 'the case has no unowned pixel: the (W + 1, H + 1) template is not compared'
    # the crop rows a maps launch folds are those of the pixel warp on a fresh table
    t3 = table_for(dev, disp, stab, H, W, R, C)
    ops.warp(torch.zeros((F, H, W, 3), dtype=torch.uint8, device=dev), t3)
    torch.cuda.synchronize()
    assert torch.equal(table.crop, t3.crop) and torch.equal(table.clip_bounds, t3.clip_bounds)


def test_every_footprint_class_occurs(dev):
    """Over the cases above HOT, PAIR, MULTI and BORDER footprints all occur (and footprints that are none of them): the oracle comparison
    cannot pass on interior pixels alone."""
    total = {'hot': 0, 'pair': 0, 'multi': 0, 'border': 0, 'all': 0}
    for F, H, W, R, C, jitter, kind, seed in CASES:
        disp, _, stab = motion(F, H, W, R, C, seed=seed, jitter=jitter, kind=kind)
        table = table_for(dev, disp, stab, H, W, R, C)
        for k, v in class_counts(table).items():
            total[k] += v
        total['all'] += F * ((H + 7) // 8) * ((W + 31) // 32)
    print(total)
    for k in ('hot', 'pair', 'multi', 'border'):
        assert total[k] > 0, total
    assert total['all'] > total['hot'] + total['pair'] + total['multi'] + total['border'], total


def test_same_crop_as_the_pixel_warps(dev):
    from meshflow_amd import ops
    F, H, W, R, C = 5, 144, 256, 8, 8
    disp, _, stab = motion(F, H, W, R, C, seed=21, jitter=2.0, kind='shift')
    fr = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (F, H, W, 3), dtype=np.uint8)).to(dev)
    tm = table_for(dev, disp, stab, H, W, R, C)
    maps = ops.warp_maps(tm)
    tw = table_for(dev, disp, stab, H, W, R, C)
    out = ops.warp(fr, tw)
    ts = table_for(dev, disp, stab, H, W, R, C)
    ops.crop_scan(ts)
    torch.cuda.synchronize()
    defaults = torch.tensor([0, 0, W - 1, H - 1], dtype=torch.int32, device=dev)
    assert not torch.equal(tw.crop, defaults.expand(F, 4)), 'the geometry sets no crop value: nothing compared'
    for t in (tw, ts):
        assert torch.equal(tm.crop, t.crop) and torch.equal(tm.clip_bounds, t.clip_bounds)
    # maps, then the pixel warp, on ONE table: both unchanged; and the other way round
    crop0, bounds0 = tm.crop.clone(), tm.clip_bounds.clone()
    out2 = ops.warp(fr, tm)
    maps2 = ops.warp_maps(tw)
    torch.cuda.synchronize()
    assert torch.equal(out2, out) and torch.equal(maps2, maps)
    for t in (tm, tw):
        assert torch.equal(t.crop, crop0) and torch.equal(t.clip_bounds, bounds0)
    # the rectangle in the caller's tensor
    bounds = torch.empty(4, dtype=torch.int32, device=dev)
    tb = table_for(dev, disp, stab, H, W, R, C, bounds=bounds)
    maps3 = ops.warp_maps(tb, bounds=bounds)
    torch.cuda.synchronize()
    assert torch.equal(maps3, maps) and torch.equal(bounds, bounds0) and torch.equal(tb.crop, crop0)


@pytest.mark.parametrize('F,H,W,R,C,jitter,kind', [(2, 40, 52, 2, 3, 3.0, 'shift'), (2, 33, 47, 3, 2, 2.0, 'jitter'), (2, 64, 96, 4, 4, 2.0, 'jitter')])
def test_maps_reproduce_the_frames(dev, F, H, W, R, C, jitter, kind):
    """cv2.remap restated in NumPy on the device's maps gives the device's u8c3 warp, byte for byte."""
    from meshflow_amd import ops
    from oracle import meshflow_oracle as mo
    disp, _, stab = motion(F, H, W, R, C, seed=H + W, jitter=jitter, kind=kind)
    fr = np.random.default_rng(W).integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    border = (9, 99, 199)
    table = table_for(dev, disp, stab, H, W, R, C)
    maps = ops.warp_maps(table).cpu().numpy()
    out = ops.warp(torch.from_numpy(fr).to(dev), table, border).cpu().numpy()
    assert unowned_mask(maps, W, H).any()               # (two frames at least: a single frame's smoothed path is its own, i.e. zero motion)
    for f in range(F):
        want = mo.remap_bilinear_u8c3(fr[f], np.ascontiguousarray(maps[f, ..., 0]), np.ascontiguousarray(maps[f, ..., 1]), border)
        np.testing.assert_array_equal(out[f], want)


@pytest.mark.parametrize('H,W,R,C', [(64, 96, 4, 4), (72, 100, 3, 5), (144, 256, 16, 16), (9, 34, 1, 2)])
def test_zero_motion_and_integer_shifts(dev, H, W, R, C):
    """stab == unstab: every owned pixel maps to itself, exactly.  stab - unstab = (dx, dy) on every vertex: the mesh moves by (dx, dy),
    output pixel (x, y) samples (x - dx, y - dy), exactly, and what the moved mesh does not cover is unowned.  Both also bit for bit the
    oracle's maps."""
    from meshflow_amd import ops
    F = 3
    disp = np.random.default_rng(H).normal(0, 2.0, (F, R + 1, C + 1, 2))
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing='ij')
    maps = ops.warp_maps(table_for(dev, disp, disp.copy(), H, W, R, C)).cpu().numpy()
    # (zero motion: the mesh covers the frame exactly -- no pixel is unowned)
    assert not unowned_mask(maps, W, H).any()
    assert np.array_equal(maps[..., 0], np.broadcast_to(xs, (F, H, W))) and np.array_equal(maps[..., 1], np.broadcast_to(ys, (F, H, W)))
    for dx, dy in ((5, -3), (-4, 2)):
        stab = disp + np.array([dx, dy], dtype=np.float64)
        maps = ops.warp_maps(table_for(dev, disp, stab, H, W, R, C)).cpu().numpy()
        assert np.array_equal(bits(maps), bits(oracle_maps(disp, stab, H, W, R, C)))
        un = unowned_mask(maps, W, H)
        assert un.any() and not un.all()
        owned = ~un
        for got, want in ((maps[..., 0], np.broadcast_to(xs - dx, (F, H, W))), (maps[..., 1], np.broadcast_to(ys - dy, (F, H, W)))):
            # exact wherever the coordinate is not 0: the 4-point solve returns the translation to ~1e-13 (float64 rounding at coordinates of
            # a few hundred), far inside half a float32 ulp of any integer >= 1 -- but float32 resolves that residue next to 0, where the
            # reference's own arrays hold +-1e-15 instead of 0 (the oracle comparison above pins those bits)
            nonzero = owned & (want != 0)
            assert np.array_equal(got[nonzero], want[nonzero])
            assert np.all(np.abs(got[owned & (want == 0)]) <= 1e-12)
        # the strip the mesh moved away from is unowned, the interior of what it still covers is owned
        x_lo, x_hi = max(dx, 0), W + min(dx, 0)
        y_lo, y_hi = max(dy, 0), H + min(dy, 0)
        inner = np.zeros((H, W), dtype=bool)
        inner[y_lo + 1:y_hi - 1, x_lo + 1:x_hi - 1] = True
        assert owned[:, inner].all()
        outer = np.ones((H, W), dtype=bool)
        outer[max(y_lo - 1, 0):y_hi + 1, max(x_lo - 1, 0):x_hi + 1] = False
        assert un[:, outer].all() and outer.any()


SENTINEL = -12345.5


def guarded_out(dev, shape, lead):
    """A float32 buffer full of SENTINEL with a view of `shape` that starts `lead` floats in; (raw, view, lead, size)."""
    size = int(np.prod(shape))
    raw = torch.full((lead + size + 64,), SENTINEL, dtype=torch.float32, device=dev)
    return raw, raw[lead:lead + size].view(shape), lead, size


def guards_intact(raw, lead, size):
    return bool((raw[:lead] == SENTINEL).all()) and bool((raw[lead + size:] == SENTINEL).all())


@pytest.mark.parametrize('H,W', [(72, 100), (45, 33)])
def test_sub_ranges(dev, monkeypatch, H, W):
    from meshflow_amd import ops
    F, R, C = 7, 3, 5
    disp, _, stab = motion(F, H, W, R, C, seed=31, jitter=4.0, kind='shift')
    whole_table = table_for(dev, disp, stab, H, W, R, C)
    whole = ops.warp_maps(whole_table)
    torch.cuda.synchronize()
    want_crop = whole_table.crop.clone()
    defaults = torch.tensor([0, 0, W - 1, H - 1], dtype=torch.int32, device=dev)
    assert any(not torch.equal(want_crop[f], defaults) for f in range(F)), 'no frame sets a crop value: the row checks below would see defaults only'
    for first, count in ((0, 0), (F, 0), (3, 0), (F - 1, 1), (0, 1), (2, 3), (1, 6), (0, F)):
        t = table_for(dev, disp, stab, H, W, R, C)
        part = ops.warp_maps(t, first=first, count=count)
        torch.cuda.synchronize()
        assert part.shape == (count, H, W, 2)
        assert torch.equal(part, whole[first:first + count])
        # rows outside the range keep their defaults, rows inside are the whole clip's
        for f in range(F):
            assert torch.equal(t.crop[f], want_crop[f] if first <= f < first + count else defaults), (first, count, f)
        if count:
            assert t.clip_bounds.tolist() == [int(want_crop[first:first + count, 0].max()), int(want_crop[first:first + count, 1].max()),
                                              int(want_crop[first:first + count, 2].min()), int(want_crop[first:first + count, 3].min())]
        else:
            assert t.clip_bounds.tolist() == defaults.tolist()
    # count=None: up to the last frame
    assert torch.equal(ops.warp_maps(whole_table, first=4), whole[4:])
    # an `out` that is 8-byte but not 16-byte aligned, inside a guarded buffer; and a 16-byte aligned one
    for lead in (66, 64):
        raw, view, lead, size = guarded_out(dev, (3, H, W, 2), lead)
        assert view.data_ptr() % 16 == (8 if lead == 66 else 0)
        got = ops.warp_maps(whole_table, first=2, count=3, out=view)
        torch.cuda.synchronize()
        assert got.data_ptr() == view.data_ptr()
        assert torch.equal(view, whole[2:5]) and guards_intact(raw, lead, size)
    # a walk through a two-frame buffer
    buf = torch.empty((2, H, W, 2), dtype=torch.float32, device=dev)
    for first in range(0, F, 2):
        count = min(2, F - first)
        ops.warp_maps(whole_table, first=first, count=count, out=buf[:count])
        assert torch.equal(buf[:count], whole[first:first + count])
    # the launch split, forced
    for per in ('1', '2', '3'):
        monkeypatch.setenv('MF_WARP_FRAMES_PER_LAUNCH', per)
        t = table_for(dev, disp, stab, H, W, R, C)
        assert torch.equal(ops.warp_maps(t), whole)
        assert torch.equal(t.crop, want_crop)
        raw, view, lead, size = guarded_out(dev, (5, H, W, 2), 66)
        ops.warp_maps(t, first=1, count=5, out=view)
        torch.cuda.synchronize()
        assert torch.equal(view, whole[1:6]) and guards_intact(raw, lead, size)
    monkeypatch.delenv('MF_WARP_FRAMES_PER_LAUNCH')


def test_raw_ctypes_calls(dev):
    """The C ABI without `ops`: both entries on a table `ops` built, a sub-range into the middle of a guarded buffer."""
    from meshflow_amd import _lib, ops
    F, H, W, R, C = 4, 50, 70, 4, 4
    disp, _, stab = motion(F, H, W, R, C, seed=41, jitter=3.0, kind='shift')
    want = torch.from_numpy(oracle_maps(disp, stab, H, W, R, C)).to(dev)
    L = _lib.lib
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    table = table_for(dev, disp, stab, H, W, R, C)
    raw, view, lead, size = guarded_out(dev, (2, H, W, 2), 66)
    assert L.mf_warp_maps_f32(p(table.buf), p(view), F, W, H, R, C, 1, 2, p(table.crop), st) == _lib.MF_OK
    torch.cuda.synchronize()
    assert torch.equal(view.view(torch.int32), want[1:3].view(torch.int32)) and guards_intact(raw, lead, size)
    bounds = torch.empty(4, dtype=torch.int32, device=dev)
    t2 = table_for(dev, disp, stab, H, W, R, C, bounds=bounds)
    full = torch.empty((F, H, W, 2), dtype=torch.float32, device=dev)
    assert L.mf_warp_maps_bounds_f32(p(t2.buf), p(full), F, W, H, R, C, 0, F, p(t2.crop), p(bounds), None) == _lib.MF_OK
    torch.cuda.synchronize()
    assert torch.equal(full.view(torch.int32), want.view(torch.int32))
    t3 = table_for(dev, disp, stab, H, W, R, C)
    ops.warp(torch.zeros((F, H, W, 3), dtype=torch.uint8, device=dev), t3)
    torch.cuda.synchronize()
    assert torch.equal(t2.crop, t3.crop) and torch.equal(bounds, t3.clip_bounds)
    # refusals: nothing is launched, nothing is written
    raw, view, lead, size = guarded_out(dev, (F, H, W, 2), 64)
    E = _lib.MF_ERR_INVALID_ARG
    assert L.mf_warp_maps_f32(p(table.buf), p(view), F, W, H, R, C, 2, 3, p(table.crop), st) == E
    assert L.mf_warp_maps_f32(p(table.buf), p(view), F, W, H, R, C, -1, 2, p(table.crop), st) == E
    assert L.mf_warp_maps_f32(p(table.buf), p(view), F, 1, H, R, C, 0, F, p(table.crop), st) == E
    assert L.mf_warp_maps_f32(p(table.buf), p(view), F, W, H, 65, C, 0, F, p(table.crop), st) == E
    assert L.mf_warp_maps_f32(p(table.buf), ctypes.c_void_p(view.data_ptr() + 4), F, W, H, R, C, 0, 1, p(table.crop), st) == E
    assert L.mf_warp_maps_bounds_f32(p(table.buf), p(view), F, W, H, R, C, 0, F, p(table.crop), None, st) == E
    assert L.mf_warp_maps_f32(p(table.buf), p(view), F, W, H, R, C, F, 0, p(table.crop), st) == _lib.MF_OK
    torch.cuda.synchronize()
    assert bool((raw == SENTINEL).all())


def test_determinism_and_streams(dev):
    from meshflow_amd import ops
    F, H, W, R, C = 4, 144, 256, 16, 16
    disp, _, stab = motion(F, H, W, R, C, seed=51, jitter=2.0)
    table = table_for(dev, disp, stab, H, W, R, C)
    a = ops.warp_maps(table)
    b = ops.warp_maps(table)
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = ops.warp_maps(table, first=1, count=2)
    side.synchronize()
    assert torch.equal(c.view(torch.int32), a[1:3].view(torch.int32))
    torch.cuda.current_stream().wait_stream(side)


def test_refusals(dev):
    from meshflow_amd import ops
    F, H, W, R, C = 4, 40, 64, 2, 2
    disp, _, stab = motion(F, H, W, R, C, seed=61, jitter=1.0)
    table = table_for(dev, disp, stab, H, W, R, C)
    crop0 = table.crop.clone()
    for first, count in ((-1, 1), (F + 1, 0), (0, F + 1), (2, 3), (0, -1), (1.0, 1)):
        with pytest.raises(ValueError):
            ops.warp_maps(table, first=first, count=count)
    raw, view, lead, size = guarded_out(dev, (F, H, W, 2), 64)
    bad_outs = [
        (view.view(F, W, H, 2), 'shape'),                                        # a table of another (n, W, H)
        (view[:F - 1], 'shape'), (view.view(F, H, 2 * W), 'shape'),
        (view.view(torch.int32), 'dtype'), (view.double(), 'dtype'),
        (view.transpose(1, 2), 'contiguous'), (view[..., :1], 'contiguous'),
        (view.cpu(), 'CUDA/HIP'),
    ]
    for out, word in bad_outs:
        with pytest.raises(ValueError, match=word):
            ops.warp_maps(table, out=out)
    with pytest.raises(ValueError, match='contiguous'):
        ops.warp_maps(table, out=torch.empty((F, H, W, 4), dtype=torch.float32, device=dev)[..., ::2])
    with pytest.raises(ValueError, match='bounds'):
        ops.warp_maps(table, out=view, bounds=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.warp_maps(table, out=view, bounds=torch.zeros(4, dtype=torch.int64, device=dev))
    torch.cuda.synchronize()
    assert bool((raw == SENTINEL).all()) and torch.equal(table.crop, crop0)


def test_stabilization_maps(dev, monkeypatch):
    from meshflow_amd import ops, synthetic
    from meshflow_amd.stabilizer import DegenerateMeshError, MeshFlowStabilizer
    F, H, W, R, C = 12, 96, 128, 4, 4
    disp, hom = synthetic.motion(F, R, C, seed=71, jitter_sigma=1.0)
    s = MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, temporal_smoothing_radius=4, optimization_num_iterations=15, device='cuda:0')
    frames = [np.zeros((H, W, 3), dtype=np.uint8)] * F
    stab = s._get_stabilized_vertex_displacements(F, frames, s.ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, disp, hom)
    table = table_for(dev, disp, stab, H, W, R, C)
    want = ops.warp_maps(table)
    torch.cuda.synchronize()
    maps, bounds = s.stabilization_maps(dev64(disp, dev), hom, W, H)
    torch.cuda.synchronize()
    assert torch.equal(maps.view(torch.int32), want.view(torch.int32))
    assert bounds.dtype == torch.int32 and torch.equal(bounds, table.clip_bounds)
    # a sub-range into the caller's tensor: its own rectangle
    out = torch.empty((3, H, W, 2), dtype=torch.float32, device=dev)
    part, b2 = s.stabilization_maps(dev64(disp, dev), hom, W, H, first=5, count=3, out=out)
    torch.cuda.synchronize()
    assert part.data_ptr() == out.data_ptr() and torch.equal(out.view(torch.int32), want[5:8].view(torch.int32))
    crop = table.crop[5:8]
    assert b2.tolist() == [int(crop[:, 0].max()), int(crop[:, 1].max()), int(crop[:, 2].min()), int(crop[:, 3].min())]
    with pytest.raises(ValueError):
        s.stabilization_maps(dev64(disp, dev), hom, W, H, adaptive_weights_definition=17)
    with pytest.raises(ValueError):
        s.stabilization_maps(dev64(disp[:, :-1], dev), hom, W, H)
    # a degenerate mesh: the sweep's result replaced by displacements that put vertex (0, 1) of frame 1 onto vertex (0, 0)
    flat = np.zeros((F, R + 1, C + 1, 2))
    collapsed = flat.copy()
    collapsed[1, 0, 1] = [-W / C, 0.0]
    monkeypatch.setattr(s, '_stabilized_vertex_displacements_device', lambda *a, **k: dev64(collapsed, dev))
    raw, view, lead, size = guarded_out(dev, (F, H, W, 2), 64)
    with pytest.raises(DegenerateMeshError) as e:
        s.stabilization_maps(dev64(flat, dev), hom, W, H, out=view)
    assert e.value.cells >= 1 and e.value.clip_serial is None
    torch.cuda.synchronize()
    assert bool((raw == SENTINEL).all())


def test_float_layer_end_to_end(dev):
    """The recipes of INTEGRATION.md on the device: a float32 plane through grid_sample(maps_to_grid(maps)) under an integer shift is the
    shifted plane (zeros where no cell owns the pixel), and a label plane through the nearest-neighbour gather likewise.
    The float32 plane meets 1e-6 when grid and sampling are float64 (the recipe INTEGRATION.md gives for exact positions).  All in float32,
    1e-6 cannot be had at W = 100 whatever the maps hold: normalising a coordinate to [-1, 1] and back rounds values of up to 2 a few times
    and scales the error by W / 2, about W 2^-24 = 6e-6 pixels per rounding, each pixel of error moving that much weight to a neighbour of
    values in [0, 1).  That path is therefore held to the arithmetic's own bound, 8 W 2^-24, next to -- not instead of -- the 1e-6 check."""
    from meshflow_amd import ops
    F, H, W, R, C = 2, 72, 100, 3, 5
    dx, dy = 6, -4
    disp = np.random.default_rng(5).normal(0, 1.5, (F, R + 1, C + 1, 2))
    stab = disp + np.array([dx, dy], dtype=np.float64)
    maps = ops.warp_maps(table_for(dev, disp, stab, H, W, R, C))
    plane = torch.from_numpy(np.random.default_rng(6).random((F, 1, H, W)).astype(np.float32)).to(dev)
    owned = ~((maps[..., 0] == W + 1) & (maps[..., 1] == H + 1))
    want = torch.zeros_like(plane)
    want[:, :, :H + dy, dx:] = plane[:, :, -dy:, :W - dx]
    want = want * owned[:, None]
    for ac in (True, False):
        # the recipe as INTEGRATION.md gives it for exact positions: the grid and the sampling in float64
        got = torch.nn.functional.grid_sample(plane.double(), ops.maps_to_grid(maps.double(), align_corners=ac), mode='bilinear',
                                              padding_mode='zeros', align_corners=ac)
        err = float((got - want.double()).abs().max())
        print('float64 grid, align_corners', ac, 'max error', err)
        assert err <= 1e-6, (ac, err)
        # ... and all in float32: normalising and un-normalising a coordinate of up to W costs a few roundings of values of up to 2, scaled
        # back by W / 2 -- within 8 W 2^-24 pixels of the integer, i.e. that much weight on a neighbour, times values in [0, 1)
        got = torch.nn.functional.grid_sample(plane, ops.maps_to_grid(maps, align_corners=ac), mode='bilinear', padding_mode='zeros', align_corners=ac)
        err = float((got - want).abs().max())
        print('float32 grid, align_corners', ac, 'max error', err)
        assert err <= 8 * W * 2.0 ** -24, (ac, err)
    assert float(want.abs().sum()) > 0 and bool((~owned).any())
    # labels: nearest neighbour, -1 where the source lies outside the frame or no cell owns the pixel
    labels = torch.from_numpy(np.random.default_rng(7).integers(0, 1000, (F, H, W))).to(dev)
    idx = maps.round().long()
    ix, iy = idx[..., 0], idx[..., 1]
    inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    flat = (iy.clamp(0, H - 1) * W + ix.clamp(0, W - 1)).view(F, -1)
    moved = torch.where(inside, labels.view(F, -1).gather(1, flat).view(F, H, W), torch.full_like(labels, -1))
    want_l = torch.full_like(labels, -1)
    want_l[:, :H + dy, dx:] = labels[:, -dy:, :W - dx]
    want_l = torch.where(owned, want_l, torch.full_like(labels, -1))
    assert torch.equal(moved, want_l)
