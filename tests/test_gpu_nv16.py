"""-m gpu: NV16 clips (4:2:2) -- `ops.warp_nv16`, mf_warp_bounds_nv16 through raw ctypes, `MeshFlowStabilizer.stabilized_nv16`.

Every equality is byte for byte.  Luma is compared with `ops.warp` on the luma planes (the grey warp, itself proven against the oracle) AND with
the model; its crop rows, clip rectangle and status with the grey call's.  Chroma is compared with tests/nv16_model.py on the reference's own
maps (the C oracle, on the CPU).  The cases (tests/nv16_cases.py: even and odd heights) are checked on the CPU to hold border, partly-outside
and deep-interior chroma samples before a kernel result is looked at."""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nv16_cases  # noqa: E402
import nv16_model  # noqa: E402
from nv16_cases import BORDER, case_for  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def dev64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def put(a, dev, offset=None):
    """numpy bytes -> device tensor of the same shape.  offset=None: an allocation of its own; else the bytes start `offset` bytes past a
    16-byte boundary of a buffer filled with the sentinel 0xA5, 16 bytes to spare behind them (tests/test_gpu_pixel_edges.py's method)."""
    raw = np.array(a, copy=True).reshape(-1)                           # (a writable copy: the cases' arrays are read-only)
    if offset is None:
        return torch.from_numpy(raw).to(dev).view(a.shape)
    buf = torch.full((raw.size + 32,), 0xA5, dtype=torch.uint8, device=dev)
    lead = (-buf.data_ptr()) % 16 + offset
    t = buf[lead:lead + raw.size]
    t.copy_(torch.from_numpy(raw).to(dev))
    assert t.data_ptr() % 16 == offset
    return t.view(a.shape)


def table_for(dev, c, bounds=None):
    from meshflow_amd import ops
    return ops.cell_table(dev64(c['disp'], dev), dev64(c['stab'], dev), c['W'], c['H'], c['R'], c['C'], bounds=bounds)


def differing(got, want):
    d = got != want
    return int(d.sum()), np.argwhere(d)[:5].tolist()


@pytest.mark.parametrize('name', nv16_cases.NAMES)
def test_warp_nv16_equals_the_grey_warp_and_the_model(dev, name):
    from meshflow_amd import ops
    c = case_for(name)                                                  # (the class check is in there, on the CPU)
    print(name, c['classes'])
    y, uv = put(c['y'], dev), put(c['uv'], dev)
    # the grey call on a table of its own: luma bytes, crop rows, rectangle, status
    grey_table = table_for(dev, c)
    grey = ops.warp(y, grey_table, (BORDER[0],))
    table = table_for(dev, c)
    out_y, out_uv = ops.warp_nv16(y, uv, table, BORDER)
    again_y, again_uv = ops.warp_nv16(y, uv, table, BORDER)              # a second launch: equal bytes, and the folds are idempotent
    torch.cuda.synchronize()
    table.check()
    assert out_y.dtype == torch.uint8 and out_uv.dtype == torch.uint8
    assert tuple(out_y.shape) == c['y'].shape and tuple(out_uv.shape) == c['uv'].shape
    assert torch.equal(out_y, grey), differing(out_y.cpu().numpy(), grey.cpu().numpy())
    assert torch.equal(table.crop, grey_table.crop) and torch.equal(table.clip_bounds, grey_table.clip_bounds)
    assert torch.equal(table.status, grey_table.status) and int(table.status.item()) == 0
    assert np.array_equal(table.crop.cpu().numpy(), c['crop'])
    assert np.array_equal(out_y.cpu().numpy(), c['want_y']), differing(out_y.cpu().numpy(), c['want_y'])
    got = out_uv.cpu().numpy()
    assert np.array_equal(got, c['want_uv']), differing(got, c['want_uv'])
    assert torch.equal(again_y, out_y) and torch.equal(again_uv, out_uv)
    assert np.array_equal(y.cpu().numpy(), c['y']) and np.array_equal(uv.cpu().numpy(), c['uv'])
    # the caller's rectangle
    bounds = torch.empty(4, dtype=torch.int32, device=dev)
    tb = table_for(dev, c, bounds=bounds)
    by, buv = ops.warp_nv16(y, uv, tb, BORDER, bounds=bounds)
    torch.cuda.synchronize()
    assert torch.equal(by, out_y) and torch.equal(buv, out_uv)
    assert torch.equal(tb.crop, grey_table.crop) and torch.equal(bounds, grey_table.clip_bounds)


@pytest.mark.parametrize('name', ['100x72_3x5_shift', '66x49_2x2_jitter', '128x96_32x32', '2x33_tiny'])
def test_model_maps_are_the_maps_kernel_s(dev, name):
    """`ops.warp_maps(table)[:, :, ::2]` with x halved is what the model samples chroma at, bit for bit -- and fed to the model it gives the
    model's chroma."""
    from meshflow_amd import ops
    c = case_for(name)
    maps = ops.warp_maps(table_for(dev, c))
    even = maps[:, :, ::2, :]
    hx, hy = (even[..., 0] * 0.5).cpu().numpy(), even[..., 1].contiguous().cpu().numpy()
    assert hx.dtype == np.float32 and hy.dtype == np.float32
    assert np.array_equal(hx.view(np.uint32), c['cmx'].view(np.uint32))
    assert np.array_equal(hy.view(np.uint32), c['cmy'].view(np.uint32))
    want = np.stack([nv16_model.remap_chroma(c['uv'][f], hx[f], hy[f], BORDER[1:]) for f in range(c['F'])])
    assert np.array_equal(want, c['want_uv'])


@pytest.mark.parametrize('name', ['66x49_2x2_shift', '66x50_2x2_jitter', '100x71_3x5_jitter', '4x3_tiny'])
def test_unaligned_stacks(dev, name):
    """uv 2, 6 and 14 bytes past a 16-byte boundary, y 1 and 3 bytes past one, inputs and outputs alike -- with W % 4 == 2 every other chroma
    row, and with an odd H every other frame, is only 2-byte aligned on top of that: the same bytes, and not a byte of the sentinel around an
    output changes."""
    from meshflow_amd import ops
    c = case_for(name)
    table = table_for(dev, c)
    y, uv = put(c['y'], dev), put(c['uv'], dev)
    for y_off, uv_off in ((1, 2), (3, 6), (1, 14), (0, 2), (3, 0)):
        yy, uu = put(c['y'], dev, y_off), put(c['uv'], dev, uv_off)
        got_y, got_uv = ops.warp_nv16(yy, uu, table, BORDER)                                   # offset inputs, aligned outputs
        oy, ouv = put(np.full_like(c['y'], 0xA5), dev, y_off), put(np.full_like(c['uv'], 0xA5), dev, uv_off)
        ops.warp_nv16(y, uv, table, BORDER, out=(oy, ouv))                                     # aligned inputs, offset outputs
        torch.cuda.synchronize()
        for g in (got_y, oy):
            assert np.array_equal(g.cpu().numpy(), c['want_y']), (y_off, uv_off)
        for g in (got_uv, ouv):
            assert np.array_equal(g.cpu().numpy(), c['want_uv']), (y_off, uv_off)
        for t in (oy, ouv):
            whole = t.untyped_storage()
            flat = torch.empty(0, dtype=torch.uint8, device=dev).set_(whole)
            lead = t.data_ptr() - flat.data_ptr()
            assert bool((flat[:lead] == 0xA5).all()) and bool((flat[lead + t.numel():] == 0xA5).all()), (y_off, uv_off)


def test_refused_call_leaves_out_untouched(dev):
    from meshflow_amd import ops
    c = case_for('66x49_2x2_jitter')
    table = table_for(dev, c)
    y, uv = put(c['y'], dev), put(c['uv'], dev)
    oy, ouv = torch.full_like(y, 0x5A), torch.full_like(uv, 0x5A)
    crop0 = table.crop.clone()
    with pytest.raises(ValueError, match='alias'):
        ops.warp_nv16(y, uv, table, BORDER, out=(oy, uv))              # out_uv is the input chroma: refused before the luma launch
    with pytest.raises(ValueError):
        ops.warp_nv16(y, uv, table, BORDER, out=(oy, ouv[:1]))
    with pytest.raises(ValueError):
        ops.warp_nv16(y, uv[:, :, :-1], table, BORDER, out=(oy, ouv))
    with pytest.raises(ValueError):
        ops.warp_nv16(y, uv[:, ::2].contiguous(), table, BORDER, out=(oy, ouv))         # an NV12-shaped chroma stack
    torch.cuda.synchronize()
    assert bool((oy == 0x5A).all()) and bool((ouv == 0x5A).all()) and torch.equal(table.crop, crop0)
    assert np.array_equal(uv.cpu().numpy(), c['uv'])
    got_y, got_uv = ops.warp_nv16(y, uv, table, BORDER, out=(oy, ouv))
    assert got_y.data_ptr() == oy.data_ptr() and got_uv.data_ptr() == ouv.data_ptr()
    assert np.array_equal(ouv.cpu().numpy(), c['want_uv']) and np.array_equal(oy.cpu().numpy(), c['want_y'])


def test_default_border_is_bt601_red(dev):
    from meshflow_amd import ops
    c = case_for('64x48_4x6_shift')
    table = table_for(dev, c)
    y, uv = put(c['y'], dev), put(c['uv'], dev)
    dy, duv = ops.warp_nv16(y, uv, table)
    ry, ruv = ops.warp_nv16(y, uv, table, (81, 90, 240))
    fy, fuv = ops.warp_nv16(y, uv, table, (80.6, 89.5, 300.0))         # clamp(round(v), 0, 255): 81, 90 (half to even), 255
    assert torch.equal(dy, ry) and torch.equal(duv, ruv)
    want = np.stack([nv16_model.remap_chroma(c['uv'][f], c['cmx'][f], c['cmy'][f], (90, 240)) for f in range(c['F'])])
    assert np.array_equal(duv.cpu().numpy(), want)
    want = np.stack([nv16_model.remap_chroma(c['uv'][f], c['cmx'][f], c['cmy'][f], (90, 255)) for f in range(c['F'])])
    assert np.array_equal(fuv.cpu().numpy(), want) and torch.equal(fy, ry)


def test_raw_ctypes_bounds_call(dev):
    from meshflow_amd import _lib, ops
    c = case_for('100x71_3x5_jitter')
    n, W, H, R, C = c['F'], c['W'], c['H'], c['R'], c['C']
    bounds = torch.empty(4, dtype=torch.int32, device=dev)
    table = table_for(dev, c, bounds=bounds)
    grey_bounds = torch.empty(4, dtype=torch.int32, device=dev)
    grey_table = table_for(dev, c, bounds=grey_bounds)
    y, uv = put(c['y'], dev), put(c['uv'], dev)
    grey = ops.warp(y, grey_table, (BORDER[0],), bounds=grey_bounds)
    oy, ouv = torch.empty_like(y), torch.empty_like(uv)
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib.mf_warp_bounds_nv16(vp(y.data_ptr()), vp(uv.data_ptr()), vp(oy.data_ptr()), vp(ouv.data_ptr()), vp(table.buf.data_ptr()), n, W, H,
                                      R, C, (ctypes.c_uint8 * 3)(*BORDER), vp(table.crop.data_ptr()), vp(bounds.data_ptr()), stream)
    assert rc == _lib.MF_OK, _lib.lib.mf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(oy, grey) and np.array_equal(ouv.cpu().numpy(), c['want_uv'])
    assert torch.equal(table.crop, grey_table.crop) and torch.equal(bounds, grey_bounds)
    assert tuple(bounds.tolist()) != (0, 0, W - 1, H - 1)


def test_stabilized_nv16(dev):
    from meshflow_amd import ops, synthetic
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    F, H, W, R, C = 8, 63, 98, 3, 4                                    # an odd H, W % 4 == 2
    disp, hom = synthetic.motion(F, R, C, seed=71, jitter_sigma=2.0)
    s = MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, temporal_smoothing_radius=4, optimization_num_iterations=15, device='cuda:0')
    rng = np.random.default_rng(8)
    y = put(rng.integers(0, 256, (F, H, W), dtype=np.uint8), dev)
    uv = put(rng.integers(0, 256, (F, H, W // 2, 2), dtype=np.uint8), dev)
    _, maps_bounds = s.stabilization_maps(dev64(disp, dev), hom, W, H)
    stab = s._get_stabilized_vertex_displacements(F, [np.zeros((H, W, 3), np.uint8)] * F, s.ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, disp, hom)
    table = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
    want_y, want_uv = ops.warp_nv16(y, uv, table, BORDER)
    got_y, got_uv, b = s.stabilized_nv16(y, uv, dev64(disp, dev), hom, BORDER)
    torch.cuda.synchronize()
    assert torch.equal(got_y, want_y) and torch.equal(got_uv, want_uv)
    assert b.dtype == torch.int32 and torch.equal(b, maps_bounds) and torch.equal(b, table.clip_bounds)
    assert tuple(b.tolist()) != (0, 0, W - 1, H - 1)
    # ... which is the model on the oracle's maps
    for f in (0, F - 1):
        mx, my, _, bad = __import__('cv16_model').warp_maps(W, H, R, C, disp[f], stab[f])
        assert bad == 0
        my_y, my_uv = nv16_model.warp_frame(y[f].cpu().numpy(), uv[f].cpu().numpy(), mx, my, BORDER)
        assert np.array_equal(got_y[f].cpu().numpy(), my_y) and np.array_equal(got_uv[f].cpu().numpy(), my_uv)
    # the default border, and out=
    oy, ouv = torch.empty_like(y), torch.empty_like(uv)
    r_y, r_uv, _ = s.stabilized_nv16(y, uv, dev64(disp, dev), hom, out=(oy, ouv))
    d_y, d_uv = ops.warp_nv16(y, uv, table, (81, 90, 240))
    assert r_y.data_ptr() == oy.data_ptr() and r_uv.data_ptr() == ouv.data_ptr() and torch.equal(oy, d_y) and torch.equal(ouv, d_uv)
    with pytest.raises(ValueError):
        s.stabilized_nv16(y[..., None], uv, dev64(disp, dev), hom)
    with pytest.raises(ValueError):
        s.stabilized_nv16(y, uv[:, :-1], dev64(disp, dev), hom)
    with pytest.raises(TypeError):
        s.stabilized_nv16(y, uv, dev64(disp, dev), hom, crop=True)      # no crop-resize of 4:2:2 clips
