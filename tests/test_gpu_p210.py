"""-m gpu: P210 clips (10-bit 4:2:2) -- `ops.warp_p210`, mf_warp_bounds_p210 through raw ctypes, `MeshFlowStabilizer.stabilized_p210`.

Every equality is bit for bit, no tolerance.  Both planes are compared with tests/p210_model.py on the reference's own maps (the C oracle, on
the CPU); luma's crop rows, clip rectangle and status with those of the P010-independent luma oracle: channel 0 of `ops.warp` on the clip
stack(Y, Y, Y) (the uint16 BGR warp) on the cases small enough for it, and the oracle's crop rows everywhere.  The cases (tests/p210_cases.py)
are checked on the CPU to hold border, partly-outside and deep-interior chroma taps before a kernel result is looked at.  (uint16 tensors are
compared as NumPy arrays or as int16 views.)"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p210_cases  # noqa: E402
import p210_model  # noqa: E402
from p210_cases import BORDER, case_for  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def dev64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def put(a, dev, offset=None, fill=0xA5):
    """uint16 samples -> device tensor of the same shape.  offset=None: an allocation of its own; else the samples start `offset` bytes (even)
    past a 16-byte boundary of a buffer filled with the sentinel byte, 16 bytes to spare behind them."""
    raw = np.array(a, dtype=np.uint16, copy=True).reshape(-1)          # (a writable copy: the cases' arrays are read-only)
    if offset is None:
        return torch.from_numpy(raw).to(dev).view(a.shape)
    assert offset % 2 == 0
    buf = torch.full((2 * raw.size + 32,), fill, dtype=torch.uint8, device=dev)
    lead = (-buf.data_ptr()) % 16 + offset
    t = buf[lead:lead + 2 * raw.size]
    t.copy_(torch.from_numpy(raw.view(np.uint8)).to(dev))
    assert t.data_ptr() % 16 == offset
    return t.view(torch.uint16).view(a.shape)


def canaries_intact(t, fill=0xA5):
    flat = torch.empty(0, dtype=torch.uint8, device=t.device).set_(t.untyped_storage())
    lead = t.data_ptr() - flat.data_ptr()
    return bool((flat[:lead] == fill).all()) and bool((flat[lead + 2 * t.numel():] == fill).all())


def get(t):
    return t.cpu().numpy()


def same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def table_for(dev, c, bounds=None):
    from meshflow_amd import ops
    return ops.cell_table(dev64(c['disp'], dev), dev64(c['stab'], dev), c['W'], c['H'], c['R'], c['C'], bounds=bounds)


def differing(got, want):
    d = got != want
    if d.ndim == 4:
        d = d.any(axis=-1)
    return int(d.sum()), np.argwhere(d)[:5].tolist()


@pytest.mark.parametrize('name', p210_cases.NAMES)
def test_warp_p210_equals_the_model_and_the_u16c3_warp(dev, name):
    from meshflow_amd import ops
    c = case_for(name)                                                  # (the class check is in there, on the CPU)
    print(name, c['classes'])
    y, uv = put(c['y'], dev), put(c['uv'], dev)
    # the luma oracle: the uint16 BGR call on stack(Y, Y, Y), on a fresh table from the same motion -- luma bits, crop rows, rectangle, status
    bgr_table = table_for(dev, c)
    bgr = ops.warp(put(np.stack([c['y']] * 3, axis=-1), dev), bgr_table, (BORDER[0],) * 3)
    table = table_for(dev, c)
    out_y, out_uv = ops.warp_p210(y, uv, table, BORDER)
    again_y, again_uv = ops.warp_p210(y, uv, table, BORDER)              # a second pair of launches: equal bits, and the folds are idempotent
    torch.cuda.synchronize()
    table.check()
    assert out_y.dtype == torch.uint16 and out_uv.dtype == torch.uint16
    assert tuple(out_y.shape) == c['y'].shape and tuple(out_uv.shape) == c['uv'].shape
    got_y, got_uv = get(out_y), get(out_uv)
    assert np.array_equal(got_y, c['want_y']), differing(got_y, c['want_y'])
    assert np.array_equal(got_uv, c['want_uv']), differing(got_uv, c['want_uv'])
    assert np.array_equal(got_y, get(bgr)[..., 0])
    # the chroma launch ran behind the luma launch and left the crop rows as that wrote them: they are the u16c3 call's, and the oracle's
    assert torch.equal(table.crop, bgr_table.crop) and torch.equal(table.clip_bounds, bgr_table.clip_bounds)
    assert torch.equal(table.status, bgr_table.status) and int(table.status.item()) == 0
    assert np.array_equal(get(table.crop), c['crop'])
    assert same(again_y, out_y) and same(again_uv, out_uv)
    assert np.array_equal(get(y), c['y']) and np.array_equal(get(uv), c['uv'])
    # the caller's rectangle, and an out= pair filled in place
    bounds = torch.empty(4, dtype=torch.int32, device=dev)
    tb = table_for(dev, c, bounds=bounds)
    oy, ouv = put(np.full_like(c['y'], 0x5A5A), dev), put(np.full_like(c['uv'], 0x5A5A), dev)
    ry, ruv = ops.warp_p210(y, uv, tb, BORDER, out=(oy, ouv), bounds=bounds)
    torch.cuda.synchronize()
    assert ry.data_ptr() == oy.data_ptr() and ruv.data_ptr() == ouv.data_ptr()
    assert same(oy, out_y) and same(ouv, out_uv)
    assert torch.equal(tb.crop, bgr_table.crop) and torch.equal(bounds, bgr_table.clip_bounds)


@pytest.mark.parametrize('name', ['100x72_3x5_shift', '66x49_2x2_jitter', '128x96_32x32', '2x33_tiny'])
def test_model_maps_are_the_maps_kernel_s(dev, name):
    """`ops.warp_maps(table)[:, :, ::2]` with x halved is what the model samples chroma at, bit for bit -- and fed to the model it gives the
    model's chroma."""
    from meshflow_amd import ops
    c = case_for(name)
    maps = ops.warp_maps(table_for(dev, c))
    even = maps[:, :, ::2, :]
    hx, hy = (even[..., 0] * 0.5).cpu().numpy(), even[..., 1].contiguous().cpu().numpy()
    assert np.array_equal(hx.view(np.uint32), c['cmx'].view(np.uint32))
    assert np.array_equal(hy.view(np.uint32), c['cmy'].view(np.uint32))
    want = np.stack([p210_model.remap_chroma(c['uv'][f], hx[f], hy[f], BORDER[1:]) for f in range(c['F'])])
    assert np.array_equal(want, c['want_uv'])


@pytest.mark.parametrize('name', ['66x49_2x2_shift', '66x50_2x2_jitter', '100x71_3x5_jitter', '4x3_tiny'])
def test_stacks_aligned_to_2_bytes_only(dev, name):
    """All four stacks 2, 6, 10 and 14 bytes past a 16-byte boundary, inputs and outputs alike -- with W % 4 == 2 every other chroma row, and
    with an odd H every other frame, is off by another 4 bytes --: the same bits, and not a byte of the sentinel around an output changes."""
    from meshflow_amd import ops
    c = case_for(name)
    table = table_for(dev, c)
    y, uv = put(c['y'], dev), put(c['uv'], dev)
    for y_off, uv_off in ((2, 6), (6, 2), (10, 14), (0, 2), (14, 0)):
        yy, uu = put(c['y'], dev, y_off), put(c['uv'], dev, uv_off)
        got_y, got_uv = ops.warp_p210(yy, uu, table, BORDER)                                   # offset inputs, aligned outputs
        oy, ouv = put(np.full_like(c['y'], 0xA5A5), dev, y_off), put(np.full_like(c['uv'], 0xA5A5), dev, uv_off)
        ops.warp_p210(y, uv, table, BORDER, out=(oy, ouv))                                     # aligned inputs, offset outputs
        torch.cuda.synchronize()
        for g in (got_y, oy):
            assert np.array_equal(get(g), c['want_y']), (y_off, uv_off)
        for g in (got_uv, ouv):
            assert np.array_equal(get(g), c['want_uv']), (y_off, uv_off)
        assert canaries_intact(oy) and canaries_intact(ouv), (y_off, uv_off)


def test_refused_call_leaves_out_untouched(dev):
    from meshflow_amd import ops
    c = case_for('66x49_2x2_jitter')
    table = table_for(dev, c)
    y, uv = put(c['y'], dev), put(c['uv'], dev)
    oy, ouv = put(np.full_like(c['y'], 0x5A5A), dev), put(np.full_like(c['uv'], 0x5A5A), dev)
    crop0 = table.crop.clone()
    with pytest.raises(ValueError, match='alias'):
        ops.warp_p210(y, uv, table, BORDER, out=(oy, uv))              # out_uv is the input chroma: refused before the luma launch
    with pytest.raises(ValueError):
        ops.warp_p210(y, uv, table, BORDER, out=(oy, ouv[:1]))
    with pytest.raises(ValueError):
        ops.warp_p210(y, uv[:, :, :-1], table, BORDER, out=(oy, ouv))
    with pytest.raises(ValueError):
        ops.warp_p210(y, uv[:, :24].contiguous(), table, BORDER, out=(oy, ouv))          # a P010-shaped chroma stack
    with pytest.raises(ValueError, match='a P010 frame has an even width and height'):
        ops.warp_p010(y, uv, table, BORDER)                            # ... and P010 keeps refusing the odd H
    torch.cuda.synchronize()
    assert (get(oy) == 0x5A5A).all() and (get(ouv) == 0x5A5A).all() and torch.equal(table.crop, crop0)
    got_y, got_uv = ops.warp_p210(y, uv, table, BORDER, out=(oy, ouv))
    assert got_y.data_ptr() == oy.data_ptr() and got_uv.data_ptr() == ouv.data_ptr()
    assert np.array_equal(get(ouv), c['want_uv']) and np.array_equal(get(oy), c['want_y'])


def test_default_border_and_values(dev):
    """The default border is P010's red; the top of the range saturates and does not wrap; a wholly-outside footprint is the border word."""
    from meshflow_amd import ops
    c = case_for('64x48_4x6_shift')
    table = table_for(dev, c)
    y, uv = put(c['y'], dev), put(c['uv'], dev)
    dy, duv = ops.warp_p210(y, uv, table)
    ry, ruv = ops.warp_p210(y, uv, table, ops.P010_BORDER_RED)
    assert same(dy, ry) and same(duv, ruv)
    want = np.stack([p210_model.remap_chroma(c['uv'][f], c['cmx'][f], c['cmy'][f], ops.P010_BORDER_RED[1:]) for f in range(c['F'])])
    assert np.array_equal(get(duv), want)
    top_uv = np.full(c['uv'].shape, 65535, np.uint16)
    _, ouv = ops.warp_p210(y, put(top_uv, dev), table, (0, 65535, 65535))
    assert (get(ouv) == 65535).all()
    _, ouv = ops.warp_p210(y, put(top_uv, dev), table, (0, 0, 7))
    want = np.stack([p210_model.remap_chroma(top_uv[f], c['cmx'][f], c['cmy'][f], (0, 7)) for f in range(c['F'])])
    assert np.array_equal(get(ouv), want)


def test_raw_ctypes_bounds_call(dev):
    from meshflow_amd import _lib
    c = case_for('100x71_3x5_jitter')
    n, W, H, R, C = c['F'], c['W'], c['H'], c['R'], c['C']
    bounds = torch.empty(4, dtype=torch.int32, device=dev)
    table = table_for(dev, c, bounds=bounds)
    y, uv = put(c['y'], dev), put(c['uv'], dev)
    oy, ouv = torch.empty_like(y), torch.empty_like(uv)
    vp = ctypes.c_void_p
    stream = vp(torch.cuda.current_stream().cuda_stream)
    rc = _lib.lib.mf_warp_bounds_p210(vp(y.data_ptr()), vp(uv.data_ptr()), vp(oy.data_ptr()), vp(ouv.data_ptr()), vp(table.buf.data_ptr()), n, W, H,
                                      R, C, (ctypes.c_uint16 * 3)(*BORDER), vp(table.crop.data_ptr()), vp(bounds.data_ptr()), stream)
    assert rc == _lib.MF_OK, _lib.lib.mf_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(get(oy), c['want_y']) and np.array_equal(get(ouv), c['want_uv'])
    assert np.array_equal(get(table.crop), c['crop'])
    crop = c['crop']
    assert tuple(bounds.tolist()) == (crop[:, 0].max(), crop[:, 1].max(), crop[:, 2].min(), crop[:, 3].min())
    assert tuple(bounds.tolist()) != (0, 0, W - 1, H - 1)


def test_stabilized_p210(dev):
    from meshflow_amd import ops, synthetic
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    F, H, W, R, C = 8, 63, 98, 3, 4                                    # an odd H, W % 4 == 2
    disp, hom = synthetic.motion(F, R, C, seed=71, jitter_sigma=2.0)
    s = MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, temporal_smoothing_radius=4, optimization_num_iterations=15, device='cuda:0')
    rng = np.random.default_rng(8)
    y = put(rng.integers(0, 65536, (F, H, W), dtype=np.uint16), dev)
    uv = put(rng.integers(0, 65536, (F, H, W // 2, 2), dtype=np.uint16), dev)
    _, maps_bounds = s.stabilization_maps(dev64(disp, dev), hom, W, H)
    stab = s._get_stabilized_vertex_displacements(F, [np.zeros((H, W, 3), np.uint8)] * F, s.ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, disp, hom)
    table = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
    want_y, want_uv = ops.warp_p210(y, uv, table, BORDER)
    got_y, got_uv, b = s.stabilized_p210(y, uv, dev64(disp, dev), hom, BORDER)
    torch.cuda.synchronize()
    assert same(got_y, want_y) and same(got_uv, want_uv)
    assert b.dtype == torch.int32 and torch.equal(b, maps_bounds) and torch.equal(b, table.clip_bounds)
    assert tuple(b.tolist()) != (0, 0, W - 1, H - 1)
    # ... which is the model on the oracle's maps
    for f in (0, F - 1):
        mx, my, _, bad = __import__('cv16_model').warp_maps(W, H, R, C, disp[f], stab[f])
        assert bad == 0
        my_y, my_uv = p210_model.warp_frame(get(y[f]), get(uv[f]), mx, my, BORDER)
        assert np.array_equal(get(got_y[f]), my_y) and np.array_equal(get(got_uv[f]), my_uv)
    # the cropped call is the composition, from the rectangle on the device
    c_y, c_uv, cb = s.stabilized_p210_cropped(y, uv, dev64(disp, dev), hom, BORDER, output_size=(80, 51))
    w_y, w_uv, _ = ops.crop_resize_p210(want_y, want_uv, b, size=(80, 51))
    assert torch.equal(cb, b) and same(c_y, w_y) and same(c_uv, w_uv) and tuple(c_uv.shape) == (F, 51, 40, 2)
    with pytest.raises(ValueError):
        s.stabilized_p210(y[..., None], uv, dev64(disp, dev), hom)
    with pytest.raises(ValueError):
        s.stabilized_p210(y, uv[:, :-1], dev64(disp, dev), hom)
    with pytest.raises(TypeError):
        s.stabilized_p210(y, uv, dev64(disp, dev), hom, crop=True)
