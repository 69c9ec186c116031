"""The two P010 calls in the header, the ctypes table and the built library, every refusal they make before anything is launched --
invalid-argument status with the call's name in mf_last_error() -- and every refusal of `ops.warp_p010` and `stabilized_p010`.  The C refusals
and what Python decides before it reaches a device need no GPU; the Python refusals that need device tensors are marked gpu."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {'mf_warp_p010': 13, 'mf_warp_bounds_p010': 14}
N, W, H = 3, 64, 48
Y_BYTES, UV_BYTES = N * W * H * 2, N * (W // 2) * (H // 2) * 4


def test_library_exports_the_p010_calls():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    for name, nargs in CALLS.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(_lib.lib, name), name
        assert re.search(r'\bint %s\(' % name, header), name
    block = header[header.index('P010 clips'):header.index('int mf_warp_p010(')]
    assert '(20736, 23040, 61440)' in block and 'even luma sample' in block and 'nothing is masked' in block and 'P016' in block
    assert _lib.lib.mf_abi_version() == 1


def test_exported_symbols_are_the_header_s_and_no_public_u16c1():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    declared = set(re.findall(r'^(?:int|size_t|const char\*)\s+(mf_\w+)\(', header, re.M))
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if len(l.split()) == 3 and l.split()[1] == 'T' and l.split()[-1].startswith('mf_')}
    assert set(CALLS) <= declared
    assert declared == exported == set(_lib.SIGNATURES)
    assert not [n for n in declared if 'u16c1' in n]


def test_default_border_value():
    from meshflow_amd import ops
    assert ops.P010_BORDER_RED == (20736, 23040, 61440) == tuple(v << 8 for v in ops.NV12_BORDER_RED)
    assert list(ops._p010_border((80.6, 70000, -3))) == [81, 65535, 0]              # clamp(round(v), 0, 65535)
    assert list(ops._p010_border((0.5, 1.5, 65534.5))) == [0, 2, 65534]             # half to even


@pytest.fixture(scope='module')
def env():
    from meshflow_amd import _lib
    buf = (ctypes.c_uint8 * (2 * (Y_BYTES + UV_BYTES) + 64))()
    base = (ctypes.addressof(buf) + 15) & ~15
    return _lib, buf, base


def refused(_lib, name, *args):
    rc = getattr(_lib.lib, name)(*args)
    err = _lib.lib.mf_last_error()
    assert rc == _lib.MF_ERR_INVALID_ARG, (name, args, rc, err)
    assert name.encode() in err, (name, err)
    return err


def test_c_refusals(env):
    """Host addresses throughout, and no GPU needed: a call that got as far as a launch would not return MF_ERR_INVALID_ARG."""
    _lib, buf, base = env
    vp = ctypes.c_void_p
    at = dict(y=base, uv=base + Y_BYTES, out_y=base + Y_BYTES + UV_BYTES, out_uv=base + 2 * Y_BYTES + UV_BYTES)
    border = (ctypes.c_uint16 * 3)(20736, 23040, 61440)
    good = dict(n=N, W=W, H=H, R=4, C=4, table=base, crop=base, bounds=base, border=border, **at)

    def plain(**kw):
        a = dict(good, **kw)
        return ('mf_warp_p010', vp(a['y']), vp(a['uv']), vp(a['out_y']), vp(a['out_uv']), vp(a['table']), a['n'], a['W'], a['H'], a['R'], a['C'],
                a['border'], vp(a['crop']), None)

    def with_bounds(**kw):
        a = dict(good, **kw)
        return ('mf_warp_bounds_p010', vp(a['y']), vp(a['uv']), vp(a['out_y']), vp(a['out_uv']), vp(a['table']), a['n'], a['W'], a['H'], a['R'],
                a['C'], a['border'], vp(a['crop']), vp(a['bounds']), None)

    for call in (plain, with_bounds):
        for key in ('y', 'uv', 'out_y', 'out_uv', 'table', 'border', 'crop'):
            assert b'null' in refused(_lib, *call(**{key: None}))
        for n in (0, -2):
            refused(_lib, *call(n=n))
        # aliasing: equal pointers, input against input, output against output, and stacks that merely overlap
        for kw in (dict(out_y=at['y']), dict(out_uv=at['uv']), dict(uv=at['y']), dict(out_uv=at['out_y']), dict(out_y=at['uv']), dict(out_uv=at['y']),
                   dict(out_y=at['y'] + 100), dict(out_uv=at['y'] + Y_BYTES - 2), dict(out_y=at['uv'] - Y_BYTES + 2),
                   dict(out_uv=at['out_y'] - 2), dict(uv=at['out_uv'] + UV_BYTES - 2)):
            assert b'alias' in refused(_lib, *call(**kw)), kw
        for kw in (dict(W=63), dict(H=47), dict(W=65, H=49), dict(W=3), dict(H=32767)):
            assert b'even' in refused(_lib, *call(**kw)), kw
        for kw in (dict(W=0), dict(H=0), dict(W=1), dict(H=1), dict(W=-64), dict(W=32768), dict(H=32768), dict(W=32769), dict(H=40000)):
            assert b'32,767' in refused(_lib, *call(**kw)), kw
        for kw in (dict(R=0), dict(C=0), dict(R=65), dict(C=65), dict(R=-1), dict(C=-3)):
            assert b'mesh' in refused(_lib, *call(**kw)), kw
        for kw in (dict(y=at['y'] + 1), dict(uv=at['uv'] + 1), dict(out_y=at['out_y'] + 1), dict(out_uv=at['out_uv'] + 1),
                   dict(uv=at['uv'] + 1, out_uv=at['out_uv'] + 3)):
            assert b'2-byte aligned' in refused(_lib, *call(**kw)), kw
    assert b'null' in refused(_lib, *with_bounds(bounds=None))
    assert bytes(buf) == bytes(len(buf))                                # nothing was written anywhere


def test_python_refusals_before_the_library():
    """What `ops.warp_p010` and `stabilized_p010` decide without a device."""
    torch = pytest.importorskip('torch')
    import types
    from meshflow_amd import ops
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    table = types.SimpleNamespace(n=2, W=8, H=4, R=1, C=1)
    y, uv = torch.zeros((2, 4, 8), dtype=torch.uint16), torch.zeros((2, 2, 4, 2), dtype=torch.uint16)
    with pytest.raises(ValueError, match='y must be a CUDA/HIP'):
        ops.warp_p010(y, uv, table)
    with pytest.raises(ValueError, match='y must be a CUDA/HIP'):
        ops.warp_p010(y.numpy(), uv, table)
    # the frame formats still refuse grey uint16 tensors: P010 luma is no frame stack
    with pytest.raises(ValueError, match='single-channel frames must be uint8'):
        ops.pixel_format(torch.uint16, (2, 4, 8))
    s = MeshFlowStabilizer(mesh_row_count=2, mesh_col_count=2, temporal_smoothing_radius=2, optimization_num_iterations=2)
    for kw in (dict(crop=True), dict(output_size=(8, 4)), dict(crop=True, output_size=(8, 4))):
        with pytest.raises(ValueError, match='crop-resize of 16-bit 4:2:0 clips is not built yet'):
            s.stabilized_p010(y, uv, None, None, **kw)                  # refused before anything else is looked at


@pytest.mark.gpu
def test_python_refusals_on_the_device():
    torch = pytest.importorskip('torch')
    import numpy as np
    from meshflow_amd import ops
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    dev = torch.device('cuda:0')
    n, H, W, R, C = 2, 16, 24, 2, 2
    flat = torch.zeros((n, R + 1, C + 1, 2), dtype=torch.float64, device=dev)
    table = ops.cell_table(flat, flat, W, H, R, C)
    crop0 = table.crop.clone()

    def u16(shape, value=0):
        return torch.from_numpy(np.full(shape, value, np.uint16)).to(dev)

    def b8(t):
        return t.view(torch.uint8)

    y, uv = u16((n, H, W), 5), u16((n, H // 2, W // 2, 2), 6)
    oy, ouv = u16((n, H, W), 0xA5A5), u16((n, H // 2, W // 2, 2), 0xA5A5)

    def no(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            ops.warp_p010(*args, **kw)

    no('dtype', b8(y)[..., ::2].contiguous(), uv, table)                # uint8 planes: an NV12 clip
    no('dtype', y.view(torch.int16), uv, table)
    no('dtype', y, uv.view(torch.int16), table)
    no('CUDA/HIP', y, uv.cpu(), table)
    no('CUDA/HIP', y.cpu(), uv, table)
    no('contiguous', u16((n, H, 2 * W))[..., ::2], uv, table)           # a pitched surface
    no('contiguous', y, u16((n, H // 2, W // 2, 4))[..., ::2], table)
    no('shape', y[..., None], uv, table)                                # (n, H, W, 1)
    no('contiguous', y, uv[..., 0], table)                              # a planar U as a strided view
    no('shape', y, u16((n, H // 2, W // 2)), table)                     # ... and as a plane of its own
    no('shape', y, uv.view(n, H // 2, W, 1), table)
    no('shape', y, u16((n, H, W, 2)), table)                            # 4:4:4
    no('shape', y, uv[:1], table)
    no('shape', u16((n, H * 3 // 2, W)), uv, table)                     # one tensor that holds both planes
    no('even', u16((n, H, W + 1)), uv, table)
    no('even', u16((n, H - 1, W)), uv, table)
    no('cell table', y[:1], uv[:1], table)                              # n != table.n
    no('cell table', u16((n, W, H)), u16((n, W // 2, H // 2, 2)), table)
    no('border_yuv', y, uv, table, border_yuv=(1, 2))
    for bad in ((oy,), (oy, ouv, ouv), oy, (oy, ouv[..., 0]), (oy[:1], ouv), (oy, ouv.view(torch.int16)), (oy.cpu(), ouv), (ouv, oy),
                (b8(oy)[..., ::2].contiguous(), ouv), (np.zeros((n, H, W), np.uint16), ouv)):
        with pytest.raises(ValueError):
            ops.warp_p010(y, uv, table, out=bad)
    with pytest.raises(ValueError):
        ops.warp_p010(y, uv, table, bounds=torch.zeros(3, dtype=torch.int32, device=dev))
    # what the library refuses comes back as ValueError too: planes that alias
    with pytest.raises(ValueError, match='alias'):
        ops.warp_p010(y, uv, table, out=(y, ouv))
    with pytest.raises(ValueError, match='alias'):
        ops.warp_p010(y, uv, table, out=(oy, uv))
    torch.cuda.synchronize()
    assert bool((b8(oy) == 0xA5).all()) and bool((b8(ouv) == 0xA5).all())
    assert np.array_equal(y.cpu().numpy(), np.full((n, H, W), 5, np.uint16)) and torch.equal(table.crop, crop0)
    # the frame operators still refuse (n, H, W) uint16 tensors
    with pytest.raises(ValueError):
        ops.warp(y, table)
