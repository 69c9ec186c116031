"""The four 4:2:2 calls -- mf_warp_nv16, mf_warp_bounds_nv16, mf_unpack_422_u8, mf_pack_422_u8 -- in the header, the ctypes table and the
built library, every refusal they make before anything is launched -- invalid-argument status with the call's name in mf_last_error() --
and every refusal of `ops.warp_nv16`, `ops.unpack_422`, `ops.pack_422` and `ops.warp_packed_422`.  The C refusals and what Python decides
before it reaches a device need no GPU; the Python refusals that need device tensors are marked gpu."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {'mf_warp_nv16': 13, 'mf_warp_bounds_nv16': 14, 'mf_unpack_422_u8': 8, 'mf_pack_422_u8': 8}
N, W, H = 3, 64, 47                       # an odd H: 4:2:2 has no rule about it
Y_BYTES = UV_BYTES = N * W * H
PACKED_BYTES = 2 * Y_BYTES


def test_library_exports_the_422_calls():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    for name, nargs in CALLS.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(_lib.lib, name), name
        assert re.search(r'\bint %s\(' % name, header), name
    block = header[header.index('NV16 clips'):header.index('int mf_warp_nv16(')]
    assert 'mfs.py:1063-1069' in block and '(81, 90, 240)' in block and 'even luma sample of the same row' in block
    assert 'either parity' in block and 'Not provided' in block
    block = header[header.index('int mf_warp_bounds_nv16('):header.index('int mf_unpack_422_u8(')]
    assert 'Y0 U Y1 V' in block and 'U Y0 V Y1' in block and '4-byte aligned' in block
    assert _lib.lib.mf_abi_version() == 1


def test_exported_symbols_are_the_header_s():
    """`nm -D` of the library and the header declare the same mf_* functions, and the ctypes table lists them all."""
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    declared = set(re.findall(r'^(?:int|size_t|const char\*)\s+(mf_\w+)\(', header, re.M))
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if len(l.split()) == 3 and l.split()[1] == 'T' and l.split()[-1].startswith('mf_')}
    assert set(CALLS) <= declared
    assert declared == exported
    assert declared == set(_lib.SIGNATURES)


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


def test_c_refusals_of_the_warp(env):
    """Host addresses throughout, and no GPU needed: a call that got as far as a launch would not return MF_ERR_INVALID_ARG."""
    _lib, buf, base = env
    vp = ctypes.c_void_p
    at = dict(y=base, uv=base + Y_BYTES, out_y=base + Y_BYTES + UV_BYTES, out_uv=base + 2 * Y_BYTES + UV_BYTES)
    border = (ctypes.c_uint8 * 3)(81, 90, 240)
    good = dict(n=N, W=W, H=H, R=4, C=4, table=base, crop=base, bounds=base, border=border, **at)

    def plain(**kw):
        a = dict(good, **kw)
        return ('mf_warp_nv16', vp(a['y']), vp(a['uv']), vp(a['out_y']), vp(a['out_uv']), vp(a['table']), a['n'], a['W'], a['H'], a['R'], a['C'],
                a['border'], vp(a['crop']), None)

    def with_bounds(**kw):
        a = dict(good, **kw)
        return ('mf_warp_bounds_nv16', vp(a['y']), vp(a['uv']), vp(a['out_y']), vp(a['out_uv']), vp(a['table']), a['n'], a['W'], a['H'], a['R'],
                a['C'], a['border'], vp(a['crop']), vp(a['bounds']), None)

    for call in (plain, with_bounds):
        for key in ('y', 'uv', 'out_y', 'out_uv', 'table', 'border', 'crop'):
            assert b'null' in refused(_lib, *call(**{key: None}))
        for n in (0, -2):
            refused(_lib, *call(n=n))
        # aliasing: equal pointers, input against input, output against output, and stacks that merely overlap -- the chroma stacks are n W H
        # bytes, twice an NV12 clip's: the last two overlap only in a chroma stack's second half
        for kw in (dict(out_y=at['y']), dict(out_uv=at['uv']), dict(uv=at['y']), dict(out_uv=at['out_y']), dict(out_y=at['uv']), dict(out_uv=at['y']),
                   dict(out_y=at['y'] + 100), dict(out_uv=at['y'] + Y_BYTES - 2), dict(out_y=at['uv'] - Y_BYTES + 1),
                   dict(out_uv=at['out_y'] - 2), dict(uv=at['out_uv'] + UV_BYTES - 2), dict(out_y=at['uv'] + UV_BYTES - 1),
                   dict(y=at['uv'] + UV_BYTES // 2 + 2, out_y=at['out_uv'] + UV_BYTES)):
            assert b'alias' in refused(_lib, *call(**kw)), kw
        for kw in (dict(W=63), dict(W=65, H=49), dict(W=3), dict(W=32767)):
            assert b'even' in refused(_lib, *call(**kw)), kw
        for kw in (dict(W=0), dict(H=0), dict(W=1), dict(H=1), dict(W=-64), dict(W=32768), dict(H=32768), dict(W=32769), dict(H=40000)):
            assert b'32,767' in refused(_lib, *call(**kw)), kw
        for kw in (dict(R=0), dict(C=0), dict(R=65), dict(C=65), dict(R=-1), dict(C=-3)):
            assert b'mesh' in refused(_lib, *call(**kw)), kw
        for kw in (dict(uv=at['uv'] + 1), dict(out_uv=at['out_uv'] + 1), dict(uv=at['uv'] + 1, out_uv=at['out_uv'] + 3)):
            assert b'2-byte aligned' in refused(_lib, *call(**kw)), kw
    assert b'null' in refused(_lib, *with_bounds(bounds=None))
    assert bytes(buf) == bytes(len(buf))                                # nothing was written anywhere


def test_c_refusals_of_pack_and_unpack(env):
    _lib, buf, base = env
    vp = ctypes.c_void_p
    at = dict(packed=base, y=base + PACKED_BYTES, uv=base + PACKED_BYTES + Y_BYTES)
    good = dict(n=N, W=W, H=H, order=0, **at)

    def unpack(**kw):
        a = dict(good, **kw)
        return ('mf_unpack_422_u8', vp(a['packed']), vp(a['y']), vp(a['uv']), a['n'], a['W'], a['H'], a['order'], None)

    def pack(**kw):
        a = dict(good, **kw)
        return ('mf_pack_422_u8', vp(a['y']), vp(a['uv']), vp(a['packed']), a['n'], a['W'], a['H'], a['order'], None)

    for call in (unpack, pack):
        for key in ('packed', 'y', 'uv'):
            assert b'null' in refused(_lib, *call(**{key: None}))
        for n in (0, -1):
            assert b'n must be' in refused(_lib, *call(n=n))
        for w in (63, 1, 0, -2, 32767, 32768, 40000):
            assert b'W must be even' in refused(_lib, *call(W=w)), w
        for h in (0, -1, 32768):
            assert b'H must be' in refused(_lib, *call(H=h)), h
        for order in (2, -1, 422):
            assert b'order' in refused(_lib, *call(order=order)), order
        for off in (1, 2, 3):
            assert b'4-byte aligned' in refused(_lib, *call(packed=at['packed'] + off)), off
        for kw in (dict(y=at['y'] + 1), dict(uv=at['uv'] + 1), dict(y=at['y'] + 3, uv=at['uv'] + 1)):
            assert b'2-byte aligned' in refused(_lib, *call(**kw)), kw
        for kw in (dict(y=at['packed']), dict(uv=at['packed']), dict(uv=at['y']), dict(y=at['packed'] + PACKED_BYTES - 2),
                   dict(uv=at['y'] + Y_BYTES - 2), dict(uv=at['y'] - UV_BYTES + 2), dict(packed=at['uv'] + UV_BYTES - 4),
                   dict(y=at['packed'] + 16, uv=at['uv'] + 64)):
            assert b'overlap' in refused(_lib, *call(**kw)), kw
    assert bytes(buf) == bytes(len(buf))                                # nothing was written anywhere


def test_python_refusals_before_the_library():
    """What the `ops` calls decide without a device: host tensors are refused first of all, whatever else is wrong with the call."""
    torch = pytest.importorskip('torch')
    import types
    from meshflow_amd import ops
    table = types.SimpleNamespace(n=2, W=8, H=3, R=1, C=1)
    y, uv = torch.zeros((2, 3, 8), dtype=torch.uint8), torch.zeros((2, 3, 4, 2), dtype=torch.uint8)
    packed = torch.zeros((2, 3, 8, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match='y must be a CUDA/HIP'):
        ops.warp_nv16(y, uv, table)
    with pytest.raises(ValueError, match='y must be a CUDA/HIP'):
        ops.warp_nv16(y.numpy(), uv, table)
    with pytest.raises(ValueError, match='y must be a CUDA/HIP'):
        ops.pack_422(y, uv)
    with pytest.raises(ValueError, match='packed must be a CUDA/HIP'):
        ops.unpack_422(packed)
    with pytest.raises(ValueError, match='packed must be a CUDA/HIP'):
        ops.warp_packed_422(packed, table, order='nv16')
    assert ops.ORDERS_422 == {'yuyv': 0, 'uyvy': 1}
    with pytest.raises(ValueError):
        ops.pixel_format(torch.uint8, (2, 4, 8, 2))                     # a packed clip is no frame stack


@pytest.mark.gpu
def test_python_refusals_on_the_device():
    torch = pytest.importorskip('torch')
    import numpy as np
    from meshflow_amd import ops
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    dev = torch.device('cuda:0')
    n, H, W, R, C = 2, 15, 24, 2, 2
    flat = torch.zeros((n, R + 1, C + 1, 2), dtype=torch.float64, device=dev)
    table = ops.cell_table(flat, flat, W, H, R, C)
    crop0 = table.crop.clone()
    y = torch.full((n, H, W), 5, dtype=torch.uint8, device=dev)
    uv = torch.full((n, H, W // 2, 2), 6, dtype=torch.uint8, device=dev)
    packed = torch.full((n, H, W, 2), 7, dtype=torch.uint8, device=dev)
    oy, ouv, op = torch.full_like(y, 0xA5), torch.full_like(uv, 0xA5), torch.full_like(packed, 0xA5)

    def no(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            ops.warp_nv16(*args, **kw)

    no('dtype', y.to(torch.int8), uv, table)
    no('dtype', y, uv.to(torch.int16), table)
    no('CUDA/HIP', y, uv.cpu(), table)
    no('CUDA/HIP', y.cpu(), uv, table)
    no('contiguous', torch.zeros((n, H, 2 * W), dtype=torch.uint8, device=dev)[..., ::2], uv, table)
    no('contiguous', y, torch.zeros((n, H, W // 2, 4), dtype=torch.uint8, device=dev)[..., ::2], table)
    no('shape', y[..., None], uv, table)                                # (n, H, W, 1)
    no('shape', y, uv[..., 0].contiguous(), table)                      # a planar U
    no('shape', y, uv.view(n, H, W, 1), table)
    no('shape', y, torch.zeros((n, H, W, 2), dtype=torch.uint8, device=dev), table)                 # 4:4:4
    no('shape', y, torch.zeros((n, H // 2, W // 2, 2), dtype=torch.uint8, device=dev), table)       # 4:2:0
    no('shape', y, uv[:1], table)
    no('even', torch.zeros((n, H, W + 1), dtype=torch.uint8, device=dev), uv, table)
    no('cell table', y[:1], uv[:1], table)                              # n != table.n
    no('cell table', torch.zeros((n, H + 1, W), dtype=torch.uint8, device=dev), torch.zeros((n, H + 1, W // 2, 2), dtype=torch.uint8, device=dev), table)
    no('border_yuv', y, uv, table, border_yuv=(1, 2))
    for bad in ((oy,), (oy, ouv, ouv), oy, (oy, ouv[..., 0]), (oy[:1], ouv), (oy, ouv.to(torch.int8)), (oy.cpu(), ouv), (ouv, oy),
                (np.zeros((n, H, W), np.uint8), ouv)):
        with pytest.raises(ValueError):
            ops.warp_nv16(y, uv, table, out=bad)
    with pytest.raises(ValueError):
        ops.warp_nv16(y, uv, table, bounds=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match='alias'):                      # what the library refuses comes back as ValueError too
        ops.warp_nv16(y, uv, table, out=(y, ouv))
    # pack / unpack / the packed warp
    for bad_order in ('YUYV', 'yvyu', 0, None):
        with pytest.raises(ValueError, match='order'):
            ops.unpack_422(packed, bad_order)
        with pytest.raises(ValueError, match='order'):
            ops.pack_422(y, uv, bad_order)
        with pytest.raises(ValueError, match='order'):
            ops.warp_packed_422(packed, table, bad_order)
    for bad in (packed[..., 0].contiguous(), packed[..., :1], packed.view(n, H, W // 2, 4), packed.to(torch.int8), packed.cpu(),
                torch.zeros((n, H, W, 4), dtype=torch.uint8, device=dev)[..., ::2], torch.zeros((n, H, W + 1, 2), dtype=torch.uint8, device=dev),
                torch.zeros((0, H, W, 2), dtype=torch.uint8, device=dev)):
        with pytest.raises(ValueError):
            ops.unpack_422(bad)
        with pytest.raises(ValueError):
            ops.warp_packed_422(bad, table)
        with pytest.raises(ValueError):
            ops.pack_422(y, uv, out=bad)
    for bad in ((oy,), (oy, ouv[:1]), (ouv, oy), (oy.cpu(), ouv), oy):
        with pytest.raises(ValueError):
            ops.unpack_422(packed, out=bad)
    with pytest.raises(ValueError):
        ops.pack_422(y, uv[:, :-1])
    with pytest.raises(ValueError):
        ops.pack_422(y[..., None], uv)
    with pytest.raises(ValueError, match='cell table'):
        ops.warp_packed_422(packed[:1], table)
    with pytest.raises(ValueError):
        ops.warp_packed_422(packed, table, out=op[:1])
    with pytest.raises(ValueError):
        ops.warp_packed_422(packed, table, border_yuv=(1,))
    with pytest.raises(ValueError):
        ops.warp_packed_422(packed, table, bounds=torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match='overlap'):
        ops.unpack_422(packed, out=(packed.view(-1)[:y.numel()].view(y.shape), ouv))
    torch.cuda.synchronize()
    assert bool((oy == 0xA5).all()) and bool((ouv == 0xA5).all()) and bool((op == 0xA5).all())
    assert bool((y == 5).all()) and bool((uv == 6).all()) and bool((packed == 7).all())
    assert torch.equal(table.crop, crop0)
