"""The seven P210 / Y210 calls in the header, the ctypes table and the built library, every refusal they make before anything is launched --
invalid-argument status with the call's name in mf_last_error() --, the workspace size, and the refusals of the Python calls (`ops.warp_p210`,
`ops.crop_resize_p210`, `ops.unpack_y210`, `ops.pack_y210`, `ops.warp_y210`, `ops.crop_resize_y210`, the four stabilizer calls,
`online.luma_of`).  The C refusals and what Python decides before it reaches a device need no GPU; the rest is marked gpu.

An odd H and an odd out_H are NOT refused.  A CPU test cannot let such a call reach its launch -- its addresses are the host's --, so it shows
the acceptance through the check order instead: with an odd H the call is refused only by a LATER check (the mesh, overlap, the rectangle, the
tile count), under that check's message.  The launch itself with odd sizes is tests/test_gpu_p210.py's and tests/test_gpu_p210_crop.py's."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {'mf_warp_p210': 13, 'mf_warp_bounds_p210': 14, 'mf_crop_resize_p210_workspace_bytes': 2, 'mf_crop_resize_p210': 15,
         'mf_crop_resize_dev_p210': 13, 'mf_unpack_y210_u16': 7, 'mf_pack_y210_u16': 7}
N, W, H = 3, 64, 47                       # an odd H: 4:2:2 has no rule about it
OW, OH = 80, 59                           # ... nor about the output's
Y_BYTES = UV_BYTES = 2 * N * W * H
OY_BYTES = OUV_BYTES = 2 * N * OW * OH


def test_library_exports_the_calls():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    for name, nargs in CALLS.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(_lib.lib, name), name
        assert re.search(r'^(?:int|size_t) %s\(' % name, header, re.M), name
    for op in ('mf_warp_', 'mf_warp_bounds_', 'mf_crop_resize_', 'mf_crop_resize_dev_'):
        assert _lib.SIGNATURES[op + 'p210'] == _lib.SIGNATURES[op + 'p010'], op
    block = header[header.index('---- P210 clips'):header.index('int mf_warp_p210(')]
    assert 'mfs.py:1063-1069' in block and 'either parity' in block and 'An odd H is not' in block and 'v210' in block
    block = header[header.index('Packed Y210 / Y216 against the P210 pair'):header.index('int mf_unpack_y210_u16(')]
    assert 'd_packed 8-byte aligned' in block and 'd_y and d_uv 2-byte aligned' in block
    block = header[header.index('_crop_frames (mfs.py:1111-1157) for a P210 clip'):header.index('size_t mf_crop_resize_p210_workspace_bytes(')]
    assert "LUMA table's own entry" in block and 'NO area branch' in block and 'An odd H or out_H is not refused' in block
    assert 'No 10-bit 4:2:2' not in header
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if len(l.split()) == 3 and l.split()[1] == 'T'}
    assert set(CALLS) <= exported
    assert _lib.lib.mf_abi_version() == 1


def test_workspace_is_the_luma_tables_then_the_chroma_x_entries():
    from meshflow_amd import _lib
    ws, luma, p010 = (_lib.lib.mf_crop_resize_p210_workspace_bytes, _lib.lib.mf_crop_resize_workspace_bytes,
                      _lib.lib.mf_crop_resize_p010_workspace_bytes)
    for oW, oH in ((2, 2), (2, 3), (64, 47), (1280, 189), (3840, 2160), (32766, 32767), (2, 32767)):
        assert ws(oW, oH) == luma(oW, oH) + 8 * (oW // 2), (oW, oH)
        assert luma(oW, oH) == 8 * (oW + oH)                            # (the chroma entries start on an 8-byte boundary)
        assert ws(oW, oH) == p010(oW, oH) - 8 * (oH // 2)               # P010's layout without its second y table
    assert ws(0, 4) == 0 and ws(4, -2) == 0


@pytest.fixture(scope='module')
def env():
    from meshflow_amd import _lib
    buf = (ctypes.c_uint8 * (Y_BYTES + UV_BYTES + OY_BYTES + OUV_BYTES + 64))()
    base = (ctypes.addressof(buf) + 15) & ~15
    return _lib, buf, base


def refused(_lib, name, *args):
    rc = getattr(_lib.lib, name)(*args)
    err = _lib.lib.mf_last_error()
    assert rc == _lib.MF_ERR_INVALID_ARG, (name, args, rc, err)
    assert name.encode() + b':' in err, (name, err)
    return err


def test_c_refusals_of_the_warp(env):
    """Host addresses throughout, and no GPU needed: a call that got as far as a launch would not return MF_ERR_INVALID_ARG."""
    _lib, buf, base = env
    vp = ctypes.c_void_p
    border = (ctypes.c_uint16 * 3)(4660, 51966, 300)
    at = dict(y=base, uv=base + Y_BYTES, out_y=base + 2 * Y_BYTES, out_uv=base + 3 * Y_BYTES)
    good = dict(n=N, W=W, H=H, R=4, C=4, table=base, border=ctypes.addressof(border), crop=base, bounds=base, **at)

    def plain(**kw):
        a = dict(good, **kw)
        return ('mf_warp_p210', vp(a['y']), vp(a['uv']), vp(a['out_y']), vp(a['out_uv']), vp(a['table']), a['n'], a['W'], a['H'], a['R'], a['C'],
                vp(a['border']), vp(a['crop']), None)

    def with_bounds(**kw):
        a = dict(good, **kw)
        return ('mf_warp_bounds_p210',) + plain(**kw)[1:-1] + (vp(a['bounds']), None)

    for call in (plain, with_bounds):
        for key in ('y', 'uv', 'out_y', 'out_uv', 'table', 'border', 'crop'):
            assert b'null' in refused(_lib, *call(**{key: None}))
        for n in (0, -2):
            assert b'bad sizes' in refused(_lib, *call(n=n))
        for kw in (dict(W=0), dict(H=0), dict(W=1), dict(H=1), dict(W=32768), dict(H=40000)):
            assert b'32,767' in refused(_lib, *call(**kw)), kw
        for kw in (dict(W=63), dict(W=65, H=48), dict(W=3)):
            assert b'a P210 frame has an even W, got' in refused(_lib, *call(**kw)), kw
        # the check order: the odd H = 47 of `good` has passed the parity check and is refused only by what comes later
        for kw in (dict(R=0), dict(C=65), dict(R=-1, C=2)):
            assert b'outside 1 .. 64' in refused(_lib, *call(**kw)), kw
        for kw in (dict(y=at['y'] + 1), dict(uv=at['uv'] + 1), dict(out_y=at['out_y'] + 1), dict(out_uv=at['out_uv'] + 3)):
            assert b'd_y, d_uv, d_out_y and d_out_uv must be 2-byte aligned' in refused(_lib, *call(**kw)), kw
        # aliasing of the four stacks: every stack is 2 n W H bytes, odd H included
        for kw in (dict(out_y=at['y']), dict(out_uv=at['uv']), dict(uv=at['y']), dict(out_uv=at['out_y']), dict(out_y=at['uv']),
                   dict(out_uv=at['y']), dict(uv=at['y'] + Y_BYTES - 2), dict(out_y=at['uv'] + UV_BYTES - 2),
                   dict(out_uv=at['out_y'] + Y_BYTES - 2), dict(out_uv=at['uv'] - UV_BYTES + 2)):
            assert b'alias' in refused(_lib, *call(**kw)), kw
    assert b'null' in refused(_lib, *with_bounds(bounds=None))
    # P010 keeps its rule and its words: the odd H is its to refuse
    rc = _lib.lib.mf_warp_p010(vp(at['y']), vp(at['uv']), vp(at['out_y']), vp(at['out_uv']), vp(base), N, W, H, 4, 4, vp(ctypes.addressof(border)),
                               vp(base), None)
    assert rc == _lib.MF_ERR_INVALID_ARG and b'mf_warp_p010: a P010 frame has an even W and H, got W=64 H=47' in _lib.lib.mf_last_error()
    assert bytes(buf) == bytes(len(buf))                                # nothing was written anywhere


def test_c_refusals_of_the_crop(env):
    _lib, buf, base = env
    vp = ctypes.c_void_p
    at = dict(y=base, uv=base + Y_BYTES, out_y=base + Y_BYTES + UV_BYTES, out_uv=base + Y_BYTES + UV_BYTES + OY_BYTES)
    good = dict(n=N, W=W, H=H, oW=OW, oH=OH, rect=(3, 2, 60, 44), work=base, bounds=base, status=base, **at)

    def host(**kw):
        a = dict(good, **kw)
        return ('mf_crop_resize_p210', vp(a['y']), vp(a['uv']), vp(a['out_y']), vp(a['out_uv']), a['n'], a['W'], a['H']) + tuple(a['rect']) + (
            a['oW'], a['oH'], vp(a['work']), None)

    def dev(**kw):
        a = dict(good, **kw)
        return ('mf_crop_resize_dev_p210', vp(a['y']), vp(a['uv']), vp(a['out_y']), vp(a['out_uv']), a['n'], a['W'], a['H'], vp(a['bounds']),
                a['oW'], a['oH'], vp(a['work']), vp(a['status']), None)

    for call in (host, dev):
        for key in ('y', 'uv', 'out_y', 'out_uv', 'work'):
            assert b'null' in refused(_lib, *call(**{key: None}))
        for n in (0, -2):
            assert b'bad sizes n=' in refused(_lib, *call(n=n))
        for kw in (dict(out_y=at['y']), dict(out_uv=at['uv']), dict(uv=at['y']), dict(out_uv=at['out_y']), dict(out_y=at['uv']), dict(out_uv=at['y']),
                   dict(out_y=at['y'] + 100), dict(out_uv=at['y'] + Y_BYTES - 2), dict(out_y=at['uv'] - OY_BYTES + 2),
                   dict(out_uv=at['out_y'] + OY_BYTES - 2), dict(uv=at['out_uv'] + OUV_BYTES - 2), dict(out_y=at['out_uv'] - OY_BYTES + 2)):
            assert b'alias' in refused(_lib, *call(**kw)), kw
        for kw in (dict(W=63), dict(W=65, H=49), dict(W=3), dict(W=32767)):
            assert b'a P210 frame has an even W, got' in refused(_lib, *call(**kw)), kw
        for kw in (dict(oW=79), dict(oW=3, oH=3), dict(oW=32767), dict(oW=81, oH=60)):
            assert b'a P210 output has an even width, got' in refused(_lib, *call(**kw)), kw
        for kw in (dict(W=0), dict(H=0), dict(W=1), dict(H=1), dict(W=-64), dict(W=32768), dict(H=32768), dict(H=40000),
                   dict(oW=0), dict(oH=0), dict(oW=1), dict(oH=1), dict(oW=-80), dict(oW=32768), dict(oH=32768), dict(oH=40000)):
            assert b'32,767' in refused(_lib, *call(**kw)), kw
        for kw in (dict(y=at['y'] + 1), dict(uv=at['uv'] + 1), dict(out_y=at['out_y'] + 1), dict(out_uv=at['out_uv'] + 1),
                   dict(uv=at['uv'] + 1, out_uv=at['out_uv'] + 3)):
            assert b'd_y, d_uv, d_out_y and d_out_uv must be 2-byte aligned' in refused(_lib, *call(**kw)), kw
        # too many tiles, the last check before the launch (addresses far apart: nothing is dereferenced before a launch).  H = 47 and
        # out_H = 32,767 are odd: every check in front of this one has let them through
        far = dict(y=1 << 40, uv=2 << 40, out_y=1 << 52, out_uv=1 << 56, n=1 << 20, oW=32766, oH=32767)
        assert b'too many tiles' in refused(_lib, *call(**far))
        assert b'too many tiles' in refused(_lib, *call(**dict(far, H=4001, rect=(0, 0, 63, 4000))))
    for key in ('bounds', 'status'):
        assert b'null' in refused(_lib, *dev(**{key: None}))
    # an empty or out-of-frame host rectangle; the last row of the odd-H frame is a row like any other
    for rect in ((5, 3, 4, 40), (2, 9, 60, 8), (-1, 3, 60, 40), (2, -1, 60, 40), (2, 3, 64, 40), (2, 3, 60, 47)):
        assert b'rectangle' in refused(_lib, *host(rect=rect)), rect
    # P010 keeps its words
    for kw, msg in ((dict(H=47), b'a P010 frame has an even W and H, got W=64 H=47'), (dict(oH=59), b'a P010 output has an even size, got 80x59')):
        a = dict(W=64, H=48, oW=80, oH=60)
        a.update(kw)
        rc = _lib.lib.mf_crop_resize_p010(vp(base), vp(base + (1 << 20)), vp(base + (1 << 21)), vp(base + (1 << 22)), 1, a['W'], a['H'], 0, 0, 9, 9,
                                          a['oW'], a['oH'], vp(base), None)
        assert rc == _lib.MF_ERR_INVALID_ARG and b'mf_crop_resize_p010: ' + msg in _lib.lib.mf_last_error()
    assert bytes(buf) == bytes(len(buf))


def test_c_refusals_of_y210(env):
    _lib, buf, base = env
    vp = ctypes.c_void_p
    words = N * (W // 2) * H
    at = dict(packed=base, y=base + 8 * words, uv=base + 12 * words)
    good = dict(n=N, W=W, H=H, **at)

    def unpack(**kw):
        a = dict(good, **kw)
        return ('mf_unpack_y210_u16', vp(a['packed']), vp(a['y']), vp(a['uv']), a['n'], a['W'], a['H'], None)

    def pack(**kw):
        a = dict(good, **kw)
        return ('mf_pack_y210_u16', vp(a['y']), vp(a['uv']), vp(a['packed']), a['n'], a['W'], a['H'], None)

    for call in (unpack, pack):
        for key in ('packed', 'y', 'uv'):
            assert b'null' in refused(_lib, *call(**{key: None}))
        for n in (0, -1):
            assert b'n must be at least 1' in refused(_lib, *call(n=n))
        for w in (0, 1, 63, 32767, 32768, -2):
            assert b'W must be even and in 2 .. 32767' in refused(_lib, *call(W=w)), w
        for h in (0, -1, 32768):
            assert b'H must be in 1 .. 32767' in refused(_lib, *call(H=h)), h
        # the alignment contract: packed to 8 bytes, the planes to 2
        for off in (1, 2, 4, 6, 12):
            assert b'd_packed must be 8-byte aligned' in refused(_lib, *call(packed=at['packed'] + off)), off
        for kw in (dict(y=at['y'] + 1), dict(uv=at['uv'] + 1), dict(y=at['y'] + 3, uv=at['uv'] + 5)):
            assert b'd_y and d_uv must be 2-byte aligned' in refused(_lib, *call(**kw)), kw
        for kw in (dict(y=at['packed']), dict(uv=at['packed'] + 8), dict(uv=at['y']), dict(y=at['packed'] + 8 * words - 2),
                   dict(uv=at['y'] + 4 * words - 2), dict(uv=at['y'] - 4 * words + 2)):
            assert b'overlap' in refused(_lib, *call(**kw)), kw
    # the 8-bit pair keeps what it refuses: a 4-byte aligned packed pointer is its rule, an order other than 0 or 1 its refusal
    rc = _lib.lib.mf_unpack_422_u8(vp(base + 2), vp(base + 8 * words), vp(base + 12 * words), N, W, H, 0, None)
    assert rc == _lib.MF_ERR_INVALID_ARG and b'd_packed must be 4-byte aligned' in _lib.lib.mf_last_error()
    rc = _lib.lib.mf_pack_422_u8(vp(base + 8 * words), vp(base + 12 * words), vp(base), N, W, H, 2, None)
    assert rc == _lib.MF_ERR_INVALID_ARG and b'order must be 0' in _lib.lib.mf_last_error()
    assert bytes(buf) == bytes(len(buf))


def test_python_refusals_before_the_library():
    """What the Python calls decide without a device."""
    torch = pytest.importorskip('torch')
    from meshflow_amd import ops
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    y, uv = torch.zeros((2, 3, 8), dtype=torch.uint16), torch.zeros((2, 3, 4, 2), dtype=torch.uint16)
    packed = torch.zeros((2, 3, 8, 2), dtype=torch.uint16)
    assert ops._P210.half_rows is False and ops._P210.dtype == torch.uint16 and ops._P210.noun == 'a P210' and None not in ops._P210
    assert ops._P210.border is ops._P010.border
    with pytest.raises(ValueError, match='y must be a CUDA/HIP'):
        ops.crop_resize_p210(y, uv, (0, 0, 7, 2))
    with pytest.raises(ValueError, match='y must be a CUDA/HIP'):
        ops.warp_p210(y, uv, None)
    for call in (ops.unpack_y210, lambda p: ops.warp_y210(p, None), lambda p: ops.crop_resize_y210(p, (0, 0, 7, 2))):
        with pytest.raises(ValueError, match='packed must be a CUDA/HIP'):
            call(packed)
    with pytest.raises(ValueError, match='y must be a CUDA/HIP'):
        ops.pack_y210(y, uv)
    with pytest.raises(ValueError, match='a P210 output has an even width'):
        ops._yuv_output_size(ops._P210, (3, 4))
    assert ops._yuv_output_size(ops._P210, (2, 32767)) == (2, 32767) and ops._yuv_output_size(ops._P210, (4, 3)) == (4, 3)
    with pytest.raises(ValueError, match='an NV12 output has an even width and height'):      # P010 keeps the 4:2:0 rule and its words
        ops._yuv_output_size(ops._P010, (4, 3))
    s = MeshFlowStabilizer(mesh_row_count=2, mesh_col_count=2, device='cpu')
    disp = torch.zeros((2, 3, 3, 2), dtype=torch.float64)
    for bad in ((7, 4), (0, 4), (8, 32768), (8,)):
        with pytest.raises(ValueError, match='output_size'):
            s.stabilized_p210_cropped(y, uv, disp, None, output_size=bad)
        with pytest.raises(ValueError):
            s.stabilized_y210_cropped(packed, disp, None, output_size=bad)
    with pytest.raises(ValueError, match='d_packed must be a CUDA/HIP'):
        s.stabilized_y210_cropped(packed, disp, None)
    with pytest.raises(ValueError, match='d_packed must be a CUDA/HIP'):
        s.stabilized_y210(packed, disp, None)
    with pytest.raises(ValueError, match='d_y must be a CUDA/HIP'):
        s.stabilized_p210(y, uv, disp, None)
    # the uncropped calls take neither crop nor output_size
    with pytest.raises(TypeError):
        s.stabilized_p210(y, uv, disp, None, crop=True)
    with pytest.raises(TypeError):
        s.stabilized_y210(packed, disp, None, output_size=(8, 3))
    # the P010 entry keeps its refusal
    with pytest.raises(ValueError, match='stabilized_p010_cropped'):
        s.stabilized_p010(y, uv, disp, None, crop=True)


@pytest.mark.gpu
def test_python_refusals_on_the_device():
    torch = pytest.importorskip('torch')
    from meshflow_amd import online, ops
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    dev = torch.device('cuda:0')
    n, H, W = 2, 15, 24
    rect = (3, 2, 20, 13)
    import numpy as np

    def full16(shape, v):
        """(uint16 tensors are made as int16 and viewed: torch fills and compares few unsigned types on the device)"""
        return torch.full(shape, int(np.array(v, np.uint16).view(np.int16)), dtype=torch.int16, device=dev).view(torch.uint16)

    def all16(t, v):
        return bool((t.cpu().numpy() == v).all())

    y, uv, packed = full16((n, H, W), 5), full16((n, H, W // 2, 2), 6), full16((n, H, W, 2), 7)
    oy, ouv, op = full16(y.shape, 0xA5A5), full16(uv.shape, 0xA5A5), full16(packed.shape, 0xA5A5)
    bounds = torch.tensor(rect, dtype=torch.int32, device=dev)

    def no(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            ops.crop_resize_p210(*args, **kw)

    for b in (rect, bounds):
        no('dtype', torch.zeros((n, H, W), dtype=torch.uint8, device=dev), uv, b)
        no('dtype', y, uv.view(torch.int16), b)
        no('CUDA/HIP', y, uv.cpu(), b)
        no('contiguous', y, uv[..., 0], b)
        no('shape', y[..., None], uv, b)
        no('shape', y, full16((n, H, W, 2), 0), b)                  # 4:4:4
        no('shape', y, full16((n, H // 2, W // 2, 2), 0), b)        # 4:2:0
        no('shape', y, uv[:1], b)
        no('even', full16((n, H, W + 1), 0), uv, b)
        for size in ((23, 16), (0, 16), (24, 32768), (24,), 24, (24, 1)):
            no('size', y, uv, b, size=size)
        for bad in ((oy,), oy, (oy, ouv[..., 0]), (oy[:1], ouv), (oy, ouv.view(torch.int16)), (oy.cpu(), ouv), (ouv, oy)):
            with pytest.raises(ValueError):
                ops.crop_resize_p210(y, uv, b, out=bad)
        no('shape', y, uv, b, size=(32, 21), out=(oy, ouv))
        no('alias', y, uv, b, out=(y, ouv))
        no('alias', y, uv, b, out=(oy, uv))
        for bad in (packed[..., 0].contiguous(), packed.view(n, H, W // 2, 4), packed.view(torch.int16), packed.cpu(),
                    torch.zeros((n, H, W, 2), dtype=torch.uint8, device=dev), full16((n, H, W + 1, 2), 0)):
            with pytest.raises(ValueError):
                ops.crop_resize_y210(bad, b)
            with pytest.raises(ValueError):
                ops.unpack_y210(bad)
        with pytest.raises(ValueError, match='size'):
            ops.crop_resize_y210(packed, b, size=(23, 15))
        with pytest.raises(ValueError):
            ops.crop_resize_y210(packed, b, size=(32, 21), out=op)
    no('status', y, uv, rect, status=torch.zeros(1, dtype=torch.int32, device=dev))
    for bad in ((5, 3, 4, 10), (-1, 0, 23, 14), (0, 0, 24, 14), (0, 0, 23, 15), (0, 9, 23, 8)):
        no('rectangle', y, uv, bad)
    # the 8-bit pack / unpack pair refuses uint16, and the uint16 pair uint8: neither took over the other's clips
    with pytest.raises(ValueError, match='dtype'):
        ops.unpack_422(packed)
    with pytest.raises(ValueError, match='dtype'):
        ops.pack_422(y, uv)
    with pytest.raises(ValueError, match='dtype'):
        ops.pack_y210(torch.zeros((n, H, W), dtype=torch.uint8, device=dev), torch.zeros((n, H, W // 2, 2), dtype=torch.uint8, device=dev))
    with pytest.raises(ValueError, match='overlap'):
        ops.unpack_y210(packed, out=(packed.view(-1)[:n * H * W].view(n, H, W), ouv))
    # Y210's alignment contract: a packed view 4 bytes into its storage is refused by the library
    store = full16((n * H * W * 2 + 8,), 0)
    with pytest.raises(Exception, match='8-byte aligned'):
        ops.unpack_y210(store[2:2 + n * H * W * 2].view(n, H, W, 2))
    # `online.luma_of`: a P210 pair is told from a P010 one by its d_uv's rows; every other uint16 pair meets the P010 checks and their words
    form, luma = online.luma_of((y, uv))
    assert form.fmt is ops._P210 and form.pair and luma.dtype == torch.uint8 and tuple(luma.shape) == (n, H, W)
    y14 = full16((n, 14, W), 0)

    def chroma(*shape):
        return full16(shape + (W // 2, 2), 0)

    assert online.luma_of((y14, chroma(n, 7)))[0].fmt is ops._P010 and online.luma_of((y14, chroma(n, 14)))[0].fmt is ops._P210
    with pytest.raises(ValueError, match='a P010 frame has an even width and height'):
        online.luma_of((y, chroma(n, 7)))
    with pytest.raises(ValueError, match='uv must have shape'):
        online.luma_of((y14, chroma(n, 8)))
    with pytest.raises(ValueError, match='uv must have shape'):
        online.luma_of((y14, chroma(1, 14)))
    torch.cuda.synchronize()
    assert all16(oy, 0xA5A5) and all16(ouv, 0xA5A5) and all16(op, 0xA5A5)
    assert all16(y, 5) and all16(uv, 6) and all16(packed, 7)
