"""The NV16 crop-resize calls in the header, the ctypes table and the built library, every refusal they make before anything is launched --
invalid-argument status with the call's name in mf_last_error() --, the workspace size, every refusal of `ops.crop_resize_nv16` and
`ops.crop_resize_packed_422`, and the argument errors of `MeshFlowStabilizer.stabilized_nv16_cropped` / `stabilized_packed_422_cropped`.  The C
refusals and what Python decides before it reaches a device need no GPU; the Python refusals that need device tensors are marked gpu.

An odd H and an odd out_H are NOT refused.  A CPU test cannot let such a call reach its launch -- its addresses are the host's, and on a machine
that has a GPU the kernels would run on them --, so it shows the acceptance through the check order instead: with an odd H and an odd out_H the
call is refused only by a LATER check (overlap, the rectangle, and the last one of all, the tile count), under that check's message.  The launch
itself with odd sizes is tests/test_gpu_nv16_crop.py's."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {'mf_crop_resize_nv16_workspace_bytes': 2, 'mf_crop_resize_nv16': 15, 'mf_crop_resize_dev_nv16': 13}
N, W, H = 3, 64, 47                       # an odd H: 4:2:2 has no rule about it
OW, OH = 80, 59                           # ... nor about the output's
Y_BYTES = UV_BYTES = N * W * H
OY_BYTES = OUV_BYTES = N * OW * OH


def test_library_exports_the_calls():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    for name, nargs in CALLS.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(_lib.lib, name), name
        assert re.search(r'^(?:int|size_t) %s\(' % name, header, re.M), name
        assert header.index(name + '(') > header.index('int mf_pack_422_u8(')          # declared behind the pack / unpack pair
    assert _lib.SIGNATURES['mf_crop_resize_nv16'] == _lib.SIGNATURES['mf_crop_resize_nv12']
    assert _lib.SIGNATURES['mf_crop_resize_dev_nv16'] == _lib.SIGNATURES['mf_crop_resize_dev_nv12']
    block = header[header.index('_crop_frames (mfs.py:1111-1157) for an NV16 clip'):header.index('size_t mf_crop_resize_nv16_workspace_bytes(')]
    assert 'mfs.py:1111-1157' in block and 'c0 = min((left + 1) >> 1, c1)' in block and "LUMA table's own entry" in block
    assert 'either parity' in block and 'An odd H or out_H is not refused' in block
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if len(l.split()) == 3 and l.split()[1] == 'T'}
    assert set(CALLS) <= exported
    assert _lib.lib.mf_abi_version() == 1


def test_workspace_is_the_luma_tables_then_the_chroma_x_entries():
    from meshflow_amd import _lib
    ws, luma = _lib.lib.mf_crop_resize_nv16_workspace_bytes, _lib.lib.mf_crop_resize_workspace_bytes
    for oW, oH in ((2, 2), (2, 3), (64, 47), (1280, 189), (3840, 2160), (32766, 32767), (2, 32767)):
        assert ws(oW, oH) == luma(oW, oH) + 8 * (oW // 2), (oW, oH)
        assert luma(oW, oH) == 8 * (oW + oH)                            # (the chroma entries start on an 8-byte boundary)
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


def test_c_refusals(env):
    """Host addresses throughout, and no GPU needed: a call that got as far as a launch would not return MF_ERR_INVALID_ARG."""
    _lib, buf, base = env
    vp = ctypes.c_void_p
    at = dict(y=base, uv=base + Y_BYTES, out_y=base + Y_BYTES + UV_BYTES, out_uv=base + Y_BYTES + UV_BYTES + OY_BYTES)
    good = dict(n=N, W=W, H=H, oW=OW, oH=OH, rect=(3, 2, 60, 44), work=base, bounds=base, status=base, **at)

    def host(**kw):
        a = dict(good, **kw)
        return ('mf_crop_resize_nv16', vp(a['y']), vp(a['uv']), vp(a['out_y']), vp(a['out_uv']), a['n'], a['W'], a['H']) + tuple(a['rect']) + (
            a['oW'], a['oH'], vp(a['work']), None)

    def dev(**kw):
        a = dict(good, **kw)
        return ('mf_crop_resize_dev_nv16', vp(a['y']), vp(a['uv']), vp(a['out_y']), vp(a['out_uv']), a['n'], a['W'], a['H'], vp(a['bounds']),
                a['oW'], a['oH'], vp(a['work']), vp(a['status']), None)

    for call in (host, dev):
        for key in ('y', 'uv', 'out_y', 'out_uv', 'work'):
            assert b'null' in refused(_lib, *call(**{key: None}))
        for n in (0, -2):
            refused(_lib, *call(n=n))
        # aliasing: equal pointers, input against input, output against output, and stacks that merely overlap -- the chroma stacks are as
        # long as the luma stacks (the odd H and out_H of `good` have passed the parity checks by then)
        for kw in (dict(out_y=at['y']), dict(out_uv=at['uv']), dict(uv=at['y']), dict(out_uv=at['out_y']), dict(out_y=at['uv']), dict(out_uv=at['y']),
                   dict(out_y=at['y'] + 100), dict(out_uv=at['y'] + Y_BYTES - 2), dict(out_y=at['uv'] - OY_BYTES + 1),
                   dict(out_uv=at['out_y'] + OY_BYTES - 2), dict(uv=at['out_uv'] + OUV_BYTES - 2), dict(out_y=at['out_uv'] - OY_BYTES + 1),
                   dict(out_uv=at['uv'] + UV_BYTES // 2 + 2, uv=at['uv'])):
            assert b'alias' in refused(_lib, *call(**kw)), kw
        for kw in (dict(W=63), dict(W=65, H=49), dict(W=3), dict(W=32767)):
            err = refused(_lib, *call(**kw))
            assert b'even W' in err and b'NV16' in err, kw
        for kw in (dict(oW=79), dict(oW=3, oH=3), dict(oW=32767), dict(oW=81, oH=60)):
            err = refused(_lib, *call(**kw))
            assert b'even width' in err and b'NV16' in err, kw
        for kw in (dict(W=0), dict(H=0), dict(W=1), dict(H=1), dict(W=-64), dict(W=32768), dict(H=32768), dict(H=40000),
                   dict(oW=0), dict(oH=0), dict(oW=1), dict(oH=1), dict(oW=-80), dict(oW=32768), dict(oH=32768), dict(oH=40000)):
            assert b'32,767' in refused(_lib, *call(**kw)), kw
        for kw in (dict(uv=at['uv'] + 1), dict(out_uv=at['out_uv'] + 1), dict(uv=at['uv'] + 1, out_uv=at['out_uv'] + 3)):
            assert b'2-byte aligned' in refused(_lib, *call(**kw)), kw
        # too many tiles, the last check before the launch: 2^20 frames of 32,766 x 32,767 outputs (addresses far apart: nothing is
        # dereferenced before a launch).  H = 47 and out_H = 32,767 are odd: every check in front of this one has let them through
        far = dict(y=1 << 40, uv=2 << 40, out_y=1 << 52, out_uv=1 << 56, n=1 << 20, oW=32766, oH=32767)
        assert b'too many tiles' in refused(_lib, *call(**far))
        assert b'too many tiles' in refused(_lib, *call(**dict(far, H=4001, rect=(0, 0, 63, 4000))))
        # ... and where only the luma call's tiles are too many: chroma has half the samples in tiles of the same area
        assert b'too many tiles' in refused(_lib, *call(**dict(far, n=1 << 14)))
    for key in ('bounds', 'status'):
        assert b'null' in refused(_lib, *dev(**{key: None}))
    # an empty or out-of-frame host rectangle; the last row of the odd-H frame is a row like any other
    for rect in ((5, 3, 4, 40), (2, 9, 60, 8), (-1, 3, 60, 40), (2, -1, 60, 40), (2, 3, 64, 40), (2, 3, 60, 47)):
        assert b'rectangle' in refused(_lib, *host(rect=rect)), rect
    assert bytes(buf) == bytes(len(buf))                                # nothing was written anywhere


def test_nv12_and_p010_messages_are_what_they_were(env):
    """The entry the three formats now share keeps the 4:2:0 calls' words: an odd H or out_H is still theirs to refuse."""
    _lib, buf, base = env
    vp = ctypes.c_void_p
    for fmt, noun in (('nv12', b'an NV12'), ('p010', b'a P010')):
        for kw, msg in ((dict(H=47), b'frame has an even W and H, got W=64 H=47'), (dict(oH=59), b'output has an even size, got 80x59')):
            a = dict(W=64, H=48, oW=80, oH=60)
            a.update(kw)
            name = 'mf_crop_resize_' + fmt
            rc = getattr(_lib.lib, name)(vp(base), vp(base + (1 << 20)), vp(base + (1 << 21)), vp(base + (1 << 22)), 1, a['W'], a['H'], 0, 0, 9, 9,
                                         a['oW'], a['oH'], vp(base), None)
            err = _lib.lib.mf_last_error()
            assert rc == _lib.MF_ERR_INVALID_ARG and name.encode() + b': ' + noun + b' ' + msg in err, err


def test_python_refusals_before_the_library():
    """What `ops.crop_resize_nv16`, `ops.crop_resize_packed_422` and the two stabilizer calls decide without a device."""
    torch = pytest.importorskip('torch')
    from meshflow_amd import ops
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    y, uv = torch.zeros((2, 3, 8), dtype=torch.uint8), torch.zeros((2, 3, 4, 2), dtype=torch.uint8)
    packed = torch.zeros((2, 3, 8, 2), dtype=torch.uint8)
    with pytest.raises(ValueError, match='y must be a CUDA/HIP'):
        ops.crop_resize_nv16(y, uv, (0, 0, 7, 2))
    with pytest.raises(ValueError, match='y must be a CUDA/HIP'):
        ops.crop_resize_nv16(y.numpy(), uv, (0, 0, 7, 2))
    with pytest.raises(ValueError, match='packed must be a CUDA/HIP'):
        ops.crop_resize_packed_422(packed, (0, 0, 7, 2))
    for bad in ((3, 4), (0, 2), (2, 32768), (2,), (2.0, 4), None, (5, 5)):
        with pytest.raises(ValueError):
            ops._yuv_output_size(ops._NV16, bad)
    with pytest.raises(ValueError, match='an NV16 output has an even width'):
        ops._yuv_output_size(ops._NV16, (3, 4))
    assert ops._yuv_output_size(ops._NV16, (2, 32767)) == (2, 32767) and ops._yuv_output_size(ops._NV16, (4, 3)) == (4, 3)
    with pytest.raises(ValueError, match='an NV12 output has an even width and height'):      # the 4:2:0 formats keep their rule and their words
        ops._yuv_output_size(ops._NV12, (4, 3))
    assert ops._NV16.half_rows is False and None not in ops._NV16
    s = MeshFlowStabilizer(mesh_row_count=2, mesh_col_count=2, device='cpu')
    disp = torch.zeros((2, 3, 3, 2), dtype=torch.float64)
    for bad in ((7, 4), (0, 4), (8, 32768), (8,)):
        with pytest.raises(ValueError, match='output_size'):
            s.stabilized_nv16_cropped(y, uv, disp, None, output_size=bad)
    with pytest.raises(ValueError, match='d_packed must be a CUDA/HIP'):
        s.stabilized_packed_422_cropped(packed, disp, None)
    # the uncropped calls keep their signatures
    with pytest.raises(TypeError):
        s.stabilized_nv16(y, uv, disp, None, crop=True)
    with pytest.raises(TypeError):
        s.stabilized_packed_422(packed, disp, None, output_size=(8, 3))


@pytest.mark.gpu
def test_python_refusals_on_the_device():
    torch = pytest.importorskip('torch')
    import numpy as np
    from meshflow_amd import online, ops
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    dev = torch.device('cuda:0')
    n, H, W = 2, 15, 24
    rect = (3, 2, 20, 13)
    y = torch.full((n, H, W), 5, dtype=torch.uint8, device=dev)
    uv = torch.full((n, H, W // 2, 2), 6, dtype=torch.uint8, device=dev)
    packed = torch.full((n, H, W, 2), 7, dtype=torch.uint8, device=dev)
    oy, ouv, op = torch.full_like(y, 0xA5), torch.full_like(uv, 0xA5), torch.full_like(packed, 0xA5)
    bounds = torch.tensor(rect, dtype=torch.int32, device=dev)

    def no(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            ops.crop_resize_nv16(*args, **kw)

    for b in (rect, bounds):
        no('dtype', y.to(torch.int8), uv, b)
        no('dtype', y, uv.to(torch.int16), b)
        no('CUDA/HIP', y, uv.cpu(), b)
        no('contiguous', torch.zeros((n, H, 2 * W), dtype=torch.uint8, device=dev)[..., ::2], uv, b)
        no('contiguous', y, uv[..., 0], b)
        no('shape', y[..., None], uv, b)
        no('shape', y, uv[..., 0].contiguous(), b)
        no('shape', y, torch.zeros((n, H, W, 2), dtype=torch.uint8, device=dev), b)                  # 4:4:4
        no('shape', y, torch.zeros((n, H // 2, W // 2, 2), dtype=torch.uint8, device=dev), b)        # 4:2:0
        no('shape', y, uv[:1], b)
        no('even', torch.zeros((n, H, W + 1), dtype=torch.uint8, device=dev), uv, b)
        for size in ((23, 16), (0, 16), (24, 32768), (24,), 24, (24, 1)):
            no('size', y, uv, b, size=size)
        for bad in ((oy,), (oy, ouv, ouv), oy, (oy, ouv[..., 0]), (oy[:1], ouv), (oy, ouv.to(torch.int8)), (oy.cpu(), ouv), (ouv, oy),
                    (np.zeros((n, H, W), np.uint8), ouv)):
            with pytest.raises(ValueError):
                ops.crop_resize_nv16(y, uv, b, out=bad)
        no('shape', y, uv, b, size=(32, 21), out=(oy, ouv))                 # an `out` of the frame's size for another output size
        no('alias', y, uv, b, out=(y, ouv))
        no('alias', y, uv, b, out=(oy, uv))
        for bad_order in ('YUYV', 'yvyu', 0, None):
            with pytest.raises(ValueError, match='order'):
                ops.crop_resize_packed_422(packed, b, bad_order)
        for bad in (packed[..., 0].contiguous(), packed.view(n, H, W // 2, 4), packed.to(torch.int8), packed.cpu(),
                    torch.zeros((n, H, W + 1, 2), dtype=torch.uint8, device=dev)):
            with pytest.raises(ValueError):
                ops.crop_resize_packed_422(bad, b)
        with pytest.raises(ValueError, match='size'):
            ops.crop_resize_packed_422(packed, b, size=(23, 15))
        with pytest.raises(ValueError):
            ops.crop_resize_packed_422(packed, b, size=(32, 21), out=op)
    no('status', y, uv, rect, status=torch.zeros(1, dtype=torch.int32, device=dev))
    no('status', y, uv, bounds, status=torch.zeros(2, dtype=torch.int32, device=dev))
    no('dtype', y, uv, bounds, status=torch.zeros(1, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match='status'):
        ops.crop_resize_packed_422(packed, rect, status=torch.zeros(1, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.crop_resize_nv16(y, uv, torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.crop_resize_nv16(y, uv, torch.zeros(4, dtype=torch.int64, device=dev))
    for bad in ((5, 3, 4, 10), (-1, 0, 23, 14), (0, 0, 24, 14), (0, 0, 23, 15), (0, 9, 23, 8)):
        no('rectangle', y, uv, bad)
    # `online.luma_of`: an NV16 pair is told by its d_uv's rows; every other pair meets the NV12 / P010 checks and their words
    form, luma = online.luma_of((y, uv))
    assert form.fmt is ops._NV16 and luma is y and form.pair
    y14 = torch.zeros((n, 14, W), dtype=torch.uint8, device=dev)

    def chroma(*shape):
        return torch.zeros(shape + (W // 2, 2), dtype=torch.uint8, device=dev)

    assert online.luma_of((y14, chroma(n, 7)))[0].fmt is ops._NV12 and online.luma_of((y14, chroma(n, 14)))[0].fmt is ops._NV16
    with pytest.raises(ValueError, match='an NV12 frame has an even width and height'):
        online.luma_of((y, chroma(n, 7)))
    with pytest.raises(ValueError, match='uv must have shape'):
        online.luma_of((y14, chroma(n, 8)))
    with pytest.raises(ValueError, match='uv must have shape'):
        online.luma_of((y14, chroma(1, 14)))
    torch.cuda.synchronize()
    assert bool((oy == 0xA5).all()) and bool((ouv == 0xA5).all()) and bool((op == 0xA5).all())
    assert bool((y == 5).all()) and bool((uv == 6).all()) and bool((packed == 7).all())
