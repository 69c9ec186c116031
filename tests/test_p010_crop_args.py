"""The P010 crop-resize calls in the header, the ctypes table and the built library, every refusal they make before anything is launched --
invalid-argument status with the call's name in mf_last_error() --, the workspace size, every refusal of `ops.crop_resize_p010` and the argument
errors of `MeshFlowStabilizer.stabilized_p010_cropped`.  The C refusals and what Python decides before it reaches a device need no GPU; the
Python refusals that need device tensors are marked gpu."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {'mf_crop_resize_p010_workspace_bytes': 2, 'mf_crop_resize_p010': 15, 'mf_crop_resize_dev_p010': 13}
N, W, H = 3, 64, 48
OW, OH = 80, 60
Y_BYTES, UV_BYTES = 2 * N * W * H, N * (W // 2) * (H // 2) * 4
OY_BYTES, OUV_BYTES = 2 * N * OW * OH, N * (OW // 2) * (OH // 2) * 4


def test_library_exports_the_calls():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    for name, nargs in CALLS.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(_lib.lib, name), name
        assert re.search(r'\b(?:int|size_t) %s\(' % name, header), name
    block = header[header.index('_crop_frames (mfs.py:1111-1157) for a P010 clip'):header.index('size_t mf_crop_resize_p010_workspace_bytes(')]
    for text in ('mfs.py:1111-1157', 'even luma sample', 'c0 = min((left + 1) >> 1, c1)', 'NO\n * area branch', 'f = 0.25', 'nothing is masked',
                 '(S00 + S01 + S10 + S11 + 2) >> 2', 'no 2048 quantisation'):
        assert text in block, text
    assert _lib.lib.mf_abi_version() == 1


def test_header_library_and_ctypes_table_list_the_same_calls():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    declared = set(re.findall(r'^(?:int|size_t|const char\*)\s+(mf_\w+)\(', header, re.M))
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if len(l.split()) == 3 and l.split()[1] == 'T' and l.split()[-1].startswith('mf_')}
    assert set(CALLS) <= declared
    assert declared == exported == set(_lib.SIGNATURES)


def test_workspace_holds_the_luma_tables_and_the_chroma_tables():
    from meshflow_amd import _lib
    ws, luma = _lib.lib.mf_crop_resize_p010_workspace_bytes, _lib.lib.mf_crop_resize_workspace_bytes
    for oW, oH in ((2, 2), (64, 48), (1280, 190), (3840, 2160), (32766, 32766), (2, 32766)):
        assert ws(oW, oH) == luma(oW, oH) + 8 * (oW // 2 + oH // 2), (oW, oH)
        assert luma(oW, oH) % 8 == 0                                    # the chroma tables start on an 8-byte boundary
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
    good = dict(n=N, W=W, H=H, oW=OW, oH=OH, rect=(3, 2, 60, 45), work=base, bounds=base, status=base, **at)

    def host(**kw):
        a = dict(good, **kw)
        return ('mf_crop_resize_p010', vp(a['y']), vp(a['uv']), vp(a['out_y']), vp(a['out_uv']), a['n'], a['W'], a['H']) + tuple(a['rect']) + (
            a['oW'], a['oH'], vp(a['work']), None)

    def dev(**kw):
        a = dict(good, **kw)
        return ('mf_crop_resize_dev_p010', vp(a['y']), vp(a['uv']), vp(a['out_y']), vp(a['out_uv']), a['n'], a['W'], a['H'], vp(a['bounds']),
                a['oW'], a['oH'], vp(a['work']), vp(a['status']), None)

    for call in (host, dev):
        for key in ('y', 'uv', 'out_y', 'out_uv', 'work'):
            assert b'null' in refused(_lib, *call(**{key: None}))
        for n in (0, -2):
            refused(_lib, *call(n=n))
        # aliasing: equal pointers, input against input, output against output, and stacks that merely overlap (by one sample)
        for kw in (dict(out_y=at['y']), dict(out_uv=at['uv']), dict(uv=at['y']), dict(out_uv=at['out_y']), dict(out_y=at['uv']), dict(out_uv=at['y']),
                   dict(out_y=at['y'] + 100), dict(out_uv=at['y'] + Y_BYTES - 2), dict(out_y=at['uv'] - OY_BYTES + 2),
                   dict(out_uv=at['out_y'] + OY_BYTES - 2), dict(uv=at['out_uv'] + OUV_BYTES - 2), dict(out_y=at['out_uv'] - OY_BYTES + 2)):
            assert b'alias' in refused(_lib, *call(**kw)), kw
        for kw in (dict(W=63), dict(H=47), dict(W=65, H=49), dict(W=3), dict(H=32767)):
            assert b'even' in refused(_lib, *call(**kw)), kw
        for kw in (dict(oW=79), dict(oH=61), dict(oW=3, oH=3), dict(oW=32767), dict(oH=32767)):
            assert b'even' in refused(_lib, *call(**kw)), kw
        for kw in (dict(W=0), dict(H=0), dict(W=1), dict(H=1), dict(W=-64), dict(W=32768), dict(H=32768), dict(H=40000),
                   dict(oW=0), dict(oH=0), dict(oW=1), dict(oH=1), dict(oW=-80), dict(oW=32768), dict(oH=32768), dict(oH=40000)):
            assert b'32,767' in refused(_lib, *call(**kw)), kw
        # every one of the four plane pointers must be 2-byte aligned
        for kw in (dict(y=at['y'] + 1), dict(uv=at['uv'] + 1), dict(out_y=at['out_y'] + 1), dict(out_uv=at['out_uv'] + 1),
                   dict(uv=at['uv'] + 1, out_uv=at['out_uv'] + 3)):
            assert b'2-byte aligned' in refused(_lib, *call(**kw)), kw
        # too many tiles: 2^20 frames of 32,766 x 32,766 outputs (addresses far apart: nothing is dereferenced before a launch)
        far = dict(y=1 << 40, uv=1 << 48, out_y=1 << 54, out_uv=1 << 58, n=1 << 20, oW=32766, oH=32766)
        assert b'too many tiles' in refused(_lib, *call(**far))
        # ... and where only the luma kernel's tiles are too many: chroma has a quarter of the samples in tiles of the same area
        assert b'too many tiles' in refused(_lib, *call(**dict(far, n=1 << 14)))
    for key in ('bounds', 'status'):
        assert b'null' in refused(_lib, *dev(**{key: None}))
    for rect in ((5, 3, 4, 40), (2, 9, 60, 8), (-1, 3, 60, 40), (2, -1, 60, 40), (2, 3, 64, 40), (2, 3, 60, 48)):
        assert b'rectangle' in refused(_lib, *host(rect=rect)), rect
    assert bytes(buf) == bytes(len(buf))                                # nothing was written anywhere


def test_python_refusals_before_the_library():
    """What `ops.crop_resize_p010` and `stabilized_p010_cropped` decide without a device."""
    torch = pytest.importorskip('torch')
    from meshflow_amd import ops
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    y, uv = torch.zeros((2, 4, 8), dtype=torch.uint16), torch.zeros((2, 2, 4, 2), dtype=torch.uint16)
    with pytest.raises(ValueError, match='y must be a CUDA/HIP'):
        ops.crop_resize_p010(y, uv, (0, 0, 7, 3))
    with pytest.raises(ValueError, match='y must be a CUDA/HIP'):
        ops.crop_resize_p010(y.numpy(), uv, (0, 0, 7, 3))
    s = MeshFlowStabilizer(mesh_row_count=2, mesh_col_count=2, device='cpu')
    disp = torch.zeros((2, 3, 3, 2), dtype=torch.float64)
    for bad in ((7, 4), (8, 3), (0, 4), (8, 32768), (8,)):
        with pytest.raises(ValueError, match='output_size'):
            s.stabilized_p010_cropped(y, uv, disp, None, output_size=bad)
    with pytest.raises(ValueError, match='d_y must be a CUDA/HIP'):
        s.stabilized_p010_cropped(y, uv, disp, None, output_size=(8, 4))
    with pytest.raises(ValueError, match='stabilized_p010_cropped'):       # the call that does not crop names the one that does
        s.stabilized_p010(y, uv, disp, None, crop=True)


@pytest.mark.gpu
def test_python_refusals_on_the_device():
    torch = pytest.importorskip('torch')
    import numpy as np
    from meshflow_amd import ops
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    dev = torch.device('cuda:0')
    n, H, W = 2, 16, 24
    rect = (3, 2, 20, 13)
    def full(shape, value, dtype=np.uint16):                            # (made on the host: no torch kernel is asked to handle uint16)
        return torch.from_numpy(np.full(shape, value, dtype)).to(dev)

    y, uv = full((n, H, W), 5), full((n, H // 2, W // 2, 2), 6)
    oy, ouv = full((n, H, W), 0xA5A5), full((n, H // 2, W // 2, 2), 0xA5A5)
    bounds = torch.tensor(rect, dtype=torch.int32, device=dev)

    def no(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            ops.crop_resize_p010(*args, **kw)

    for b in (rect, bounds):
        no('dtype', y.view(torch.int16), uv, b)
        no('dtype', y, uv.view(torch.int16), b)
        no('dtype', full((n, H, W), 5, np.uint8), uv, b)
        no('CUDA/HIP', y, uv.cpu(), b)
        no('contiguous', full((n, H, 2 * W), 5)[..., ::2], uv, b)
        no('contiguous', y, uv[..., 0], b)
        no('shape', y[..., None], uv, b)
        no('shape', y, full((n, H // 2, W // 2), 6), b)
        no('shape', y, full((n, H, W, 2), 6), b)
        no('shape', y, uv[:1], b)
        no('even', full((n, H, W + 1), 5), uv, b)
        no('even', full((n, H - 1, W), 5), uv, b)
        for size in ((23, 16), (24, 15), (0, 16), (24, 32768), (24,), 24):
            no('size', y, uv, b, size=size)
        for bad in ((oy,), (oy, ouv, ouv), oy, (oy, ouv[..., 0]), (oy[:1], ouv), (oy, ouv.view(torch.int16)), (oy.cpu(), ouv), (ouv, oy),
                    (np.zeros((n, H, W), np.uint16), ouv)):
            with pytest.raises(ValueError):
                ops.crop_resize_p010(y, uv, b, out=bad)
        no('shape', y, uv, b, size=(32, 20), out=(oy, ouv))                 # an `out` of the frame's size for another output size
        # what the library refuses comes back as ValueError too: planes that alias
        no('alias', y, uv, b, out=(y, ouv))
        no('alias', y, uv, b, out=(oy, uv))
    no('status', y, uv, rect, status=torch.zeros(1, dtype=torch.int32, device=dev))
    no('status', y, uv, bounds, status=torch.zeros(2, dtype=torch.int32, device=dev))
    no('dtype', y, uv, bounds, status=torch.zeros(1, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        ops.crop_resize_p010(y, uv, torch.zeros(3, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        ops.crop_resize_p010(y, uv, torch.zeros(4, dtype=torch.int64, device=dev))
    for bad in ((5, 3, 4, 10), (-1, 0, 23, 15), (0, 0, 24, 15), (0, 0, 23, 16), (0, 9, 23, 8)):
        no('rectangle', y, uv, bad)
    torch.cuda.synchronize()
    assert (oy.cpu().numpy() == 0xA5A5).all() and (ouv.cpu().numpy() == 0xA5A5).all()
    assert (y.cpu().numpy() == 5).all() and (uv.cpu().numpy() == 6).all()
