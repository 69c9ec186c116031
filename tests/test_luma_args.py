"""The four luma calls in the header, the ctypes table and the built library; every refusal they make before anything is launched --
invalid-argument status with the call's name in mf_last_error() --; and every refusal of `ops.luma`.  The C refusals and what Python decides
before it reaches a device need no GPU; the rest is marked gpu."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# call -> (bytes per source pixel, whether it takes red_first)
CALLS = {'mf_luma_u8c3': (3, True), 'mf_luma_u8c4': (4, True), 'mf_luma_u16c3': (6, True), 'mf_luma_u16': (2, False)}
N, W, H = 2, 7, 5
GUARD = 4096


def test_header_table_and_library_list_the_calls():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    declared = set(re.findall(r'^(?:int|size_t|const char\*)\s+(mf_\w+)\(', header, re.M))
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if len(l.split()) == 3 and l.split()[1] == 'T' and l.split()[-1].startswith('mf_')}
    assert set(CALLS) <= declared
    assert declared == exported == set(_lib.SIGNATURES)
    assert {n for n in declared if 'luma' in n} == set(CALLS)
    for name, (_, order) in CALLS.items():
        assert len(_lib.SIGNATURES[name][1]) == (7 if order else 6), name
        assert re.search(r'^int %s\(const void\* d_src, int n, int W, int H, %suint8_t\* d_dst, void\* stream\);' % (name, 'int red_first, ' if order else ''),
                         header, re.M), name
    block = header[header.index('the luma of a colour or 16-bit clip'):header.index('int mf_luma_u8c3(')]
    for text in ('tests/luma_model.py', '3735', '19235', '9798', '16384) >> 15', '1868', '9617', '4899', '8192) >> 14', '>> 8', 'TRUNCATION',
                 'channel 3 is ignored', 'red_first = 1 swaps', 'MSB-aligned', '1 .. 32,767', 'odd address', 'overlaps the source', '64-bit',
                 'Asynchronous on `stream`'):
        assert text in block, text
    assert _lib.lib.mf_abi_version() == 1
    makefile = open(os.path.join(REPO, 'meshflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS = .*\bluma\.hip\b', makefile, re.M) and re.search(r'^HDRS = .*\bluma_body\.h\b', makefile, re.M)


def test_the_kernel_s_constants_are_the_model_s():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import luma_model as lm
    body = open(os.path.join(REPO, 'meshflow_amd', 'csrc', 'luma_body.h')).read()
    for v in (lm.B8, lm.G8, lm.R8, lm.B16, lm.G16, lm.R16, 1 << (lm.SHIFT8 - 1), 1 << (lm.SHIFT16 - 1)):
        assert re.search(r'\b%du\b' % v, body), v
    assert re.search(r'>> %d;' % lm.SHIFT8, body) and re.search(r'>> %d\) >> 8;' % lm.SHIFT16, body)
    assert 'float' not in body and 'double' not in body
    kernel = open(os.path.join(REPO, 'meshflow_amd', 'csrc', 'luma.hip')).read()
    assert 'float' not in kernel and 'double' not in kernel and '__shared__' not in kernel


@pytest.fixture(scope='module')
def env():
    from meshflow_amd import _lib
    buf = (ctypes.c_uint8 * (3 * GUARD + 64))()
    base = (ctypes.addressof(buf) + 15) & ~15
    return _lib, buf, base


def refused(_lib, name, *args):
    rc = getattr(_lib.lib, name)(*args)
    err = _lib.lib.mf_last_error()
    assert rc == _lib.MF_ERR_INVALID_ARG, (name, args, rc, err)
    assert name.encode() + b':' in err, err
    return err


@pytest.mark.parametrize('name', sorted(CALLS))
def test_c_refusals(env, name):
    """Host addresses throughout, and no GPU needed: a call that got as far as a launch would not return MF_ERR_INVALID_ARG."""
    _lib, buf, base = env
    vp = ctypes.c_void_p
    pixel_bytes, order = CALLS[name]
    src, dst = base, base + 2 * GUARD                       # the source is at most 70 * 6 bytes
    good = dict(src=src, n=N, W=W, H=H, red_first=0, dst=dst)

    def no(**kw):
        a = dict(good, **kw)
        mid = (a['red_first'],) if order else ()
        return refused(_lib, name, vp(a['src']), a['n'], a['W'], a['H'], *mid, vp(a['dst']), None)

    assert b'null' in no(src=None) and b'null' in no(dst=None) and b'null' in no(src=None, dst=None)
    for n in (0, -1, -(1 << 31)):
        assert b'n must be at least 1' in no(n=n), n
    for key in ('W', 'H'):
        for v in (0, -1, 32768, 1 << 20, (1 << 31) - 1, -(1 << 31)):
            assert b'1 .. 32767' in no(**{key: v}), (key, v)
    if order:
        for v in (2, -1, 255, 1 << 30):
            assert b'red_first must be 0 or 1' in no(red_first=v), v
    if pixel_bytes in (2, 6):
        for off in (1, 3, 15):
            assert b'even address' in no(src=src + off), off
    total = N * W * H
    step = 2 if pixel_bytes in (2, 6) else 1                # a uint16 source stays at an even address
    for kw in (dict(dst=src), dict(dst=src + total * pixel_bytes - 1), dict(src=dst + total - step), dict(src=dst), dict(dst=src + 16),
               dict(src=dst - total * pixel_bytes + step)):
        assert b'overlaps' in no(**kw), kw
    # the largest clip the limits admit, on top of itself: the overlap is found without overflow
    assert b'overlaps' in no(n=(1 << 31) - 1, W=32767, H=32767, dst=src + 2)
    assert bytes(buf) == bytes(len(buf))                                # nothing was written anywhere


def test_python_refusals_before_the_library():
    torch = pytest.importorskip('torch')
    from meshflow_amd import ops
    from meshflow_amd.stabilizer import MeshFlowStabilizer

    def no(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            ops.luma(*args, **kw)

    bgr = torch.zeros((N, H, W, 3), dtype=torch.uint8)
    no('already luma', torch.zeros((N, H, W), dtype=torch.uint8))
    no('already luma', torch.zeros((N, H, W), dtype=torch.uint8), out=torch.zeros((N, H, W), dtype=torch.uint8))
    no('must be a CUDA/HIP torch tensor', bgr.numpy())
    no('must be a CUDA/HIP torch tensor', None)
    for bad in (bgr.float(), bgr.to(torch.int16), bgr[..., :2], torch.zeros((N, H, W, 4), dtype=torch.uint16), torch.zeros((H, W), dtype=torch.uint16),
                torch.zeros((N, H, W, 3, 1), dtype=torch.uint8), torch.zeros((N, H, W), dtype=torch.float32), torch.zeros((N, H, W, 1), dtype=torch.uint8)):
        no(r'frames must be \(n, H, W, 3\) uint8 or uint16, \(n, H, W, 4\) uint8 or \(n, H, W\) uint16', bad)
    for shape in ((0, H, W, 3), (N, 0, W, 3), (N, H, 0, 3), (1, 32768, 1, 3), (1, 1, 32768, 3)):
        no('n >= 1 and H, W in 1 .. 32767', torch.zeros(shape, dtype=torch.uint8))
    no('n >= 1 and H, W in 1 .. 32767', torch.zeros((1, 1, 32768), dtype=torch.uint16))
    for v in (2, -1, None, 'yes'):
        no('red_first must be False or True', bgr, red_first=v)
    no('red_first has no meaning', torch.zeros((N, H, W), dtype=torch.uint16), red_first=True)
    # host tensors of the right form: the device is asked for last, and before the library
    for ok in (bgr, torch.zeros((N, H, W, 4), dtype=torch.uint8), torch.zeros((N, H, W, 3), dtype=torch.uint16), torch.zeros((N, H, W), dtype=torch.uint16)):
        no('frames must be a CUDA/HIP torch tensor', ok)
    s = MeshFlowStabilizer(mesh_row_count=4, mesh_col_count=4)
    with pytest.raises(ValueError, match=r'the luma plane of a P010 clip: pass the pair \(d_y, d_uv\)'):
        s.stabilize_scored(torch.zeros((N, H, W), dtype=torch.uint16))
    with pytest.raises(ValueError, match=r'the pair \(d_y, d_uv\)'):
        s.stabilize_scored((bgr,))
    with pytest.raises(ValueError, match='frames must be a CUDA/HIP torch tensor'):
        s.stabilize_scored(bgr)
    with pytest.raises(ValueError, match='frames must be a CUDA/HIP torch tensor'):
        s.estimate_motion(bgr, red_first=True)


@pytest.mark.gpu
def test_python_refusals_on_the_device():
    torch = pytest.importorskip('torch')
    from meshflow_amd import ops
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    dev = torch.device('cuda:0')

    def no(match, *args, **kw):
        with pytest.raises(ValueError, match=match):
            ops.luma(*args, **kw)

    bgr = torch.full((N, H, W, 3), 200, dtype=torch.uint8, device=dev)
    no('already luma', bgr[..., 0].contiguous())
    no('frames must be contiguous', torch.zeros((N, H, W, 6), dtype=torch.uint8, device=dev)[..., ::2])
    no('frames must be contiguous', torch.zeros((N, H, 2 * W, 4), dtype=torch.uint8, device=dev)[:, :, ::2])
    no('frames must be contiguous', torch.zeros((N, H, 2 * W), dtype=torch.uint16, device=dev)[:, :, ::2])
    no('out must be a CUDA/HIP torch tensor', bgr, out=torch.zeros((N, H, W), dtype=torch.uint8))
    no('out must have dtype', bgr, out=torch.zeros((N, H, W), dtype=torch.int8, device=dev))
    no('out must have dtype', bgr, out=torch.zeros((N, H, W), dtype=torch.uint16, device=dev))
    no('out must be contiguous', bgr, out=torch.zeros((N, H, 2 * W), dtype=torch.uint8, device=dev)[:, :, ::2])
    for shape in ((N, H, W, 1), (N, W, H), (N + 1, H, W), (N * H * W,)):
        no(r'out must have shape \(2, 5, 7\)', bgr, out=torch.zeros(shape, dtype=torch.uint8, device=dev))
    # a destination inside the source: the library's own refusal
    flat = torch.zeros(N * H * W * 4, dtype=torch.uint8, device=dev)
    inside = flat[:N * H * W * 3].view(N, H, W, 3)
    for off in (0, 16, N * H * W * 3 - 1):
        no('mf_luma_u8c3: the destination overlaps the source', inside, out=flat[off:off + N * H * W].view(N, H, W))
    out = ops.luma(inside, out=flat[N * H * W * 3:N * H * W * 3 + N * H * W].view(N, H, W))        # right behind it: fine
    assert not out.cpu().numpy().any()
    got = ops.luma(bgr)
    assert got.shape == (N, H, W) and got.dtype == torch.uint8 and got.device == bgr.device and bool((got == 200).all())
    assert bool((bgr == 200).all())
