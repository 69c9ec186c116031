"""The two scene-cut calls in the header, the ctypes table and the built library; every refusal they make before anything is launched --
invalid-argument status with the call's name in mf_last_error() --; and what Python refuses before it reaches the library.  Host addresses
throughout: a call that got as far as a launch would not return MF_ERR_INVALID_ARG.  No GPU."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGNATURE, DISTANCE = 'mf_frame_signature_u8', 'mf_cut_distance_i32'
N, W, H = 2, 7, 5
GUARD = 4096


def test_library_exports_the_calls():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    for name, nargs in ((SIGNATURE, 6), (DISTANCE, 5)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == nargs and hasattr(_lib.lib, name), name
    assert re.search(r'^int %s\(const uint8_t\* d_luma, int n, int W, int H, int32_t\* d_sig, void\* stream\);' % SIGNATURE, header, re.M)
    assert re.search(r'^int %s\(const int32_t\* d_sig_prev, const int32_t\* d_sig, int n, int32_t\* d_dist, void\* stream\);' % DISTANCE, header, re.M)
    block = header[header.index('scene cuts: a per-frame signature'):header.index('int %s(' % SIGNATURE)]
    for text in ('tests/cuts_model.py', 'integers only', '4 x 4 tiles', 'floor(i H / 4)', 'value >> 4 == b', '[tile_row][tile_col][bin]', 'OVERWRITTEN',
                 'below 2^31', '64-bit', 'any byte', 'where d_sig_prev', 'else 0', 'MF_ERR_INVALID_ARG, nothing launched', '4-byte aligned',
                 'overlaps an input', 'Asynchronous on `stream`'):
        assert text in block, text
    for name, value in (('MF_CUT_COUNTERS', _lib.CUT_COUNTERS), ('MF_CUT_MAX_DIM', _lib.CUT_MAX_DIM)):
        assert re.search(r'#define %s %d\b' % (name, value), header), name
    assert (_lib.CUT_COUNTERS, _lib.CUT_MAX_DIM) == (256, 32767)
    makefile = open(os.path.join(REPO, 'meshflow_amd', 'csrc', 'Makefile')).read()
    assert re.search(r'^SRCS = .*\bcuts\.hip\b', makefile, re.M) and re.search(r'^HDRS = .*\bcuts_body\.h\b', makefile, re.M)


def test_the_kernel_s_constants_are_the_model_s():
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import cuts_model as cm
    body = open(os.path.join(REPO, 'meshflow_amd', 'csrc', 'cuts_body.h')).read()
    assert re.search(r'\bTILES = %d;' % cm.TILES, body) and re.search(r'\bBINS = %d;' % cm.BINS, body)
    kernel = open(os.path.join(REPO, 'meshflow_amd', 'csrc', 'cuts.hip')).read()
    for text in (body, kernel):
        assert 'float' not in text and 'double' not in text and 'asm' not in text


@pytest.fixture(scope='module')
def env():
    from meshflow_amd import _lib
    buf = (ctypes.c_uint8 * (4 * GUARD + 64))()
    base = (ctypes.addressof(buf) + 15) & ~15
    return _lib, buf, base


def refused(_lib, name, *args):
    rc = getattr(_lib.lib, name)(*args)
    err = _lib.lib.mf_last_error()
    assert rc == _lib.MF_ERR_INVALID_ARG, (name, args, rc, err)
    assert name.encode() + b':' in err, err
    return err


def test_signature_refusals(env):
    _lib, buf, base = env
    vp = ctypes.c_void_p
    luma, sig = base, base + GUARD                          # the frames are 70 bytes, the signatures 2048
    good = dict(luma=luma, n=N, W=W, H=H, sig=sig)

    def no(**kw):
        a = dict(good, **kw)
        return refused(_lib, SIGNATURE, vp(a['luma']), a['n'], a['W'], a['H'], vp(a['sig']), None)

    assert b'null' in no(luma=None) and b'null' in no(sig=None) and b'null' in no(luma=None, sig=None)
    for n in (0, -1, -(1 << 31)):
        assert b'n must be at least 1' in no(n=n), n
    for key in ('W', 'H'):
        for v in (0, -1, 32768, 1 << 20, (1 << 31) - 1, -(1 << 31)):
            assert b'1 .. 32767' in no(**{key: v}), (key, v)
    for off in (1, 2, 3):
        assert b'd_sig must be 4-byte aligned' in no(sig=sig + off), off
    total = N * W * H
    for kw in (dict(sig=luma), dict(sig=luma + 68), dict(luma=sig + N * 1024 - 1), dict(luma=sig), dict(luma=sig + 1), dict(sig=luma - N * 1024 + 4)):
        assert b'd_sig overlaps the frames' in no(**kw), kw
    assert total == 70
    # the largest clip the limits admit, on top of its signatures: the overlap is found without overflow
    assert b'overlaps' in no(n=(1 << 31) - 1, W=32767, H=32767, sig=luma + 4)
    assert bytes(buf) == bytes(len(buf))                                # nothing was written anywhere


def test_distance_refusals(env):
    _lib, buf, base = env
    vp = ctypes.c_void_p
    prev, sig, dist = base, base + GUARD, base + 3 * GUARD            # the signatures are N * 1024 bytes, the distances N * 4
    good = dict(prev=prev, sig=sig, n=N, dist=dist)

    def no(**kw):
        a = dict(good, **kw)
        return refused(_lib, DISTANCE, vp(a['prev']), vp(a['sig']), a['n'], vp(a['dist']), None)

    assert b'null' in no(sig=None) and b'null' in no(dist=None) and b'null' in no(prev=None, sig=None)
    for n in (0, -1, -(1 << 31)):
        assert b'n must be at least 1' in no(n=n), n
    for key in ('prev', 'sig', 'dist'):
        for off in (1, 2, 3):
            assert b'4-byte aligned' in no(**{key: good[key] + off}), (key, off)
    for kw in (dict(dist=sig), dict(dist=sig + N * 1024 - 4), dict(sig=dist - N * 1024 + 4), dict(dist=prev), dict(dist=prev + 1020), dict(prev=dist + 4),
               dict(prev=dist - 1020), dict(prev=None, dist=sig + 4)):
        assert b'd_dist overlaps a signature' in no(**kw), kw
    assert b'overlaps' in no(n=(1 << 31) - 1, dist=sig + 8)
    assert bytes(buf) == bytes(len(buf))


def test_python_refusals_before_the_library():
    torch = pytest.importorskip('torch')
    from meshflow_amd import online, ops
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    s = MeshFlowStabilizer(mesh_row_count=4, mesh_col_count=4, temporal_smoothing_radius=2)
    grey = torch.zeros((N, H, W), dtype=torch.uint8)
    for bad in ('split', 'Reset', None, 0, True):
        with pytest.raises(ValueError, match="on_cut must be 'ignore' or 'reset'"):
            s.online_session(on_cut=bad)
    for bad in (-0.01, 1.01, float('nan'), float('inf'), float('-inf'), None, '0.3', True, 2):
        with pytest.raises(ValueError, match=r'cut_threshold must be a finite number in \[0, 1\]'):
            s.online_session(on_cut='reset', cut_threshold=bad)
        with pytest.raises(ValueError, match=r'cut_threshold must be a finite number in \[0, 1\]'):
            s.online_session(cut_threshold=bad)                         # (checked whatever on_cut says)
        with pytest.raises(ValueError, match=r'threshold must be a finite number in \[0, 1\]'):
            s.find_cuts(grey, threshold=bad)
        with pytest.raises(ValueError, match=r'threshold must be a finite number in \[0, 1\]'):
            ops.find_cuts(grey, threshold=bad)
    for ok in (0, 1, 0.0, 1.0, 0.3):
        assert ops.check_cut_threshold(ok) == float(ok)
    assert ops.CUT_THRESHOLD == 0.30
    assert ops.cut_bound(0.30, 128, 96) == 7372 and ops.cut_bound(1.0, 32767, 32767) == 2 * 32767 * 32767 and ops.cut_bound(0.5, 5, 1) == 5
    # the right threshold, frames that are not on a device: refused before the library
    for call in (lambda: ops.frame_signatures(grey), lambda: ops.find_cuts(grey), lambda: ops.frame_signatures(grey.numpy()), lambda: s.find_cuts(grey)):
        with pytest.raises(ValueError, match='must be a CUDA/HIP torch tensor'):
            call()
    with pytest.raises(ValueError, match='d_sig must be a CUDA/HIP torch tensor'):
        ops.cut_distances(torch.zeros((N, 256), dtype=torch.int32))
    with pytest.raises(ValueError, match='red_first must be False or True'):
        s.find_cuts(grey, red_first=2)
    with pytest.raises(ValueError, match=r'the pair \(d_y, d_uv\)'):
        s.find_cuts((grey,))
    with pytest.raises(ValueError, match=r'the luma plane of a P010 clip: pass the pair \(d_y, d_uv\)'):
        s.find_cuts(torch.zeros((N, H, W), dtype=torch.uint16))
    assert tuple(online.OnlineReport._fields) == ('first', 'd_unstab', 'd_stab', 'rectangle', 'covered', 'lost')
