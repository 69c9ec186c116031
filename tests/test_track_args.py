"""The tracker's calls in the header, the ctypes table and the built library; every refusal they make before anything is launched --
invalid-argument status with the call's name in mf_last_error() --; the workspace size; and every refusal of `ops.fast_corners` and
`ops.lk_track`.  The C refusals and what Python decides before it reaches a device need no GPU; the rest is marked gpu."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {'mf_track_workspace_bytes': 6, 'mf_fast_corners_u8': 13, 'mf_lk_track_u8': 14}
N, W, H, ROWS, COLS, MAX = 2, 64, 48, 2, 2, 16
FRAMES = N * W * H


def test_library_exports_the_calls():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    for name, nargs in CALLS.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(_lib.lib, name), name
        assert re.search(r'\b(?:int|size_t) %s\(' % name, header), name
    block = header[header.index('the tracker in front of it'):header.index('size_t mf_track_workspace_bytes(')]
    for text in ('mfs.py:492-516, 581-629', 'one-channel uint8', 'EACH SUB-FRAME IS AN IMAGE OF ITS OWN', 'MF_TRACK_MIN_SUBFRAME', 'MF_TRACK_OVERFLOW',
                 'MF_TRACK_MAX_PER_SUBFRAME', 'TRUE number of corners', 'row-major order', 'left outer, top\n * inner'):
        assert text in block, text
    for name, value in (('MF_TRACK_MIN_SUBFRAME', _lib.TRACK_MIN_SUBFRAME), ('MF_TRACK_MAX_PER_SUBFRAME', _lib.TRACK_MAX_PER_SUBFRAME),
                        ('MF_TRACK_OVERFLOW', _lib.TRACK_OVERFLOW)):
        assert re.search(r'#define %s %d\b' % (name, value), header), name
    assert _lib.lib.mf_abi_version() == 1


def test_header_library_and_ctypes_table_list_the_same_calls():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    declared = set(re.findall(r'^(?:int|size_t|const char\*)\s+(mf_\w+)\(', header, re.M))
    nm = subprocess.run(['nm', '-D', '--defined-only', _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {l.split()[-1] for l in nm.splitlines() if len(l.split()) == 3 and l.split()[1] == 'T' and l.split()[-1].startswith('mf_')}
    assert set(CALLS) <= declared
    assert declared == exported == set(_lib.SIGNATURES)


def test_workspace_size():
    from meshflow_amd import _lib
    ws = _lib.lib.mf_track_workspace_bytes
    # one 64 x 48 frame as one sub-frame: the corner mask is 48 rows of 16 bytes; pyramid levels 1-3 of both stacks are 32 x 24, 16 x 12, 8 x 6
    assert ws(1, 64, 48, 1, 1, 8) == max(48 * 16, 2 * 32 * 24 + 2 * 16 * 12 + 2 * 8 * 6)
    # 1080p as 4 x 4 sub-frames of 480 x 270: levels 240 x 135, 120 x 68, 60 x 34 (each rounded up to 16 bytes per level) against the mask
    levels = sum((2 * 3 * 16 * w * h + 15) // 16 * 16 for w, h in ((240, 135), (120, 68), (60, 34)))
    assert ws(3, 1920, 1080, 4, 4, 1024) == max(levels, 3 * 16 * 270 * 120)
    assert ws(3, 1920, 1080, 4, 4, 1024) % 16 == 0
    assert ws(5, 61, 37, 2, 2, 1) > 0
    for bad in ((0, 64, 48, 1, 1, 8), (1, 0, 48, 1, 1, 8), (1, 64, 32768, 1, 1, 8), (1, 64, 48, 0, 1, 8), (1, 64, 48, 1, 65, 8),
                (1, 64, 48, 1, 1, 0), (1, 64, 48, 1, 1, 16385), (1, 7, 48, 1, 3, 8), (2048, 64, 48, 4, 4, 8)):
        assert ws(*bad) == 0, bad


@pytest.fixture(scope='module')
def env():
    from meshflow_amd import _lib
    buf = (ctypes.c_uint8 * (2 * FRAMES + 8192 + 64))()
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
    out = base + 2 * FRAMES
    at = dict(early=base, late=base + FRAMES, points=out, counts=out + 2048, status=out + 2304, moved=out + 4096, found=out + 6144, work=out + 7168)
    good = dict(n=N, W=W, H=H, rows=ROWS, cols=COLS, max=MAX, threshold=10, **at)

    def fast(**kw):
        a = dict(good, **kw)
        return ('mf_fast_corners_u8', vp(a['early']), a['n'], a['W'], a['H'], a['rows'], a['cols'], a['max'], a['threshold'], vp(a['points']),
                vp(a['counts']), vp(a['status']), vp(a['work']), None)

    def lk(**kw):
        a = dict(good, **kw)
        return ('mf_lk_track_u8', vp(a['early']), vp(a['late']), a['n'], a['W'], a['H'], a['rows'], a['cols'], a['max'], vp(a['points']),
                vp(a['counts']), vp(a['moved']), vp(a['found']), vp(a['work']), None)

    for call, pointers in ((fast, ('early', 'points', 'counts', 'status', 'work')), (lk, ('early', 'late', 'points', 'counts', 'moved', 'found', 'work'))):
        for key in pointers:
            assert b'null' in refused(_lib, *call(**{key: None})), key
        for kw in (dict(W=0), dict(H=0), dict(W=-64), dict(W=32768), dict(H=40000)):
            assert b'32,767' in refused(_lib, *call(**kw)), kw
        for kw in (dict(rows=0), dict(cols=0), dict(rows=-1), dict(rows=49), dict(cols=65)):
            assert b'sub_rows' in refused(_lib, *call(**kw)), kw
        # ceil(7 / 3) = 3: sub-frames of 3, 3 and 1 pixels; ceil(9 / 4) = 3 rows of 3 are fine, ceil(10 / 3) = 4: 4, 4 and 2 are fine, 4, 4, 1 of 9 / 3 are not
        for kw in (dict(W=7, cols=3), dict(H=7, rows=3), dict(W=13, cols=4), dict(H=1, rows=1), dict(W=1, cols=1)):
            assert b'below the minimum' in refused(_lib, *call(**kw)), kw
        for m in (0, -3, 16385, 1 << 20):
            assert b'max_per_subframe' in refused(_lib, *call(max=m)), m
        for kw in (dict(n=0), dict(n=-2), dict(n=8192), dict(n=2048, rows=4, cols=4)):
            assert b'too many' in refused(_lib, *call(**kw)), kw
        assert b'aligned' in refused(_lib, *call(points=at['points'] + 4))
        assert b'aligned' in refused(_lib, *call(counts=at['counts'] + 2))
    for t in (0, -1, 255, 1000):
        assert b'threshold' in refused(_lib, *fast(threshold=t)), t
    assert b'aligned' in refused(_lib, *fast(status=at['status'] + 1))
    assert b'aligned' in refused(_lib, *lk(moved=at['moved'] + 4))
    for kw in (dict(points=at['early'] + 64), dict(counts=at['early'] + FRAMES - 4), dict(status=at['early']), dict(work=at['early'] + 1024)):
        assert b'alias' in refused(_lib, *fast(**kw)), kw
    for kw in (dict(moved=at['early'] + 8), dict(found=at['late'] + FRAMES - 1), dict(work=at['late']), dict(moved=at['late'] + 64)):
        assert b'alias' in refused(_lib, *lk(**kw)), kw
    assert bytes(buf) == bytes(len(buf))                                # nothing was written anywhere


def test_python_refusals_before_the_library():
    torch = pytest.importorskip('torch')
    from meshflow_amd import ops
    grey = torch.zeros((2, 48, 64), dtype=torch.uint8)
    with pytest.raises(ValueError, match='grey must be a CUDA/HIP'):
        ops.fast_corners(grey, 2, 2)
    with pytest.raises(ValueError, match='grey must be a CUDA/HIP'):
        ops.fast_corners(grey.numpy(), 2, 2)
    with pytest.raises(ValueError, match='early must be a CUDA/HIP'):
        ops.lk_track(grey, grey, torch.zeros((2, 4, 8, 2)), torch.zeros((2, 4), dtype=torch.int32), 2, 2)
    assert ops.track_subframe_grid(61, 37, 2, 2) == (31, 19, 2, 2)
    assert ops.track_subframe_grid(9, 9, 4, 4) == (3, 3, 3, 3)
    for rows, cols in ((0, 1), (1, 0), (38, 1), (1, 62)):
        with pytest.raises(ValueError, match='sub_rows'):
            ops.track_subframe_grid(61, 37, rows, cols)


@pytest.mark.gpu
def test_python_refusals_on_the_device():
    torch = pytest.importorskip('torch')
    from meshflow_amd import ops
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    dev = torch.device('cuda:0')
    grey = torch.full((2, 48, 64), 7, dtype=torch.uint8, device=dev)
    points = torch.zeros((2, 4, 8, 2), dtype=torch.float32, device=dev)
    counts = torch.zeros((2, 4), dtype=torch.int32, device=dev)

    def no(match, fn, *args, **kw):
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)

    no('dtype', ops.fast_corners, grey.to(torch.int8), 2, 2)
    no('dtype', ops.fast_corners, grey.to(torch.float32), 2, 2)
    no('shape', ops.fast_corners, grey[0], 2, 2)
    no('shape', ops.fast_corners, grey[..., None], 2, 2)
    no('contiguous', ops.fast_corners, torch.zeros((2, 48, 128), dtype=torch.uint8, device=dev)[..., ::2], 2, 2)
    no('sub_rows', ops.fast_corners, grey, 0, 2)
    no('sub_rows', ops.fast_corners, grey, 2, 65)
    no('below the minimum', ops.fast_corners, grey[:, :, :7].contiguous(), 1, 3)
    for m in (0, 16385):
        no('max_per_subframe', ops.fast_corners, grey, 2, 2, m)
    no('threshold', ops.fast_corners, grey, 2, 2, 8, 0)
    no('threshold', ops.fast_corners, grey, 2, 2, 8, 255)
    no('too many', ops.fast_corners, torch.zeros((2048, 16, 16), dtype=torch.uint8, device=dev), 4, 4)
    no('same shape', ops.lk_track, grey, grey[:1], points, counts, 2, 2)
    no('same shape', ops.lk_track, grey, grey[:, :40].contiguous(), points, counts, 2, 2)
    no('dtype', ops.lk_track, grey, grey.to(torch.int16), points, counts, 2, 2)
    no('dtype', ops.lk_track, grey, grey, points.double(), counts, 2, 2)
    no('dtype', ops.lk_track, grey, grey, points, counts.long(), 2, 2)
    no('shape', ops.lk_track, grey[0], grey[0], points, counts, 2, 2)
    no('contiguous', ops.lk_track, grey, grey, torch.zeros((2, 4, 8, 4), dtype=torch.float32, device=dev)[..., ::2], counts, 2, 2)
    no('points must have shape', ops.lk_track, grey, grey, points[:, :3].contiguous(), counts, 2, 2)
    no('points must have shape', ops.lk_track, grey, grey, points[..., 0].contiguous(), counts, 2, 2)
    no('points must have shape', ops.lk_track, grey, grey, points, counts, 1, 1)
    no('counts must have shape', ops.lk_track, grey, grey, points, counts[:1], 2, 2)
    no('CUDA/HIP', ops.lk_track, grey, grey.cpu(), points, counts, 2, 2)
    no('CUDA/HIP', ops.lk_track, grey, grey, points.cpu(), counts, 2, 2)
    no('below the minimum', ops.lk_track, grey[:, :, :7].contiguous(), grey[:, :, :7].contiguous(),
       torch.zeros((2, 3, 8, 2), dtype=torch.float32, device=dev), torch.zeros((2, 3), dtype=torch.int32, device=dev), 1, 3)
    torch.cuda.synchronize()
    assert (grey.cpu().numpy() == 7).all() and not points.cpu().numpy().any()
