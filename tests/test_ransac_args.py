"""The outlier step's calls in the header, the ctypes table and the built library; every refusal they make before anything is launched --
invalid-argument status with the call's name in mf_last_error() --; the workspace size; and every refusal of `ops.ransac_inliers`,
`ops.gather_inliers` and the `outliers=` keyword.  The C refusals and what Python decides before it reaches a device need no GPU; the rest
is marked gpu."""
import ctypes
import os
import re

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CALLS = {'mf_ransac_workspace_bytes': 3, 'mf_ransac_inliers_f32': 16, 'mf_track_gather_f64': 16}
N, S, MAX, W, H, ROWS, COLS = 2, 4, 16, 64, 48, 2, 2
SLOTS, FEATURES = N * S, N * S * MAX


def test_library_exports_the_calls():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    for name, nargs in CALLS.items():
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        assert hasattr(_lib.lib, name), name
        assert re.search(r'\b(?:int|size_t) %s\(' % name, header), name
    block = header[header.index('between the two: outlier rejection'):header.index('size_t mf_ransac_workspace_bytes(')]
    for text in ('mfs.py:564-579, 614, 626; 521, 578', 'bit for bit tests/ransac_model.py', '{status, k, inliers, iterations run}',
                 'sub-frame order outer, point order inner', 'mf_vertex_motion_f64', 'No atomics', 'asynchronous on `stream`', '65,535'):
        assert text in block, text
    for name, value in (('MF_RANSAC_OK', _lib.RANSAC_OK), ('MF_RANSAC_TOO_FEW', _lib.RANSAC_TOO_FEW),
                        ('MF_RANSAC_NO_CONSENSUS', _lib.RANSAC_NO_CONSENSUS), ('MF_RANSAC_MAX_ITERS', _lib.RANSAC_MAX_ITERS),
                        ('MF_TRACK_PAIR_TOO_FEW', _lib.TRACK_PAIR_TOO_FEW)):
        assert re.search(r'#define %s %d\b' % (name, value), header), name


def test_workspace_size():
    from meshflow_amd import _lib
    ws = _lib.lib.mf_ransac_workspace_bytes
    assert ws(32, 16, 1024) == 16                                        # every sub-frame fits the staged capacity: nothing but a valid pointer
    assert ws(1, 1, 1025) == 1025 * 16 and ws(3, 6, 1089) == 3 * 6 * 1089 * 16          # 16 bytes per candidate beyond it
    assert ws(2047, 16, 16384) == 2047 * 16 * 16384 * 16
    for bad in ((0, 4, 16), (2, 0, 16), (2, 4, 0), (2, 4, 16385), (-1, 4, 16), (2048, 16, 16), (1, 32768, 16)):
        assert ws(*bad) == 0, bad


@pytest.fixture(scope='module')
def env():
    from meshflow_amd import _lib
    buf = (ctypes.c_uint8 * (16 * 4096 + 64))()
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
    # 4 KB apart: points and moved are FEATURES * 8 = 1 KB, early and late FEATURES * 16 = 2 KB
    at = {k: base + 4096 * i for i, k in enumerate(('points', 'moved', 'counts', 'found', 'inlier', 'info', 'work', 'early', 'late', 'offsets',
                                                    'status'))}
    good = dict(n=N, S=S, max=MAX, min=4, threshold=3.0, confidence=0.995, iters=2000, seed=0, W=W, H=H, rows=ROWS, cols=COLS, **at)

    def ransac(**kw):
        a = dict(good, **kw)
        return ('mf_ransac_inliers_f32', vp(a['points']), vp(a['moved']), vp(a['counts']), vp(a['found']), a['n'], a['S'], a['max'], a['min'],
                a['threshold'], a['confidence'], a['iters'], a['seed'], vp(a['inlier']), vp(a['info']), vp(a['work']), None)

    def gather(**kw):
        a = dict(good, **kw)
        return ('mf_track_gather_f64', vp(a['points']), vp(a['moved']), vp(a['inlier']), vp(a['info']), a['n'], a['W'], a['H'], a['rows'], a['cols'],
                a['max'], a['min'], vp(a['early']), vp(a['late']), vp(a['offsets']), vp(a['status']), None)

    for call, pointers in ((ransac, ('points', 'moved', 'counts', 'found', 'inlier', 'info', 'work')),
                           (gather, ('points', 'moved', 'inlier', 'info', 'early', 'late', 'offsets', 'status'))):
        for key in pointers:
            assert b'null' in refused(_lib, *call(**{key: None})), key
        for m in (0, -3, 16385, 1 << 20):
            assert b'max_per_subframe' in refused(_lib, *call(max=m)), m
        for kw in (dict(n=0), dict(n=-2), dict(n=8192)):
            assert b'too many' in refused(_lib, *call(**kw)), kw
        for m in (0, -1):
            assert b'min_features' in refused(_lib, *call(min=m)), m
        assert b'aligned' in refused(_lib, *call(points=at['points'] + 4))
        assert b'aligned' in refused(_lib, *call(moved=at['moved'] + 4))
        assert b'aligned' in refused(_lib, *call(info=at['info'] + 2))
    for kw in (dict(S=0), dict(S=-1), dict(n=2048, S=16), dict(n=1, S=32768)):
        assert b'too many' in refused(_lib, *ransac(**kw)), kw
    for t in (0.0, -3.0, float('inf'), float('nan')):
        assert b'threshold' in refused(_lib, *ransac(threshold=t)), t
    for c in (0.0, 1.0, -0.5, 1.5, float('nan')):
        assert b'confidence' in refused(_lib, *ransac(confidence=c)), c
    for i in (0, -1, 65537, 1 << 30):
        assert b'max_iters' in refused(_lib, *ransac(iters=i)), i
    assert b'aligned' in refused(_lib, *ransac(counts=at['counts'] + 2))
    assert b'aligned' in refused(_lib, *ransac(work=at['work'] + 8))
    for kw in (dict(inlier=at['points'] + 64), dict(info=at['moved'] + FEATURES * 8 - 4), dict(work=at['found']), dict(inlier=at['counts']),
               dict(info=at['found'] + 4)):
        assert b'alias' in refused(_lib, *ransac(**kw)), kw
    for kw in (dict(info=at['inlier'] + FEATURES - 4), dict(inlier=at['info'] + 8), dict(work=at['info']), dict(work=at['inlier'] + 16)):
        assert b'alias' in refused(_lib, *ransac(**kw)), kw
    # the tracker's own limits on the geometry
    for kw in (dict(W=0), dict(H=0), dict(W=32768)):
        assert b'32,767' in refused(_lib, *gather(**kw)), kw
    for kw in (dict(rows=0), dict(cols=0), dict(rows=49), dict(cols=65)):
        assert b'sub_rows' in refused(_lib, *gather(**kw)), kw
    assert b'below the minimum' in refused(_lib, *gather(W=7, cols=3))
    assert b'too many' in refused(_lib, *gather(n=2048, rows=4, cols=4))
    assert b'aligned' in refused(_lib, *gather(early=at['early'] + 4))
    assert b'aligned' in refused(_lib, *gather(offsets=at['offsets'] + 2))
    assert b'aligned' in refused(_lib, *gather(status=at['status'] + 1))
    for kw in (dict(early=at['points'] + 8), dict(late=at['moved']), dict(offsets=at['inlier'] + FEATURES - 4), dict(status=at['info']),
               dict(late=at['early'] + 16), dict(status=at['offsets'] + 4 * N), dict(offsets=at['early'] + FEATURES * 16 - 4)):
        assert b'alias' in refused(_lib, *gather(**kw)), kw
    assert bytes(buf) == bytes(len(buf))                                # nothing was written anywhere


def test_python_refusals_before_the_library():
    torch = pytest.importorskip('torch')
    from meshflow_amd import ops, tracker
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    points = torch.zeros((N, S, MAX, 2))
    counts, found = torch.zeros((N, S), dtype=torch.int32), torch.zeros((N, S, MAX), dtype=torch.uint8)
    with pytest.raises(ValueError, match='points must be a CUDA/HIP'):
        ops.ransac_inliers(points, counts, points, found)
    with pytest.raises(ValueError, match='points must be a CUDA/HIP'):
        ops.ransac_inliers(points.numpy(), counts, points, found)
    with pytest.raises(ValueError, match='points must be a CUDA/HIP'):
        ops.gather_inliers(points, points, found, torch.zeros((N, S, 4), dtype=torch.int32), W, H, ROWS, COLS, 4)
    for bad in ('gpu', 'Host', None, 1, ''):
        with pytest.raises(ValueError, match="outliers must be 'host' or 'device'"):
            tracker.DeviceTracker(2, 2, 4, outliers=bad)
        with pytest.raises(ValueError, match="outliers must be 'host' or 'device'"):
            MeshFlowStabilizer(mesh_row_count=4, mesh_col_count=4).device_tracker(outliers=bad)
        with pytest.raises(ValueError, match="outliers must be 'host' or 'device'"):
            MeshFlowStabilizer(mesh_row_count=4, mesh_col_count=4).estimate_motion(torch.zeros((3, 48, 64), dtype=torch.uint8), outliers=bad)
    assert tracker.DeviceTracker(2, 2, 4).outliers == 'host' and tracker.DeviceTracker(2, 2, 4, outliers='device').outliers == 'device'
    assert tracker.finish_packed(np.zeros((0, 2)), np.zeros((0, 2))) == (None, None, None)


@pytest.mark.gpu
def test_python_refusals_on_the_device():
    torch = pytest.importorskip('torch')
    from meshflow_amd import ops
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    dev = torch.device('cuda:0')
    points = torch.full((N, S, MAX, 2), 5.0, dtype=torch.float32, device=dev)
    moved = points.clone()
    counts = torch.zeros((N, S), dtype=torch.int32, device=dev)
    found = torch.zeros((N, S, MAX), dtype=torch.uint8, device=dev)
    inlier = torch.zeros((N, S, MAX), dtype=torch.uint8, device=dev)
    info = torch.zeros((N, S, 4), dtype=torch.int32, device=dev)

    def no(match, fn, *args, **kw):
        with pytest.raises(ValueError, match=match):
            fn(*args, **kw)

    r, g = ops.ransac_inliers, ops.gather_inliers
    no('dtype', r, points.double(), counts, moved, found)
    no('dtype', r, points, counts.long(), moved, found)
    no('dtype', r, points, counts, moved.half(), found)
    no('dtype', r, points, counts, moved, found.bool())
    no('points must have shape', r, points[0], counts, moved[0], found)
    no('points must have shape', r, points[..., :1].contiguous(), counts, moved[..., :1].contiguous(), found)
    no('moved must have the shape', r, points, counts, moved[:1], found)
    no('counts must have shape', r, points, counts[:1], moved, found)
    no('found must have shape', r, points, counts, moved, found[:, :, :8].contiguous())
    no('contiguous', r, torch.zeros((N, S, MAX, 4), dtype=torch.float32, device=dev)[..., ::2], counts, moved, found)
    no('CUDA/HIP', r, points, counts.cpu(), moved, found)
    no('min_features', r, points, counts, moved, found, 0)
    for t in (0.0, -1.0, float('inf'), float('nan')):
        no('threshold', r, points, counts, moved, found, threshold=t)
    for c in (0.0, 1.0, float('nan')):
        no('confidence', r, points, counts, moved, found, confidence=c)
    for i in (0, 65537):
        no('max_iters', r, points, counts, moved, found, max_iters=i)
    for seed in (-1, 1 << 32):
        no('seed', r, points, counts, moved, found, seed=seed)
    no('max_per_subframe', r, torch.zeros((1, 1, 16385, 2), dtype=torch.float32, device=dev), counts[:1, :1].contiguous(),
       torch.zeros((1, 1, 16385, 2), dtype=torch.float32, device=dev), torch.zeros((1, 1, 16385), dtype=torch.uint8, device=dev))
    no('too many', r, torch.zeros((2048, 16, 1, 2), dtype=torch.float32, device=dev), torch.zeros((2048, 16), dtype=torch.int32, device=dev),
       torch.zeros((2048, 16, 1, 2), dtype=torch.float32, device=dev), torch.zeros((2048, 16, 1), dtype=torch.uint8, device=dev))
    no('dtype', g, points, moved, inlier.int(), info, W, H, ROWS, COLS, 4)
    no('dtype', g, points, moved, inlier, info.long(), W, H, ROWS, COLS, 4)
    no('inlier must have shape', g, points, moved, inlier[:1], info, W, H, ROWS, COLS, 4)
    no('info must have shape', g, points, moved, inlier, info[:, :, :3].contiguous(), W, H, ROWS, COLS, 4)
    no('sub-frames', g, points, moved, inlier, info, W, H, 1, 1, 4)
    no('sub_rows', g, points, moved, inlier, info, W, H, 0, COLS, 4)
    no('min_features', g, points, moved, inlier, info, W, H, ROWS, COLS, 0)
    no('below the minimum', g, points[:, :3].contiguous(), moved[:, :3].contiguous(), inlier[:, :3].contiguous(), info[:, :3].contiguous(), 7, H, 1, 3, 4)
    torch.cuda.synchronize()
    assert (points.cpu().numpy() == 5).all() and not inlier.cpu().numpy().any() and not info.cpu().numpy().any()
