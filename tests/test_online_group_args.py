"""The three group calls (mf_online_smooth_group_f64, mf_path_limit_group_f64, mf_cut_distance_pairs_i32) in the header, the ctypes table and
the built library, every refusal they make before anything is launched -- invalid-argument status with the call's name in mf_last_error()
--, and the Python checks in front of them.  Host addresses throughout: a call that got as far as a launch would not return
MF_ERR_INVALID_ARG.  No GPU."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOOTH, LIMIT, PAIRS = 'mf_online_smooth_group_f64', 'mf_path_limit_group_f64', 'mf_cut_distance_pairs_i32'
K, B, N, S, OMEGA, L = 3, 4, 2, 5, 4, 8


def test_library_exports_the_calls():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    for name, args in ((SMOOTH, 20), (LIMIT, 19), (PAIRS, 5)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == args and hasattr(_lib.lib, name), name
        declaration = re.search(r'\bint %s\(([^)]*)\)' % name, header)
        assert declaration and declaration.group(1).count(',') + 1 == args, name
    block = header[header.index('online path smoothing of a group'):header.index('int %s(' % SMOOTH)]
    for text in ('tests/online_model.py', 'no fma', 'IEEE division', 'DISTINCT', "caller's duty", 'reads nothing of its', 'keeps its state bytes',
                 'touches no memory', 'Two launches', 'No atomics', 'MF_ERR_INVALID_ARG, nothing launched', 'Asynchronous on `stream`'):
        assert text in block, text
    assert re.search(r'#define MF_ONLINE_GROUP_MAX_ROWS %d\b' % _lib.ONLINE_GROUP_MAX_ROWS, header) and _lib.ONLINE_GROUP_MAX_ROWS == 65535


@pytest.fixture(scope='module')
def env():
    from meshflow_amd import _lib
    buf = (ctypes.c_uint8 * (12 * 4096 + 64))()
    base = (ctypes.addressof(buf) + 15) & ~15
    return _lib, buf, base


def refused(_lib, name, *args):
    rc = getattr(_lib.lib, name)(*args)
    err = _lib.lib.mf_last_error()
    assert rc == _lib.MF_ERR_INVALID_ARG, (name, args, rc, err)
    assert name.encode() + b':' in err, err
    return err


def test_smooth_group_refusals(env):
    _lib, buf, base = env
    vp = ctypes.c_void_p
    # 4 KB apart: vel is K N S 4 = 120 bytes, lam_known 48, taps 32, ids 12, seen 24, the stacks B (L - 1) S 8 = 1120 / 1120 / 224, the
    # outputs K N S 8 = 240 each
    keys = ('vel', 'lam_known', 'taps', 'ids', 'seen', 'c_state', 'q_state', 'lam_state', 'c_out', 'p_out')
    at = {k: base + 4096 * i for i, k in enumerate(keys)}
    good = dict(K=K, B=B, n=N, S=S, omega=OMEGA, L=L, iters=10, beta=1.0, lam_newest=0.95, **at)
    rows, stack = K * N * S * 8, B * (L - 1) * S * 8

    def call(**kw):
        a = dict(good, **kw)
        return (vp(a['vel']), vp(a['lam_known']), vp(a['taps']), vp(a['ids']), vp(a['seen']), a['K'], a['B'], a['n'], a['S'], a['omega'], a['L'],
                a['iters'], a['beta'], a['lam_newest'], vp(a['c_state']), vp(a['q_state']), vp(a['lam_state']), vp(a['c_out']), vp(a['p_out']),
                None)

    def no(**kw):
        return refused(_lib, SMOOTH, *call(**kw))

    # the single call's refusals
    for kw in (dict(n=0), dict(n=-1), dict(S=0), dict(S=-3)):
        assert b'at least 1' in no(**kw), kw
    for window in (1, 0, -1, 65, 1 << 20):
        assert b'window must be in 2 .. 64' in no(L=window), window
    for omega in (0, -1, 65):
        assert b'omega must be in 1 .. 64' in no(omega=omega), omega
    for iters in (0, -1, 1001):
        assert b'iters must be in 1 .. 1000' in no(iters=iters), iters
    for beta in (-1.0, -1e-300, float('inf'), float('nan')):
        assert b'beta must be finite' in no(beta=beta), beta
    for lam in (-0.5, float('inf'), float('-inf'), float('nan')):
        assert b'lam_newest must be finite' in no(lam_newest=lam), lam
    # the group's own
    for kw in (dict(K=0), dict(K=-1), dict(B=0), dict(B=-2), dict(K=B + 1), dict(K=2, B=1), dict(K=65536, B=65536)):
        assert b'1 <= K <= B' in no(**kw), kw
    for key in keys:                                                    # d_ids and d_seen among them
        assert b'null' in no(**{key: None}), key
    for key in keys:
        assert b'aligned' in no(**{key: at[key] + (2 if key in ('vel', 'ids') else 4)}), key
    # the overlap rules on the K N rows and the whole stacks: first and last byte
    for out in ('c_out', 'p_out'):
        for kw in (dict(vel=at[out] + rows - 4), dict(lam_known=at[out] + 8), dict(taps=at[out] - OMEGA * 8 + 8), dict(ids=at[out] + rows - 4),
                   dict(seen=at[out] - K * 8 + 8), {out: at['vel'] + K * N * S * 4 - 4 & ~7}):
            assert b'an output aliases an input' in no(**kw), (out, kw)
        for kw in (dict(c_state=at[out] + rows - 8), dict(q_state=at[out] - stack + 8), dict(lam_state=at[out] + 16)):
            assert b'an output aliases the state' in no(**kw), (out, kw)
    # ... the last stream's slices count: a single state's extent would let these through
    assert b'an output aliases the state' in no(c_out=at['c_state'] + stack - 8)
    assert b'an output aliases the state' in no(p_out=at['lam_state'] + B * (L - 1) * 8 - 8)
    for kw in (dict(p_out=at['c_out']), dict(p_out=at['c_out'] + rows - 8), dict(c_out=at['p_out'] + 8)):
        assert b'd_c_out and d_p_out alias' in no(**kw), kw
    for kw in (dict(c_state=at['vel'] + 8), dict(lam_state=at['lam_known'] + 16), dict(q_state=at['taps']), dict(ids=at['q_state'] + stack - 4),
               dict(seen=at['lam_state'] + B * (L - 1) * 8 - 8)):
        assert b'the state aliases an input' in no(**kw), kw
    for kw in (dict(q_state=at['c_state'] + stack - 8), dict(lam_state=at['q_state']), dict(lam_state=at['c_state'] + 8)):
        assert b'two of the state arrays alias' in no(**kw), kw
    # the limits themselves pass the checks: K = B, the largest window, radius and sweep count next to a refusal that comes last
    assert b'd_c_out and d_p_out alias' in no(K=B, L=2, omega=64, iters=1000, beta=0.0, lam_newest=0.0, p_out=at['c_out'])
    assert bytes(buf) == bytes(len(buf))                                # nothing was written anywhere


def test_path_limit_group_refusals(env):
    _lib, buf, base = env
    vp = ctypes.c_void_p
    W, H, R, C = 128, 96, 2, 3
    keys = ('unstab', 'stab', 'k_prev', 'k_raw', 'k', 'out')             # the paths are K (R+1)(C+1) 2 8 = 576 bytes
    at = {k: base + 4096 * i for i, k in enumerate(keys)}
    good = dict(K=K, W=W, H=H, R=R, C=C, rect=(10, 7, 117, 88), guard=2.0, steps=32, rise=2, **at)
    path = K * (R + 1) * (C + 1) * 2 * 8

    def no(**kw):
        a = dict(good, **kw)
        return refused(_lib, LIMIT, vp(a['unstab']), vp(a['stab']), a['K'], a['W'], a['H'], a['R'], a['C'], *a['rect'], a['guard'], a['steps'],
                       a['rise'], vp(a['k_prev']), vp(a['k_raw']), vp(a['k']), vp(a['out']), None)

    for rows in (0, -1):
        assert b'at least 1' in no(K=rows), rows
    for kw in (dict(R=0), dict(C=0), dict(R=500, C=13)):
        assert b'boundary vertices' in no(**kw), kw
    for kw in (dict(W=1), dict(H=1)):
        assert b'W and H must be at least 2' in no(**kw), kw
    for rect in ((-1, 7, 117, 88), (10, 7, 128, 88), (10, 7, 117, 96), (60, 7, 50, 88)):
        assert b'is not inside' in no(rect=rect), rect
    for steps in (0, 65):
        assert b'steps must be in 1 .. 64' in no(steps=steps), steps
    for rise in (0, 33):
        assert b'rise must be in 1 .. steps' in no(rise=rise), rise
    for guard in (-1.0, float('inf'), float('nan')):
        assert b'guard must be finite' in no(guard=guard), guard
    for key in keys:                                                    # d_k_prev among them: a group has a word per row
        assert b'null' in no(**{key: None}), key
    for key in keys:
        assert b'aligned' in no(**{key: at[key] + (2 if key.startswith('k') else 4)}), key
    for kw in (dict(out=at['unstab'] + path - 8), dict(k=at['stab']), dict(k_raw=at['k_prev'] + (K - 1) * 4), dict(k=at['k_prev'] + (K - 1) * 4),
               dict(k_prev=at['out'] + path - 4)):                          # (the LAST carried word: the single call has one)
        assert b'an output aliases an input' in no(**kw), kw
    for kw in (dict(k=at['k_raw'] + (K - 1) * 4), dict(out=at['k']), dict(k_raw=at['out'] + path - 4)):
        assert b'two of the outputs alias' in no(**kw), kw
    assert bytes(buf) == bytes(len(buf))


def test_cut_distance_pairs_refusals(env):
    _lib, buf, base = env
    vp = ctypes.c_void_p
    at = dict(prev=base, sig=base + 4096, dist=base + 8192)              # the stacks are K 256 4 = 3072 bytes

    def no(n=K, **kw):
        a = dict(at, **kw)
        return refused(_lib, PAIRS, vp(a['prev']), vp(a['sig']), n, vp(a['dist']), None)

    for key in at:
        assert b'null' in no(**{key: None}), key
    for n in (0, -1):
        assert b'n must be at least 1' in no(n=n), n
    for key in at:
        assert b'4-byte aligned' in no(**{key: at[key] + 2}), key
    for kw in (dict(dist=at['sig'] + K * 1024 - 4), dict(dist=at['prev'] + K * 1024 - 4), dict(dist=at['prev']), dict(sig=at['dist'] - K * 1024 + 4)):
        assert b'd_dist overlaps a signature' in no(**kw), kw
    assert bytes(buf) == bytes(len(buf))


def test_python_refusals_before_the_library():
    torch = pytest.importorskip('torch')
    from meshflow_amd import host, ops
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    for bad in (dict(B=0, S=5, L=8), dict(B=2, S=0, L=8), dict(B=2, S=5, L=1), dict(B=2, S=5, L=65)):
        with pytest.raises(ValueError, match='OnlineGroupState: B and S must be at least 1 and L in 2 .. 64'):
            ops.OnlineGroupState(device='cpu', **bad)
    state = ops.OnlineGroupState(B, S, L, 'cpu')
    assert tuple(state.c.shape) == tuple(state.q.shape) == (B, L - 1, S) and tuple(state.lam.shape) == (B, L - 1) and state.seen == [0] * B
    state.seen = [3, 1, 4, 1]
    state.reset(2)
    assert state.seen == [3, 1, 0, 1]
    state.reset()
    assert state.seen == [0] * B
    for stream in (True, B, -1, 1.0):
        with pytest.raises(ValueError, match='OnlineGroupState.reset: stream must'):
            state.reset(stream)

    vel, lam = torch.zeros((K, N, S), dtype=torch.float32), torch.zeros((K, N), dtype=torch.float64)
    taps = torch.from_numpy(host.online_taps(OMEGA))
    with pytest.raises(ValueError, match='state must be an OnlineGroupState'):
        ops.online_smooth_group(vel, lam, ops.OnlineState(S, L, 'cpu'), [0, 1, 2], taps, OMEGA, 10, 1.0, 0.95)
    # the ids are checked on the host, before a tensor is looked at: the library cannot see them
    for streams, why in (([0, 1, 1], 'distinct'), ([2, 0, 2], 'distinct'), ([0, 1, B], r'lie in 0 \.\. 3'), ([-1, 0, 1], r'lie in 0 \.\. 3'),
                         ([0, True, 2], 'sequence of ints'), ([False, 1, 2], 'sequence of ints'), ([0, 1.0, 2], 'sequence of ints'),
                         ([], 'sequence of ints'), (3, 'sequence of stream indices')):
        with pytest.raises(ValueError, match='online_smooth_group: streams must .*' + why):
            ops.online_smooth_group(vel, lam, state, streams, taps, OMEGA, 10, 1.0, 0.95)
    with pytest.raises(ValueError, match='vel must be a CUDA/HIP'):
        ops.online_smooth_group(vel, lam, state, [3, 0, 2], taps, OMEGA, 10, 1.0, 0.95)
    assert state.seen == [0] * B                                        # a refused call advances nothing
    with pytest.raises(ValueError, match='unstab must be a CUDA/HIP'):
        ops.path_limit_group(torch.zeros((K, 24)), torch.zeros((K, 24)), 128, 96, 2, 3, (10, 7, 117, 88), k_prev=torch.zeros(K, dtype=torch.int32))
    with pytest.raises(ValueError, match='rise must be an integer in 1 .. steps'):
        ops.path_limit_group(None, None, 128, 96, 2, 3, (10, 7, 117, 88), rise=0)
    with pytest.raises(ValueError, match='d_sig must be a CUDA/HIP'):
        ops.cut_distance_pairs(torch.zeros((K, 256), dtype=torch.int32), torch.zeros((K, 256), dtype=torch.int32))

    s = MeshFlowStabilizer(mesh_row_count=4, mesh_col_count=4, temporal_smoothing_radius=4, device='cpu')
    for streams in (0, -1, True, 2.0, None):
        with pytest.raises(ValueError, match='streams must be an int >= 1'):
            s.online_group(streams)
    for lag in (1, 3, True):
        with pytest.raises(ValueError, match='a group takes lag=0 only .* per stream'):
            s.online_group(2, window=8, lag=lag)
    with pytest.raises(ValueError, match="a group takes on_lost='hold' only .* must not stop the others"):
        s.online_group(2, on_lost='raise')
