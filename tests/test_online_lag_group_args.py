"""The two calls of a lagged group (mf_online_smooth_group_lag_f64, mf_ring_exchange_u8) in the header, the ctypes table and the built
library, every refusal they make before anything is launched -- invalid-argument status with the call's name in mf_last_error() --, the
Python checks in front of them and of `MeshFlowStabilizer.online_lag_group`, and tests/ring_model.py against a restatement with a list of
frames per stream.  Host addresses throughout: a call that got as far as a launch would not return MF_ERR_INVALID_ARG.  No GPU."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ring_model  # noqa: E402

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMOOTH, RING = 'mf_online_smooth_group_lag_f64', 'mf_ring_exchange_u8'
K, B, N, S, OMEGA, L, LAG = 3, 4, 2, 5, 4, 8, 3


def test_library_exports_the_calls():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    for name, args in ((SMOOTH, 21), (RING, 9)):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == args and hasattr(_lib.lib, name), name
        declaration = re.search(r'\bint %s\(([^)]*)\)' % name, header)
        assert declaration and declaration.group(1).count(',') + 1 == args, name
    block = header[header.index('online path smoothing of a group with a fixed lag'):header.index('int %s(' % SMOOTH)]
    for text in ('tests/online_lag_model.py', 'does not depend on lag', 'touches no memory', "caller's duty", 'lag outside 0 .. window - 1',
                 'MF_ERR_INVALID_ARG, nothing launched', 'Asynchronous on `stream`'):
        assert text in block, text
    block = header[header.index('the pixels a lagged group owes'):header.index('int %s(' % RING)]
    for text in ('tests/ring_model.py', 'touches no memory', 'DISTINCT', 'no barriers and no atomics', 'nothing past a frame',
                 'MF_ERR_INVALID_ARG, nothing launched', 'Asynchronous on `stream`'):
        assert text in block, text
    # the group smoother's lagged twin takes the group's arguments and `lag` behind `window`, as the single lagged call does
    plain = re.search(r'\bint mf_online_smooth_group_f64\(([^)]*)\)', header).group(1)
    lagged = re.search(r'\bint %s\(([^)]*)\)' % SMOOTH, header).group(1)
    squeeze = lambda text: re.sub(r'\s+', ' ', text)                    # noqa: E731
    assert squeeze(lagged) == squeeze(plain).replace('int window,', 'int window, int lag,')


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


def test_smooth_group_lag_refusals(env):
    _lib, buf, base = env
    vp = ctypes.c_void_p
    keys = ('vel', 'lam_known', 'taps', 'ids', 'seen', 'c_state', 'q_state', 'lam_state', 'c_out', 'p_out')
    at = {k: base + 4096 * i for i, k in enumerate(keys)}
    good = dict(K=K, B=B, n=N, S=S, omega=OMEGA, L=L, lag=LAG, iters=10, beta=1.0, lam_newest=0.95, **at)
    rows, stack = K * N * S * 8, B * (L - 1) * S * 8

    def no(**kw):
        a = dict(good, **kw)
        return refused(_lib, SMOOTH, vp(a['vel']), vp(a['lam_known']), vp(a['taps']), vp(a['ids']), vp(a['seen']), a['K'], a['B'], a['n'], a['S'],
                       a['omega'], a['L'], a['lag'], a['iters'], a['beta'], a['lam_newest'], vp(a['c_state']), vp(a['q_state']),
                       vp(a['lam_state']), vp(a['c_out']), vp(a['p_out']), None)

    # the lag: outside 0 .. window - 1, at both windows' edges
    for kw in (dict(lag=-1), dict(lag=L), dict(lag=L + 5), dict(L=2, lag=2), dict(L=64, lag=64, S=1), dict(lag=1 << 30)):
        assert b'lag must be in 0 .. window - 1' in no(**kw), kw
    # the group call's refusals, under this call's name
    for kw in (dict(n=0), dict(n=-1), dict(S=0), dict(S=-3)):
        assert b'at least 1' in no(**kw), kw
    for window in (1, 0, -1, 65, 1 << 20):
        assert b'window must be in 2 .. 64' in no(L=window, lag=0), window
    for omega in (0, -1, 65):
        assert b'omega must be in 1 .. 64' in no(omega=omega), omega
    for iters in (0, -1, 1001):
        assert b'iters must be in 1 .. 1000' in no(iters=iters), iters
    for beta in (-1.0, -1e-300, float('inf'), float('nan')):
        assert b'beta must be finite' in no(beta=beta), beta
    for lam in (-0.5, float('inf'), float('-inf'), float('nan')):
        assert b'lam_newest must be finite' in no(lam_newest=lam), lam
    for kw in (dict(K=0), dict(K=-1), dict(B=0), dict(B=-2), dict(K=B + 1), dict(K=2, B=1), dict(K=65536, B=65536)):
        assert b'1 <= K <= B' in no(**kw), kw
    for key in keys:
        assert b'null' in no(**{key: None}), key
    for key in keys:
        assert b'aligned' in no(**{key: at[key] + (2 if key in ('vel', 'ids') else 4)}), key
    for out in ('c_out', 'p_out'):
        for kw in (dict(vel=at[out] + rows - 4), dict(lam_known=at[out] + 8), dict(taps=at[out] - OMEGA * 8 + 8), dict(ids=at[out] + rows - 4),
                   dict(seen=at[out] - K * 8 + 8), {out: at['vel'] + K * N * S * 4 - 4 & ~7}):
            assert b'an output aliases an input' in no(**kw), (out, kw)
        for kw in (dict(c_state=at[out] + rows - 8), dict(q_state=at[out] - stack + 8), dict(lam_state=at[out] + 16)):
            assert b'an output aliases the state' in no(**kw), (out, kw)
    assert b'an output aliases the state' in no(c_out=at['c_state'] + stack - 8)
    assert b'an output aliases the state' in no(p_out=at['lam_state'] + B * (L - 1) * 8 - 8)
    for kw in (dict(p_out=at['c_out']), dict(p_out=at['c_out'] + rows - 8), dict(c_out=at['p_out'] + 8)):
        assert b'd_c_out and d_p_out alias' in no(**kw), kw
    for kw in (dict(c_state=at['vel'] + 8), dict(lam_state=at['lam_known'] + 16), dict(q_state=at['taps']), dict(ids=at['q_state'] + stack - 4),
               dict(seen=at['lam_state'] + B * (L - 1) * 8 - 8)):
        assert b'the state aliases an input' in no(**kw), kw
    for kw in (dict(q_state=at['c_state'] + stack - 8), dict(lam_state=at['q_state']), dict(lam_state=at['c_state'] + 8)):
        assert b'two of the state arrays alias' in no(**kw), kw
    # the limits themselves pass: the largest lag of the window next to a refusal that comes before it
    assert b'd_c_out and d_p_out alias' in no(lag=L - 1, p_out=at['c_out'])
    assert bytes(buf) == bytes(len(buf))                                # nothing was written anywhere


def test_ring_exchange_refusals(env):
    _lib, buf, base = env
    vp = ctypes.c_void_p
    frame, lag = 48, 3                                                   # the ring is B lag N = 576 bytes, new and out K N = 144
    at = dict(ring=base, new=base + 4096, out=base + 8192, rows=base + 12288)
    good = dict(K=K, B=B, lag=lag, N=frame, **at)

    def no(**kw):
        a = dict(good, **kw)
        return refused(_lib, RING, vp(a['ring']), vp(a['new']), vp(a['out']), vp(a['rows']), a['K'], a['B'], a['lag'], a['N'], None)

    for kw in (dict(K=0), dict(K=-1), dict(B=0), dict(B=-4), dict(lag=0), dict(lag=-1), dict(N=0), dict(N=-16), dict(K=65536, B=65536)):
        assert b'must be at least 1 and K <= 65535' in no(**kw), kw
    for kw in (dict(N=_lib.RING_MAX_FRAME_BYTES + 1), dict(N=1 << 62), dict(B=1 << 30, lag=1 << 30, N=1 << 20)):
        assert b'N must not exceed' in no(**kw), kw
    for key in at:
        assert b'null' in no(**{key: None}), key
    for off in (1, 2, 3):
        assert b'd_rows must be 4-byte aligned' in no(rows=at['rows'] + off), off
    ring_bytes, row_bytes = B * lag * frame, K * frame
    for kw in (dict(out=at['ring']), dict(out=at['ring'] + ring_bytes - 1), dict(out=at['ring'] - row_bytes + 1), dict(out=at['new']),
               dict(out=at['new'] + row_bytes - 1), dict(out=at['new'] - row_bytes + 1), dict(ring=at['out'] + row_bytes - 1)):
        assert b'd_out overlaps d_ring or d_new' in no(**kw), kw
    for kw in (dict(new=at['ring'] + ring_bytes - 1), dict(new=at['ring'] - row_bytes + 1)):
        assert b'd_new overlaps d_ring' in no(**kw), kw
    # neighbours that only touch are no overlap: the refusal that remains is the one asked for
    assert b'null' in no(out=at['ring'] + ring_bytes, new=at['ring'] + ring_bytes + row_bytes, rows=None)
    assert bytes(buf) == bytes(len(buf))


def test_python_refusals_before_the_library():
    torch = pytest.importorskip('torch')
    from meshflow_amd import host, ops
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    state = ops.OnlineGroupState(B, S, L, 'cpu')
    state.seen = [3, 1, 4, 1]
    vel, lam = torch.zeros((K, N, S), dtype=torch.float32), torch.zeros((K, N), dtype=torch.float64)
    taps = torch.from_numpy(host.online_taps(OMEGA))
    with pytest.raises(ValueError, match='online_smooth_group_lag: state must be an OnlineGroupState'):
        ops.online_smooth_group_lag(vel, lam, ops.OnlineState(S, L, 'cpu'), [0, 1, 2], taps, OMEGA, 10, 1.0, 0.95, LAG)
    for streams, why in (([0, 1, 1], 'distinct'), ([0, 1, B], r'lie in 0 \.\. 3'), ([0, True, 2], 'sequence of ints'), ([], 'sequence of ints')):
        with pytest.raises(ValueError, match='online_smooth_group_lag: streams must .*' + why):
            ops.online_smooth_group_lag(vel, lam, state, streams, taps, OMEGA, 10, 1.0, 0.95, LAG)
    for lag in (-1, L, True, 2.0, None):
        with pytest.raises(ValueError, match=r'online_smooth_group_lag: lag must be an int in 0 \.\. window - 1 = 7'):
            ops.online_smooth_group_lag(vel, lam, state, [0, 1, 2], taps, OMEGA, 10, 1.0, 0.95, lag)
    with pytest.raises(ValueError, match='vel must be a CUDA/HIP'):
        ops.online_smooth_group_lag(vel, lam, state, [3, 0, 2], taps, OMEGA, 10, 1.0, 0.95, LAG)
    assert state.seen == [3, 1, 4, 1]                                    # a refused call advances nothing

    with pytest.raises(ValueError, match='online_pending_group: state must be an OnlineGroupState'):
        ops.online_pending_group(ops.OnlineState(S, L, 'cpu'), [0], LAG)
    with pytest.raises(ValueError, match='online_pending_group: lag must be an int'):
        ops.online_pending_group(state, [0], L)
    with pytest.raises(ValueError, match='online_pending_group: streams must be distinct'):
        ops.online_pending_group(state, [1, 1], LAG)
    # no kernel: it runs wherever the state lives; stream b gives its last min(lag, seen) rows, oldest first
    state.c[:] = torch.arange(B * (L - 1) * S, dtype=torch.float64).reshape(B, L - 1, S)
    state.q[:] = -state.c
    pending = ops.online_pending_group(state, [2, 1], LAG)
    assert [tuple(c.shape) for c, _ in pending] == [(3, S), (1, S)]
    assert torch.equal(pending[0][0], state.c[2, L - 4:]) and torch.equal(pending[0][1], state.q[2, L - 4:])
    assert torch.equal(pending[1][0], state.c[1, L - 2:]) and pending[1][0].data_ptr() != state.c[1, L - 2:].data_ptr()

    ring, new = torch.zeros((B, LAG, 6, 8), dtype=torch.uint8), torch.zeros((K, 6, 8), dtype=torch.uint8)
    rows, M = ring_model.tick_rows([0, 1, 2], [0, 0, 0, 0], LAG)
    with pytest.raises(ValueError, match='ring_exchange: ring must be a CUDA/HIP'):
        ops.ring_exchange(ring, new, rows, M)
    # shapes and dtypes are compared before the device is looked at
    for bad_ring, bad_new in ((ring, new[:, :, :4].contiguous()), (ring, new[:, :3].contiguous()), (ring, new.to(torch.int16)),
                              (ring.to(torch.uint16), new), (ring[0], new), (ring, new[0]), (ring, new[None])):
        with pytest.raises(ValueError, match='ring_exchange: ring must be .* same dtype and trailing shape'):
            ops.ring_exchange(bad_ring, bad_new, rows, M)
    with pytest.raises(ValueError, match='ring_exchange: ring and new must be torch tensors'):
        ops.ring_exchange(ring.numpy(), new, rows, M)

    s = MeshFlowStabilizer(mesh_row_count=4, mesh_col_count=4, temporal_smoothing_radius=4, device='cpu')
    for streams in (0, -1, True, 2.0, None):
        with pytest.raises(ValueError, match='streams must be an int >= 1'):
            s.online_lag_group(streams, 1, window=8)
    with pytest.raises(ValueError, match=r'a lagged group takes lag in 1 \.\. window - 1 \(got 0\): online_group'):
        s.online_lag_group(2, 0, window=8)
    for lag in (True, False, 8, -1, 2.0, None):
        with pytest.raises(ValueError, match=r'lag must be an int in 0 \.\. window - 1 = 7'):
            s.online_lag_group(2, lag, window=8)
    with pytest.raises(ValueError, match="a group takes on_lost='hold' only .* must not stop the others"):
        s.online_lag_group(2, 1, window=8, on_lost='raise')
    # `online_group` goes on refusing a lag, and says where the look-ahead is
    with pytest.raises(ValueError, match=r'a group takes lag=0 only \(got 3\): online_lag_group\(streams, lag\) .* per stream'):
        s.online_group(2, window=8, lag=3)


def test_the_model_hands_out_each_streams_frame_from_lag_ticks_of_its_own_earlier():
    streams, lag, ticks, shape = 3, 3, 12, (2, 5)
    rng = np.random.default_rng(9)
    ring = rng.integers(0, 256, (streams, lag) + shape).astype(np.uint8)        # whatever the memory held: nothing of it may come out
    garbage = ring.copy()
    pushed = {b: [] for b in range(streams)}                                    # the restatement: every frame a stream was pushed, in order
    handed = {b: [] for b in range(streams)}
    seen = [0] * streams
    schedule = [[0, 1, 2], [2, 0], [1], [0, 1, 2], [2], [1, 0], [0, 2, 1], [0], [2, 1], [1, 2, 0], [0, 1], [2, 0, 1]]
    assert len(schedule) == ticks and {len(ids) for ids in schedule} == {1, 2, 3}
    for tick, ids in enumerate(schedule):
        new = rng.integers(0, 256, (len(ids),) + shape).astype(np.uint8)
        rows, M = ring_model.tick_rows(ids, seen, lag)
        before, kept = ring.copy(), new.copy()
        ring, out = ring_model.exchange(ring, new, rows, M)
        assert out.shape == (M,) + shape and np.array_equal(new, kept)
        j = 0
        for r, b in enumerate(ids):
            pushed[b].append(new[r])
            if len(pushed[b]) > lag:                                            # the frame from `lag` ticks OF ITS OWN earlier: sat-out ticks do not count
                assert rows[r, 2] == j and np.array_equal(out[j], pushed[b][-1 - lag]), (tick, b)
                handed[b].append(out[j])
                j += 1
            else:
                assert rows[r, 2] == -1, (tick, b)
            seen[b] += 1
        assert j == M
        # only the pushed streams' slots changed
        touched = np.zeros(ring.shape[:2], dtype=bool)
        touched[rows[:, 0], rows[:, 1]] = True
        assert np.array_equal(ring[~touched], before[~touched])
    for b in range(streams):
        assert len(handed[b]) == len(pushed[b]) - lag > 0
        assert all(np.array_equal(a, w) for a, w in zip(handed[b], pushed[b]))
        # what a stream still owes sits in its slots: its last `lag` frames
        for t in range(len(pushed[b]) - lag, len(pushed[b])):
            assert np.array_equal(ring[b, t % lag], pushed[b][t])
    assert not any(np.array_equal(o, g) for b in range(streams) for o in handed[b] for g in garbage.reshape((-1,) + shape))
