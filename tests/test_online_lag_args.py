"""The lagged online smoother's call in the header, the ctypes table and the built library, every refusal it makes before anything is
launched -- the plain call's, under its own name, plus `lag` outside 0 .. window - 1 --, and the `lag` checks of `ops` and of the session.
Host addresses throughout: a call that got as far as a launch would not return MF_ERR_INVALID_ARG.  No GPU."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME, PLAIN = 'mf_online_smooth_lag_f64', 'mf_online_smooth_f64'
N, S, OMEGA, L = 3, 5, 4, 8


def test_library_exports_the_call():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 18 and hasattr(_lib.lib, NAME)
    # the plain call's arguments with one c_int more, after `window`
    plain, lagged = _lib.SIGNATURES[PLAIN][1], _lib.SIGNATURES[NAME][1]
    assert lagged[:7] == plain[:7] and lagged[7] is ctypes.c_int and lagged[8:] == plain[7:] and _lib.SIGNATURES[NAME][0] is ctypes.c_int
    assert re.search(r'\bint %s\(' % NAME, header)
    assert header.index('int %s(' % PLAIN) < header.index('online path smoothing with a fixed lag') < header.index('int %s(' % NAME)
    block = header[header.index('online path smoothing with a fixed lag'):header.index('int %s(' % NAME)]
    for text in ('tests/online_lag_model.py', 'No atomics', 'Asynchronous on `stream`', 'written as 0.0', 'no output byte is left undefined',
                 'MF_ERR_INVALID_ARG, nothing launched', 'lag outside 0 .. window - 1', 'does not depend on lag', 'min(lag, seen)'):
        assert text in block, text
    prototype = header[header.index('int %s(' % NAME):]
    prototype = prototype[:prototype.index(';')]
    assert re.search(r'int window, int lag,\s+int iters', prototype) and prototype.count(',') == 17


@pytest.fixture(scope='module')
def env():
    from meshflow_amd import _lib
    buf = (ctypes.c_uint8 * (8 * 4096 + 64))()
    base = (ctypes.addressof(buf) + 15) & ~15
    return _lib, buf, base


def refused(_lib, *args):
    rc = getattr(_lib.lib, NAME)(*args)
    err = _lib.lib.mf_last_error()
    assert rc == _lib.MF_ERR_INVALID_ARG, (args, rc, err)
    assert NAME.encode() + b':' in err, err
    return err


def test_c_refusals(env):
    _lib, buf, base = env
    vp = ctypes.c_void_p
    # 4 KB apart: vel is N * S * 4 = 60 bytes, lam_known 24, taps 32, the state 280 / 280 / 56, the outputs 120 each
    keys = ('vel', 'lam_known', 'taps', 'c_state', 'q_state', 'lam_state', 'c_out', 'p_out')
    at = {k: base + 4096 * i for i, k in enumerate(keys)}
    good = dict(n=N, S=S, omega=OMEGA, L=L, lag=2, iters=10, beta=1.0, lam_newest=0.95, seen=0, **at)

    def call(**kw):
        a = dict(good, **kw)
        return (vp(a['vel']), vp(a['lam_known']), vp(a['taps']), a['n'], a['S'], a['omega'], a['L'], a['lag'], a['iters'], a['beta'],
                a['lam_newest'], a['seen'], vp(a['c_state']), vp(a['q_state']), vp(a['lam_state']), vp(a['c_out']), vp(a['p_out']), None)

    # a call that passes every check but the last one made: `lag`
    for kw in (dict(lag=-1), dict(lag=L), dict(lag=L + 1), dict(lag=1 << 20), dict(lag=-(1 << 31)), dict(L=2, lag=2), dict(L=64, lag=64)):
        assert b'lag must be in 0 .. window - 1' in refused(_lib, *call(**kw)), kw
    # the plain call's refusals, for several lags; a bad lag beside them does not hide them
    for lag in (0, 2, L - 1, -1):
        for kw in (dict(n=0), dict(n=-1), dict(S=0), dict(S=-3)):
            assert b'at least 1' in refused(_lib, *call(lag=lag, **kw)), kw
        for window in (1, 0, -1, 65, 1 << 20):
            assert b'window must be in 2 .. 64' in refused(_lib, *call(L=window, lag=min(lag, 0))), window
        for omega in (0, -1, 65):
            assert b'omega must be in 1 .. 64' in refused(_lib, *call(lag=lag, omega=omega)), omega
        for iters in (0, -1, 1001):
            assert b'iters must be in 1 .. 1000' in refused(_lib, *call(lag=lag, iters=iters)), iters
        for beta in (-1.0, -1e-300, float('inf'), float('nan')):
            assert b'beta must be finite' in refused(_lib, *call(lag=lag, beta=beta)), beta
        for lam in (-0.5, float('inf'), float('-inf'), float('nan')):
            assert b'lam_newest must be finite' in refused(_lib, *call(lag=lag, lam_newest=lam)), lam
        for seen in (-1, -(1 << 40)):
            assert b'seen must not be negative' in refused(_lib, *call(lag=lag, seen=seen)), seen
        for key in keys:
            assert b'null' in refused(_lib, *call(lag=lag, **{key: None})), key
        for key in keys:
            assert b'aligned' in refused(_lib, *call(lag=lag, **{key: at[key] + (2 if key == 'vel' else 4)})), key
    # an output over an input, over the state, over the other output: first and last byte
    for out in ('c_out', 'p_out'):
        for kw in (dict(vel=at[out] + N * S * 8 - 4), dict(lam_known=at[out] + 8), dict(taps=at[out] - OMEGA * 8 + 8),
                   {out: at['vel'] + N * S * 4 - 4 & ~7}):
            assert b'an output aliases an input' in refused(_lib, *call(**kw)), (out, kw)
        for kw in (dict(c_state=at[out] + N * S * 8 - 8), dict(q_state=at[out] - (L - 1) * S * 8 + 8), dict(lam_state=at[out] + 16)):
            assert b'an output aliases the state' in refused(_lib, *call(**kw)), (out, kw)
    for kw in (dict(p_out=at['c_out']), dict(p_out=at['c_out'] + N * S * 8 - 8), dict(c_out=at['p_out'] + 8)):
        assert b'd_c_out and d_p_out alias' in refused(_lib, *call(**kw)), kw
    for kw in (dict(c_state=at['vel'] + 8), dict(lam_state=at['lam_known'] + 16), dict(q_state=at['taps'])):
        assert b'the state aliases an input' in refused(_lib, *call(**kw)), kw
    for kw in (dict(q_state=at['c_state'] + (L - 1) * S * 8 - 8), dict(lam_state=at['q_state']), dict(lam_state=at['c_state'] + 8)):
        assert b'two of the state arrays alias' in refused(_lib, *call(**kw)), kw
    # the limits themselves are accepted as far as the checks go: the largest lag of the smallest and of the largest window
    for kw in (dict(L=2, lag=1), dict(L=64, lag=63, c_state=at['c_state'], q_state=at['c_state']), dict(lag=0)):
        err = refused(_lib, *call(omega=64, iters=1000, beta=0.0, lam_newest=0.0, seen=1 << 40, p_out=at['c_out'], **kw))
        assert b'alias' in err and b'lag' not in err.replace(NAME.encode(), b''), (kw, err)
    assert bytes(buf) == bytes(len(buf))                                # nothing was written anywhere


def test_ops_refuse_a_bad_lag_before_the_library():
    torch = pytest.importorskip('torch')
    from meshflow_amd import host, ops
    vel, lam = torch.zeros((N, S), dtype=torch.float32), torch.zeros(N, dtype=torch.float64)
    taps = torch.from_numpy(host.online_taps(OMEGA))
    state = ops.OnlineState(S, L, 'cpu')
    with pytest.raises(ValueError, match='online_smooth_lag: state must be an OnlineState'):
        ops.online_smooth_lag(vel, lam, None, taps, OMEGA, 10, 1.0, 0.95, 2)
    with pytest.raises(ValueError, match='online_pending: state must be an OnlineState'):
        ops.online_pending(None, 2)
    for lag in (True, False, 2.0, -1, L, None, '2'):
        with pytest.raises(ValueError, match=r'online_smooth_lag: lag must be an int in 0 \.\. window - 1 = 7'):
            ops.online_smooth_lag(vel, lam, state, taps, OMEGA, 10, 1.0, 0.95, lag)
        with pytest.raises(ValueError, match=r'online_pending: lag must be an int in 0 \.\. window - 1 = 7'):
            ops.online_pending(state, lag)
    # a good lag gets as far as the plain call's own checks
    for lag in (0, 2, L - 1):
        with pytest.raises(ValueError, match='vel must be a CUDA/HIP'):
            ops.online_smooth_lag(vel, lam, state, taps, OMEGA, 10, 1.0, 0.95, lag)
    assert state.seen == 0
    # `online_pending` needs no kernel: the last min(lag, seen) rows, as clones
    state.c.copy_(torch.arange((L - 1) * S, dtype=torch.float64).reshape(L - 1, S))
    state.q.copy_(state.c + 0.5)
    for seen, lag, rows in ((0, 3, 0), (2, 3, 2), (3, 3, 3), (100, 3, 3), (100, 0, 0), (100, L - 1, L - 1), (4, L - 1, 4)):
        state.seen = seen
        c, p = ops.online_pending(state, lag)
        assert tuple(c.shape) == tuple(p.shape) == (rows, S)
        assert torch.equal(c, state.c[L - 1 - rows:]) and torch.equal(p, state.q[L - 1 - rows:])
        assert rows == 0 or (c.data_ptr() != state.c[L - 1 - rows:].data_ptr() and p.data_ptr() != state.q[L - 1 - rows:].data_ptr())
    assert state.seen == 4


def test_the_session_refuses_a_bad_lag():
    pytest.importorskip('torch')
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    s = MeshFlowStabilizer(mesh_row_count=4, mesh_col_count=4, temporal_smoothing_radius=4, device='cpu')
    for window in (2, 8, 64):
        for lag in (True, False, 1.0, -1, window, window + 5, None, '1'):
            with pytest.raises(ValueError, match=r'lag must be an int in 0 \.\. window - 1 = %d' % (window - 1)):
                s.online_session(window=window, lag=lag)
    # (a bad window is reported as such, whatever the lag)
    with pytest.raises(ValueError, match='window must be in 2 .. 64'):
        s.online_session(window=1, lag=0)
