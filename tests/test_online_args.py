"""The online smoother's call in the header, the ctypes table and the built library, and every refusal it makes before anything is launched
-- invalid-argument status with the call's name in mf_last_error().  Host addresses throughout: a call that got as far as a launch would not
return MF_ERR_INVALID_ARG.  No GPU."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = 'mf_online_smooth_f64'
N, S, OMEGA, L = 3, 5, 4, 8


def test_library_exports_the_call():
    from meshflow_amd import _lib
    header = open(os.path.join(REPO, 'include', 'meshflow_hip.h')).read()
    assert NAME in _lib.SIGNATURES and len(_lib.SIGNATURES[NAME][1]) == 17 and hasattr(_lib.lib, NAME)
    assert re.search(r'\bint %s\(' % NAME, header)
    block = header[header.index('online path smoothing'):header.index('int %s(' % NAME)]
    for text in ('tests/online_model.py', 'No atomics', 'Asynchronous on `stream`', 'not read when seen is 0', 'lam_newest', 'updated in place',
                 'MF_ERR_INVALID_ARG, nothing launched', 'no fma', 'IEEE division'):
        assert text in block, text
    for name, value in (('MF_ONLINE_MAX_WINDOW', _lib.ONLINE_MAX_WINDOW), ('MF_ONLINE_MAX_OMEGA', _lib.ONLINE_MAX_OMEGA),
                        ('MF_ONLINE_MAX_ITERS', _lib.ONLINE_MAX_ITERS)):
        assert re.search(r'#define %s %d\b' % (name, value), header), name
    assert (_lib.ONLINE_MAX_WINDOW, _lib.ONLINE_MAX_OMEGA, _lib.ONLINE_MAX_ITERS) == (64, 64, 1000)


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
    good = dict(n=N, S=S, omega=OMEGA, L=L, iters=10, beta=1.0, lam_newest=0.95, seen=0, **at)

    def call(**kw):
        a = dict(good, **kw)
        return (vp(a['vel']), vp(a['lam_known']), vp(a['taps']), a['n'], a['S'], a['omega'], a['L'], a['iters'], a['beta'], a['lam_newest'],
                a['seen'], vp(a['c_state']), vp(a['q_state']), vp(a['lam_state']), vp(a['c_out']), vp(a['p_out']), None)

    for kw in (dict(n=0), dict(n=-1), dict(S=0), dict(S=-3)):
        assert b'at least 1' in refused(_lib, *call(**kw)), kw
    for window in (1, 0, -1, 65, 1 << 20):
        assert b'window must be in 2 .. 64' in refused(_lib, *call(L=window)), window
    for omega in (0, -1, 65):
        assert b'omega must be in 1 .. 64' in refused(_lib, *call(omega=omega)), omega
    for iters in (0, -1, 1001):
        assert b'iters must be in 1 .. 1000' in refused(_lib, *call(iters=iters)), iters
    for beta in (-1.0, -1e-300, float('inf'), float('nan')):
        assert b'beta must be finite' in refused(_lib, *call(beta=beta)), beta
    for lam in (-0.5, float('inf'), float('-inf'), float('nan')):
        assert b'lam_newest must be finite' in refused(_lib, *call(lam_newest=lam)), lam
    for seen in (-1, -(1 << 40)):
        assert b'seen must not be negative' in refused(_lib, *call(seen=seen)), seen
    for key in keys:
        assert b'null' in refused(_lib, *call(**{key: None})), key
    for key in keys:
        assert b'aligned' in refused(_lib, *call(**{key: at[key] + (2 if key == 'vel' else 4)})), key
    # an output over an input, over the state, over the other output: first and last byte
    for out in ('c_out', 'p_out'):
        for kw in (dict(vel=at[out] + N * S * 8 - 4), dict(lam_known=at[out] + 8), dict(taps=at[out] - OMEGA * 8 + 8),
                   {out: at['vel'] + N * S * 4 - 4 & ~7}):
            assert b'an output aliases an input' in refused(_lib, *call(**kw)), (out, kw)
        for kw in (dict(c_state=at[out] + N * S * 8 - 8), dict(q_state=at[out] - (L - 1) * S * 8 + 8), dict(lam_state=at[out] + 16)):
            assert b'an output aliases the state' in refused(_lib, *call(**kw)), (out, kw)
    for kw in (dict(p_out=at['c_out']), dict(p_out=at['c_out'] + N * S * 8 - 8), dict(c_out=at['p_out'] + 8)):
        assert b'd_c_out and d_p_out alias' in refused(_lib, *call(**kw)), kw
    # the state is updated in place: it may overlap neither an input nor itself
    for kw in (dict(c_state=at['vel'] + 8), dict(lam_state=at['lam_known'] + 16), dict(q_state=at['taps'])):
        assert b'the state aliases an input' in refused(_lib, *call(**kw)), kw
    for kw in (dict(q_state=at['c_state'] + (L - 1) * S * 8 - 8), dict(lam_state=at['q_state']), dict(lam_state=at['c_state'] + 8)):
        assert b'two of the state arrays alias' in refused(_lib, *call(**kw)), kw
    # the limits themselves are accepted as far as the checks go: the largest window, radius and sweep count next to a refusal that comes last
    assert b'd_c_out and d_p_out alias' in refused(_lib, *call(L=2, omega=64, iters=1000, beta=0.0, lam_newest=0.0, seen=1 << 40,
                                                                p_out=at['c_out']))
    assert bytes(buf) == bytes(len(buf))                                # nothing was written anywhere


def test_margin_rectangle():
    from meshflow_amd import online
    assert online.margin_rectangle(0.08, 1920, 1080) == (153, 86, 1766, 993)          # floor(0.08 * 1919), floor(0.08 * 1079)
    assert online.margin_rectangle(0, 128, 96) == (0, 0, 127, 95)
    assert online.margin_rectangle(0.499, 4, 2) == (1, 0, 2, 1)                        # the smallest rectangle a margin below 0.5 leaves
    for W, H in ((1, 8), (8, 1)):
        with pytest.raises(ValueError, match='leaves fewer than 2 x 2 pixels'):
            online.margin_rectangle(0.08, W, H)
    assert tuple(online.OnlineReport._fields) == ('first', 'd_unstab', 'd_stab', 'rectangle', 'covered', 'lost')


def test_python_refusals_before_the_library():
    torch = pytest.importorskip('torch')
    from meshflow_amd import host, ops
    import numpy as np
    vel, lam = torch.zeros((N, S), dtype=torch.float32), torch.zeros(N, dtype=torch.float64)
    taps = torch.from_numpy(host.online_taps(OMEGA))
    with pytest.raises(ValueError, match='state must be an OnlineState'):
        ops.online_smooth(vel, lam, None, taps, OMEGA, 10, 1.0, 0.95)
    for bad in (dict(S=0, L=8), dict(S=5, L=1), dict(S=5, L=65)):
        with pytest.raises(ValueError, match='OnlineState: S must be at least 1 and L in 2 .. 64'):
            ops.OnlineState(device='cpu', **bad)
    state = ops.OnlineState(S, L, 'cpu')
    assert tuple(state.c.shape) == (L - 1, S) and tuple(state.q.shape) == (L - 1, S) and tuple(state.lam.shape) == (L - 1,) and state.seen == 0
    with pytest.raises(ValueError, match='vel must be a CUDA/HIP'):
        ops.online_smooth(vel, lam, state, taps, OMEGA, 10, 1.0, 0.95)
    with pytest.raises(ValueError, match='vel must be a CUDA/HIP'):
        ops.online_smooth(vel.numpy(), lam, state, taps, OMEGA, 10, 1.0, 0.95)
    with pytest.raises(ValueError, match='omega must be >= 1'):
        host.online_taps(0)
    d = np.arange(1, 11)
    assert host.online_taps(10).tobytes() == np.exp(-np.square((3 / 10) * d)).tobytes()
    assert host.online_taps(10).tobytes() == host.jacobi_band_coefficients(3, 64, 48, 2, None, 10)[0][11:].tobytes()
