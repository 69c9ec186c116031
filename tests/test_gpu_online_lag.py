"""`ops.online_smooth_lag` and `ops.online_pending` (mf_online_smooth_lag_f64, csrc/online_smooth.hip) against tests/online_lag_model.py,
bit for bit in what is handed out and in all three state tensors, where the lagged store can go wrong: the ring wrap of a lane's age, windows
that are still filling, the oldest lane (lag = L - 1), frames that entered with an earlier call, and lag 0."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import online_lag_model as olm  # noqa: E402
import online_model as om  # noqa: E402
from test_gpu_online import dev, inputs, same  # noqa: E402,F401

pytestmark = pytest.mark.gpu

_MODEL = {}


def model_run(n, S, seed, L, omega, iters, beta, lag, lam_newest=0.95):
    """One block through the model, once per case: (c, p, pending c, pending p, state).  Never written to."""
    key = (n, S, seed, L, omega, iters, beta, lag, lam_newest)
    if key not in _MODEL:
        vel, lam = inputs(n, S, seed)
        state = om.State(S, L)
        c, p = olm.online_smooth_lag(vel, lam, state, om.taps_for(omega), omega, iters, beta, lam_newest, lag)
        _MODEL[key] = (c, p) + olm.pending(state, lag) + (state,)
    return _MODEL[key]


def device_run(dev, vel, lam, blocks, L, omega, iters, beta, lag, lam_newest=0.95):
    import torch
    from meshflow_amd import host, ops
    state, at, c, p = ops.OnlineState(vel.shape[1], L, dev), 0, [], []
    taps = torch.from_numpy(host.online_taps(omega)).to(dev)
    d_vel, d_lam = torch.from_numpy(vel).to(dev), torch.from_numpy(lam).to(dev)
    for b in blocks:
        seen = state.seen
        ci, pi = ops.online_smooth_lag(d_vel[at:at + b], d_lam[at:at + b], state, taps, omega, iters, beta, lam_newest, lag)
        assert tuple(ci.shape) == tuple(pi.shape) == (max(0, seen + b - lag) - max(0, seen - lag), vel.shape[1]) and state.seen == seen + b
        c.append(ci)
        p.append(pi)
        at += b
    pc, pp = ops.online_pending(state, lag)
    return torch.cat(c).cpu().numpy(), torch.cat(p).cpu().numpy(), pc.cpu().numpy(), pp.cpu().numpy(), state


def check(dev, n, S, L, omega, iters, beta, lag, seed, blocks=None):
    vel, lam = inputs(n, S, seed)
    got = device_run(dev, vel, lam, blocks or [n], L, omega, iters, beta, lag)
    want = model_run(n, S, seed, L, omega, iters, beta, lag)
    for g, w, what in zip(got[:4], want[:4], ('c', 'p', 'pending c', 'pending p')):
        same(g, w, (what, lag, blocks))
    assert want[0].shape[0] == max(0, n - lag) and want[2].shape[0] == min(lag, n)
    for name in ('c', 'q', 'lam'):
        same(getattr(got[4], name).cpu().numpy(), getattr(want[4], name), ('state.' + name, lag, blocks))
    assert got[4].seen == want[4].seen == n


def test_the_smallest_window(dev):
    check(dev, 7, 3, 2, 1, 10, 1.0, 1, seed=5)
    check(dev, 7, 3, 2, 3, 4, 0.0, 1, seed=6, blocks=[1, 1, 2, 3])


@pytest.mark.parametrize('lag', [2, 4])
@pytest.mark.parametrize('blocks', [[30], [1] * 30, [1, 3, 4, 22]], ids=['one', 'ones', 'mixed'])
def test_window_5(dev, lag, blocks):
    """L = 5, omega = 4; lag 4 is the oldest lane.  The first calls have seen < lag: rows are dropped, and with blocks of one frame the
    frame handed out always entered with an earlier call."""
    check(dev, 30, 3, 5, 4, 6, 1.0, lag, seed=12, blocks=blocks)


def test_the_largest_window_and_lag(dev):
    check(dev, 70, 3, 64, 64, 3, 1.0, 63, seed=13)
    check(dev, 70, 130, 64, 64, 3, 1.0, 63, seed=14, blocks=[63, 1, 1, 5])          # nothing, then the first frame, then across the wrap


def test_a_block_shorter_than_the_lag_hands_out_nothing(dev):
    check(dev, 3, 130, 40, 10, 10, 1.0, 5, seed=15)
    check(dev, 45, 130, 40, 10, 10, 1.0, 5, seed=16, blocks=[2, 3, 1, 39])


@pytest.mark.parametrize('S,L,omega', [(3, 5, 4), (130, 16, 20), (1, 64, 10)])
def test_lag_0_is_online_smooth(dev, S, L, omega):
    import torch
    from meshflow_amd import host, ops
    n = 2 * L + 3
    vel, lam = inputs(n, S, 17)
    taps = torch.from_numpy(host.online_taps(omega)).to(dev)
    d_vel, d_lam = torch.from_numpy(vel).to(dev), torch.from_numpy(lam).to(dev)
    plain, lagged = ops.OnlineState(S, L, dev), ops.OnlineState(S, L, dev)
    for lo, hi in ((0, 1), (1, L), (L, n)):
        c0, p0 = ops.online_smooth(d_vel[lo:hi], d_lam[lo:hi], plain, taps, omega, 5, 1.0, 0.95)
        c1, p1 = ops.online_smooth_lag(d_vel[lo:hi], d_lam[lo:hi], lagged, taps, omega, 5, 1.0, 0.95, 0)
        same(c1.cpu().numpy(), c0.cpu().numpy(), 'c')
        same(p1.cpu().numpy(), p0.cpu().numpy(), 'p')
    for name in ('c', 'q', 'lam'):
        same(getattr(lagged, name).cpu().numpy(), getattr(plain, name).cpu().numpy(), 'state.' + name)
    pc, pp = ops.online_pending(lagged, 0)
    assert tuple(pc.shape) == tuple(pp.shape) == (0, S)


@pytest.mark.parametrize('lag', [1, 7, 15])
def test_the_state_is_the_plain_calls(dev, lag):
    import torch
    from meshflow_amd import host, ops
    n, S, L, omega = 37, 130, 16, 10
    vel, lam = inputs(n, S, 18)
    taps = torch.from_numpy(host.online_taps(omega)).to(dev)
    d_vel, d_lam = torch.from_numpy(vel).to(dev), torch.from_numpy(lam).to(dev)
    plain, lagged = ops.OnlineState(S, L, dev), ops.OnlineState(S, L, dev)
    for lo, hi in ((0, 5), (5, 6), (6, n)):
        ops.online_smooth(d_vel[lo:hi], d_lam[lo:hi], plain, taps, omega, 5, 1.0, 0.95)
        ops.online_smooth_lag(d_vel[lo:hi], d_lam[lo:hi], lagged, taps, omega, 5, 1.0, 0.95, lag)
        for name in ('c', 'q', 'lam'):
            same(getattr(lagged, name).cpu().numpy(), getattr(plain, name).cpu().numpy(), ('state.' + name, hi))
        assert lagged.seen == plain.seen == hi


def test_non_finite_values_stay_in_their_series(dev):
    n, S, L, omega, lag = 30, 130, 8, 4, 3
    vel, lam = inputs(n, S, 33)
    wc, wp, wpc, wpp, wstate = model_run(n, S, 33, L, omega, 5, 1.0, lag)
    bad = vel.copy()
    bad[4, 17] = np.nan
    bad[9, 64] = np.inf
    c, p, pc, pp, state = device_run(dev, bad, lam, [11, 19], L, omega, 5, 1.0, lag)
    clean = np.ones(S, dtype=bool)
    clean[[17, 64]] = False
    for got, want in ((c, wc), (p, wp), (pc, wpc), (pp, wpp), (state.c.cpu().numpy(), wstate.c), (state.q.cpu().numpy(), wstate.q)):
        same(np.ascontiguousarray(got[:, clean]), np.ascontiguousarray(want[:, clean]), 'the other series')
    # row t is frame t: C_t is non-finite from the bad frame on; x_t is taken from window t + lag, which holds the bad frame -- within
    # reach of frame t's taps, lag <= omega -- from t = bad - lag on, and not before
    assert np.isnan(c[4:, 17]).all() and np.isfinite(c[:4, 17]).all() and np.isinf(c[9:, 64]).all() and np.isfinite(c[:9, 64]).all()
    assert np.isnan(p[4 - lag:, 17]).all() and np.isfinite(p[:4 - lag, 17]).all()
    assert not np.isfinite(p[9 - lag:, 64]).any() and np.isfinite(p[:9 - lag, 64]).all()
    assert not np.isfinite(pp[:, 17]).any() and not np.isfinite(pp[:, 64]).any()


def test_rows_of_frames_that_do_not_exist_are_zero_and_nothing_else_is_written(dev):
    """The raw C call into a poisoned arena: the first lag - seen rows of both outputs are 0.0, the rest the model's, the guards intact."""
    import torch
    from meshflow_amd import _lib, host, ops
    n, S, L, omega, lag, guard = 11, 7, 6, 3, 4, 64
    vel, lam = inputs(n, S, 41)
    wc, wp, _, _, wstate = model_run(n, S, 41, L, omega, 4, 1.0, lag)
    taps = torch.from_numpy(host.online_taps(omega)).to(dev)
    d_vel, d_lam = torch.from_numpy(vel).to(dev), torch.from_numpy(lam).to(dev)
    ptr = ops._ptr
    for blocks in ([n], [1, 2, 8], [3, 8]):
        sizes = {'sc': (L - 1) * S, 'sq': (L - 1) * S, 'sl': L - 1}
        sizes.update({f'{k}{i}': b * S for i, b in enumerate(blocks) for k in 'cp'})
        total = sum(v + 2 * guard for v in sizes.values())
        arena = torch.full((total,), -777.0, dtype=torch.float64, device=dev)
        views, inside, at = {}, np.zeros(total, dtype=bool), 0
        for k, v in sizes.items():
            views[k] = arena[at + guard:at + guard + v]
            inside[at + guard:at + guard + v] = True
            at += v + 2 * guard
        for k in ('sc', 'sq', 'sl'):
            views[k].zero_()
        seen = 0
        for i, b in enumerate(blocks):
            _lib.check(_lib.lib.mf_online_smooth_lag_f64(ptr(d_vel[seen:]), ptr(d_lam[seen:]), ptr(taps), b, S, omega, L, lag, 4, 1.0, 0.95, seen,
                                                         ptr(views['sc']), ptr(views['sq']), ptr(views['sl']), ptr(views[f'c{i}']),
                                                         ptr(views[f'p{i}']), ops._stream()))
            seen += b
        got = arena.cpu().numpy()
        assert (got[~inside] == -777.0).all()
        c = np.concatenate([views[f'c{i}'].cpu().numpy().reshape(b, S) for i, b in enumerate(blocks)])
        p = np.concatenate([views[f'p{i}'].cpu().numpy().reshape(b, S) for i, b in enumerate(blocks)])
        zeros = np.zeros((lag, S))
        same(c[:lag], zeros, ('c of no frame', blocks))                  # (+0.0, bit for bit)
        same(p[:lag], zeros, ('p of no frame', blocks))
        same(c[lag:], wc, ('c', blocks))
        same(p[lag:], wp, ('p', blocks))
        same(views['sc'].cpu().numpy().reshape(L - 1, S), wstate.c, 'state.c')
        same(views['sq'].cpu().numpy().reshape(L - 1, S), wstate.q, 'state.q')
        same(views['sl'].cpu().numpy(), wstate.lam, 'state.lam')


def test_a_lag_outside_the_window_launches_nothing(dev):
    import torch
    from meshflow_amd import host, ops
    S, L, omega = 3, 5, 4
    vel, lam = inputs(4, S, 2)
    state = ops.OnlineState(S, L, dev)
    taps = torch.from_numpy(host.online_taps(omega)).to(dev)
    for lag in (-1, L, True, 2.0):
        with pytest.raises(ValueError, match='lag must be an int in 0 .. window - 1 = 4'):
            ops.online_smooth_lag(torch.from_numpy(vel).to(dev), torch.from_numpy(lam).to(dev), state, taps, omega, 3, 1.0, 0.95, lag)
    assert state.seen == 0 and not state.c.any() and not state.q.any() and not state.lam.any()
