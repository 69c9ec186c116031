"""tests/online_lag_model.py against what it claims: lag 0 is tests/online_model.py, the state never depends on the lag, any split into
blocks gives one block's bytes, every frame comes out exactly once, and look-ahead buys smoothness.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import online_lag_model as olm  # noqa: E402
import online_model as om  # noqa: E402
from test_online_model import random_walk, second_difference  # noqa: E402

N, S, L, OMEGA, ITERS = 30, 5, 8, 4, 6


def run(vel, lam, blocks, L, omega, iters, beta, lag, lam_newest=0.95):
    """(c, p) of everything the blocks hand out, the pending (c, p), the final state."""
    state, taps, at, c, p = om.State(vel.shape[1], L), om.taps_for(omega), 0, [], []
    for b in blocks:
        seen = state.seen
        ci, pi = olm.online_smooth_lag(vel[at:at + b], lam[at:at + b], state, taps, omega, iters, beta, lam_newest, lag)
        assert ci.shape == pi.shape == (max(0, seen + b - lag) - max(0, seen - lag), vel.shape[1])
        c.append(ci)
        p.append(pi)
        at += b
    assert at == vel.shape[0] == state.seen
    return np.concatenate(c), np.concatenate(p), olm.pending(state, lag), state


def plain(vel, lam, L, omega, iters, beta, lam_newest=0.95):
    state = om.State(vel.shape[1], L)
    c, p = om.online_smooth(vel, lam, state, om.taps_for(omega), omega, iters, beta, lam_newest)
    return c, p, state


def same_state(a, b):
    return a.seen == b.seen and all(getattr(a, k).tobytes() == getattr(b, k).tobytes() for k in ('c', 'q', 'lam'))


def test_lag_0_is_the_plain_model():
    vel, lam = random_walk(N, S, 11)
    wc, wp, wstate = plain(vel, lam, L, OMEGA, ITERS, 1.0)
    for blocks in ([N], [1, 7, 7, 15]):
        c, p, (pc, pp), state = run(vel, lam, blocks, L, OMEGA, ITERS, 1.0, 0)
        assert c.tobytes() == wc.tobytes() and p.tobytes() == wp.tobytes() and same_state(state, wstate)
        assert pc.shape == pp.shape == (0, S)


@pytest.mark.parametrize('lag', range(L))
def test_the_state_does_not_depend_on_the_lag(lag):
    vel, lam = random_walk(N, S, 11)
    _, _, wstate = plain(vel, lam, L, OMEGA, ITERS, 1.0)
    for blocks in ([N], [1, 7, 7, 15]):
        assert same_state(run(vel, lam, blocks, L, OMEGA, ITERS, 1.0, lag)[3], wstate), (lag, blocks)


@pytest.mark.parametrize('lag', [1, 3, 7])
def test_any_split_gives_the_bytes_of_one_block(lag):
    vel, lam = random_walk(N, S, 11)
    c0, p0, (pc0, pp0), s0 = run(vel, lam, [N], L, OMEGA, ITERS, 1.0, lag)
    assert c0.shape == (N - lag, S)
    for blocks in ([1] * N, [1, 7, 7, 15], [29, 1], [2, 28]):
        c, p, (pc, pp), s = run(vel, lam, blocks, L, OMEGA, ITERS, 1.0, lag)
        for a, b in ((c, c0), (p, p0), (pc, pc0), (pp, pp0)):
            assert a.shape == b.shape and a.tobytes() == b.tobytes(), (lag, blocks)
        assert same_state(s, s0)


@pytest.mark.parametrize('lag', [0, 1, 3, 7])
def test_every_frame_comes_out_once_and_the_path_is_the_running_sum(lag):
    vel, lam = random_walk(N, S, 11)
    want, acc = np.zeros((N, S)), np.zeros(S)
    for t in range(1, N):
        acc = acc + vel[t].astype(np.float64)
        want[t] = acc
    for blocks in ([N], [1] * N, [1, 7, 7, 15], [2, 28]):
        c, p, (pc, pp), _ = run(vel, lam, blocks, L, OMEGA, ITERS, 1.0, lag)
        assert c.shape[0] == N - lag and pc.shape[0] == lag and p.shape == c.shape and pp.shape == pc.shape
        # C identifies the frame: the walk's running sums are pairwise distinct
        assert np.concatenate([c, pc]).tobytes() == want.tobytes(), (lag, blocks)
        assert len({row.tobytes() for row in want}) == N


def test_the_lagged_value_is_the_later_windows_solution():
    """P^lag_t read straight from the definition: push frames one at a time with the plain model and look at the state after frame
    t + lag -- including lag = L - 1, whose frame the state has just let go (taken from window t + lag solved by hand)."""
    n, lag_max = 14, L - 1
    vel, lam = random_walk(n, S, 4)
    taps = om.taps_for(OMEGA)
    state, after = om.State(S, L), []
    for t in range(n):
        om.online_smooth(vel[t:t + 1], lam[t:t + 1], state, taps, OMEGA, ITERS, 1.0, 0.95)
        after.append(state.copy())
    for lag in (1, 2, lag_max - 1):
        _, p, _, _ = run(vel, lam, [n], L, OMEGA, ITERS, 1.0, lag)
        for t in range(n - lag):
            assert p[t].tobytes() == after[t + lag].q[L - 2 - lag].tobytes(), (lag, t)
    # lag = L - 1: window xi = t + L - 1 is full; its frames' C and lam, and q from window xi - 1, all from the state after frame xi - 1
    _, p, _, _ = run(vel, lam, [3, n - 3], L, OMEGA, ITERS, 1.0, lag_max)
    for t in range(n - lag_max):
        xi = t + lag_max
        prev = after[xi - 1]
        C = np.concatenate([prev.c, after[xi].c[-1:]])
        lam_w = np.concatenate([prev.lam[:-1], [lam[xi], 0.95]])
        x = om.solve_window(C, prev.q, lam_w, taps, OMEGA, ITERS, 1.0)
        assert p[t].tobytes() == x[0].tobytes() and x[1:].tobytes() == after[xi].q.tobytes(), t


def test_limits():
    state = om.State(S, L)
    vel, lam = random_walk(2, S, 1)
    for lag in (-1, L, True, 1.0):
        with pytest.raises(AssertionError):
            olm.online_smooth_lag(vel, lam, state, om.taps_for(OMEGA), OMEGA, ITERS, 1.0, 0.95, lag)
        with pytest.raises(AssertionError):
            olm.pending(state, lag)
    assert state.seen == 0


def test_look_ahead_buys_smoothness():
    """The 60-frame walk of test_online_model.test_output_is_smoother_than_input (seed 7, step 2.0, L 20, omega 10, 10 sweeps, beta 1, 8
    series), over the complete output -- handed out plus pending: mean |second difference| falls strictly over lags 0, 1, 2, 3, 5; lag 5 is
    below 0.6 x lag 0 (0.47 when this was written); the mean correction |p - c| at lag 5 is below lag 0's."""
    vel, _ = random_walk(60, 8, 7, step=2.0)
    lam = np.full(60, 0.95)
    rough, shake, correction = None, {}, {}
    for lag in (0, 1, 2, 3, 5, 8, 10):
        c, p, (pc, pp), _ = run(vel, lam, [60], 20, 10, 10, 1.0, lag)
        c, p = np.concatenate([c, pc]), np.concatenate([p, pp])
        assert c.shape == (60, 8)
        rough = second_difference(c)
        shake[lag], correction[lag] = second_difference(p), np.abs(p - c).mean()
        print(f'lag {lag:2d}: mean |second difference| {shake[lag]:.4f} (path {rough:.4f}, ratio {shake[lag] / rough:.3f}), '
              f'mean |p - c| {correction[lag]:.3f}')
    lags = (0, 1, 2, 3, 5)
    assert all(shake[a] > shake[b] for a, b in zip(lags[:-1], lags[1:])), shake
    assert shake[5] < 0.6 * shake[0], (shake[5], shake[0])
    assert correction[5] < correction[0], correction
