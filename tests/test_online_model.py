"""tests/online_model.py against what it claims to be: the Jacobi iteration of each window's linear system, independent of how the frames
are split into blocks, equivariant under a shift of the path, and a smoother.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import online_model as om  # noqa: E402


def random_walk(n, S, seed, step=3.0):
    """(n, S) float32 velocities of a random walk, and (n,) weights in [0, 0.95]."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, S)) * step).astype(np.float32), rng.uniform(0.0, 0.95, n)


def run(vel, lam, blocks, L, omega, iters, beta, lam_newest=0.95):
    S = vel.shape[1]
    state, taps, at, c, p = om.State(S, L), om.taps_for(omega), 0, [], []
    for b in blocks:
        ci, pi = om.online_smooth(vel[at:at + b], lam[at:at + b], state, taps, omega, iters, beta, lam_newest)
        c.append(ci)
        p.append(pi)
        at += b
    assert at == vel.shape[0]
    return np.concatenate(c), np.concatenate(p), state


def test_window_solves_its_dense_system():
    """Window xi's matrix and right-hand side written out from the formulas; the model's window after enough sweeps against
    np.linalg.solve at 1e-11 absolute (omega 4, L 8, lam in [0, 0.95], |C| <= 200)."""
    omega, L, beta, S = 4, 8, 1.0, 6
    rng = np.random.default_rng(5)
    taps = om.taps_for(omega)
    for m in (1, 2, 5, L):                                     # a window that is still filling, and a full one
        C = rng.uniform(-200.0, 200.0, (m, S))
        q = C[:m - 1] + rng.uniform(-5.0, 5.0, (m - 1, S))
        lam = rng.uniform(0.0, 0.95, m)
        lam[m // 2] = 0.0
        A, rhs = np.zeros((m, m)), C.copy()
        for t in range(m):
            beta_t = beta if t < m - 1 else 0.0
            sw = 0.0
            for d in range(-omega, omega + 1):
                if d != 0 and 0 <= t + d < m:
                    A[t, t + d] = -2.0 * lam[t] * taps[abs(d) - 1]
                    sw += taps[abs(d) - 1]
            A[t, t] = (1.0 + beta_t) + 2.0 * lam[t] * sw
            if t < m - 1:
                rhs[t] = C[t] + beta_t * q[t]
        want = np.linalg.solve(A, rhs)
        got = om.solve_window(C, q, lam, taps, omega, 400, beta)
        err = np.abs(got - want).max()
        print(f'm={m}: cond {np.linalg.cond(A):.2f}, max |model - solve| {err:.3g}')
        assert err <= 1e-11, (m, err)


def test_any_split_gives_the_bytes_of_one_block():
    n, S, L, omega = 30, 5, 8, 4
    vel, lam = random_walk(n, S, 11)
    c0, p0, s0 = run(vel, lam, [n], L, omega, 6, 1.0)
    for blocks in ([1] * n, [1, 7, L - 1, n - 1 - 7 - (L - 1)], [L, L, L, n - 3 * L], [29, 1], [2, 28]):
        c, p, s = run(vel, lam, blocks, L, omega, 6, 1.0)
        for a, b in ((c, c0), (p, p0), (s.c, s0.c), (s.q, s0.q), (s.lam, s0.lam)):
            assert a.tobytes() == b.tobytes(), blocks
        assert s.seen == n
    # the path is accumulate_kernel's running sum: sequential float64 additions of the float32 velocities from C_0 = 0
    want, acc = np.zeros((n, S)), np.zeros(S)
    for t in range(1, n):
        acc = acc + vel[t].astype(np.float64)
        want[t] = acc
    assert c0.tobytes() == want.tobytes()


def test_shift_of_the_path_shifts_the_output():
    """A constant k added to the velocities' running sum -- the carried C and, with it, the carried solution q, ten frames into a session --
    moves every later output by k, within 1e-9: the window's system and its Jacobi iteration commute with a shift of the path."""
    n, S, L, omega, k = 24, 4, 8, 4, 37.25
    vel, lam = random_walk(n, S, 3)
    taps = om.taps_for(omega)
    first = om.State(S, L)
    om.online_smooth(vel[:10], lam[:10], first, taps, omega, 8, 1.0, 0.95)
    moved = first.copy()
    moved.c[L - 1 - min(first.seen, L - 1):] += k
    moved.q[L - 1 - min(first.seen, L - 1):] += k
    c0, p0 = om.online_smooth(vel[10:], lam[10:], first, taps, omega, 8, 1.0, 0.95)
    c1, p1 = om.online_smooth(vel[10:], lam[10:], moved, taps, omega, 8, 1.0, 0.95)
    assert np.abs(c1 - (c0 + k)).max() <= 1e-9 and np.abs(p1 - (p0 + k)).max() <= 1e-9
    assert np.abs(moved.q - (first.q + k)).max() <= 1e-9


def second_difference(path):
    return np.abs(path[2:] - 2.0 * path[1:-1] + path[:-2]).mean()


def test_output_is_smoother_than_input():
    """60 frames of a seeded random walk, omega 10, L 20, 10 sweeps, beta 1 (profiles/online.md has the ratio)."""
    vel, _ = random_walk(60, 8, 7, step=2.0)
    lam = np.full(60, 0.95)
    c, p, _ = run(vel, lam, [60], 20, 10, 10, 1.0)
    rough, smooth = second_difference(c), second_difference(p)
    print(f'mean |second difference|: path {rough:.4f}, smoothed {smooth:.4f}, ratio {smooth / rough:.4f}')
    assert smooth < rough
