"""`ops.online_smooth` (mf_online_smooth_f64, csrc/online_smooth.hip) against tests/online_model.py, bit for bit in the two paths and in
all three state tensors, at the shapes where the kernel can go wrong: one series and more than a wavefront's worth, the smallest and the
largest window, a band wider than the window, blocks that end before, at and after the point where the window starts to slide."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import online_model as om  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def inputs(n, S, seed, lam_hi=0.95):
    rng = np.random.default_rng(seed)
    vel = (rng.standard_normal((n, S)) * 3.0).astype(np.float32)
    lam = rng.uniform(0.0, lam_hi, n)
    lam[::5] = 0.0                                             # exact zeros: the frame then keeps (C + beta q) / (1 + beta)
    lam[3::7] = 100.0                                          # the constant-high definition's weight
    return vel, lam


def model_run(vel, lam, blocks, L, omega, iters, beta, lam_newest):
    state, taps, at, c, p = om.State(vel.shape[1], L), om.taps_for(omega), 0, [], []
    for b in blocks:
        ci, pi = om.online_smooth(vel[at:at + b], lam[at:at + b], state, taps, omega, iters, beta, lam_newest)
        c.append(ci)
        p.append(pi)
        at += b
    return np.concatenate(c), np.concatenate(p), state


def device_run(dev, vel, lam, blocks, L, omega, iters, beta, lam_newest):
    import torch
    from meshflow_amd import host, ops
    state, at, c, p = ops.OnlineState(vel.shape[1], L, dev), 0, [], []
    taps = torch.from_numpy(host.online_taps(omega)).to(dev)
    d_vel, d_lam = torch.from_numpy(vel).to(dev), torch.from_numpy(lam).to(dev)
    for b in blocks:
        ci, pi = ops.online_smooth(d_vel[at:at + b], d_lam[at:at + b], state, taps, omega, iters, beta, lam_newest)
        c.append(ci)
        p.append(pi)
        at += b
    return torch.cat(c).cpu().numpy(), torch.cat(p).cpu().numpy(), state


def same(got, want, what):
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), (
        what, np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:4].tolist(), float(np.nanmax(np.abs(got - want))))


def check(dev, n, S, L, omega, iters, beta, seed, blocks=None, lam_newest=0.95):
    vel, lam = inputs(n, S, seed)
    blocks = blocks or [n]
    c, p, state = device_run(dev, vel, lam, blocks, L, omega, iters, beta, lam_newest)
    wc, wp, wstate = model_run(vel, lam, [n], L, omega, iters, beta, lam_newest)
    same(c, wc, 'c')
    same(p, wp, 'p')
    same(state.c.cpu().numpy(), wstate.c, 'state.c')
    same(state.q.cpu().numpy(), wstate.q, 'state.q')
    same(state.lam.cpu().numpy(), wstate.lam, 'state.lam')
    assert state.seen == wstate.seen == n


# (n as a multiple of L plus an offset, S, L, omega, iters, beta)
SHAPES = [
    ((0, 1), 1, 2, 1, 1, 0.0), ((1, 0), 3, 2, 3, 10, 1.0), ((3, 0), 130, 2, 1, 10, 1.0),
    ((0, 1), 3, 5, 8, 10, 1.0), ((1, -1), 130, 5, 8, 1, 0.0), ((1, 0), 1, 5, 8, 10, 1.0), ((1, 1), 3, 5, 8, 10, 0.0), ((3, 0), 130, 5, 8, 10, 1.0),
    ((1, -1), 3, 64, 1, 10, 1.0), ((1, 1), 130, 64, 1, 1, 1.0), ((1, 0), 3, 64, 64, 10, 1.0), ((1, 1), 130, 64, 64, 10, 0.0),
    ((3, 0), 3, 64, 64, 1, 1.0), ((3, 0), 130, 40, 10, 10, 1.0), ((0, 1), 130, 64, 64, 10, 1.0),
]


@pytest.mark.parametrize('n_of,S,L,omega,iters,beta', SHAPES)
def test_equals_the_model(dev, n_of, S, L, omega, iters, beta):
    check(dev, n_of[0] * L + n_of[1], S, L, omega, iters, beta, seed=S + L + omega)


@pytest.mark.parametrize('S,L,omega', [(3, 9, 4), (130, 16, 20), (1, 64, 10)])
def test_blocks_give_the_bytes_of_one_call(dev, S, L, omega):
    n = 3 * L + 2
    check(dev, n, S, L, omega, 10, 1.0, seed=9, blocks=[1, 7, L - 1, n - 1 - 7 - (L - 1)])
    check(dev, n, S, L, omega, 3, 0.5, seed=10, blocks=[1] * 12 + [n - 12], lam_newest=0.0)


def test_two_launches_give_the_same_bytes(dev):
    vel, lam = inputs(50, 130, 21)
    a = device_run(dev, vel, lam, [20, 30], 16, 10, 10, 1.0, 0.95)
    b = device_run(dev, vel, lam, [20, 30], 16, 10, 10, 1.0, 0.95)
    for x, y in zip(a[:2], b[:2]):
        assert x.tobytes() == y.tobytes()
    for name in ('c', 'q', 'lam'):
        assert getattr(a[2], name).cpu().numpy().tobytes() == getattr(b[2], name).cpu().numpy().tobytes()


def test_non_finite_values_stay_in_their_series(dev):
    n, S, L, omega = 30, 130, 8, 4
    vel, lam = inputs(n, S, 33)
    wc, wp, wstate = model_run(vel, lam, [n], L, omega, 5, 1.0, 0.95)
    bad = vel.copy()
    bad[4, 17] = np.nan
    bad[9, 64] = np.inf
    c, p, state = device_run(dev, bad, lam, [11, 19], L, omega, 5, 1.0, 0.95)
    clean = np.ones(S, dtype=bool)
    clean[[17, 64]] = False
    for got, want in ((c, wc), (p, wp), (state.c.cpu().numpy(), wstate.c), (state.q.cpu().numpy(), wstate.q)):
        same(np.ascontiguousarray(got[:, clean]), np.ascontiguousarray(want[:, clean]), 'the other series')
    assert np.isnan(p[4:, 17]).all() and np.isfinite(p[:4, 17]).all()
    assert not np.isfinite(p[9:, 64]).any() and np.isfinite(p[:9, 64]).all()
    assert np.isinf(c[9:, 64]).all()


def test_outputs_stay_inside_their_bounds(dev):
    import torch
    from meshflow_amd import _lib, host, ops
    n, S, L, omega, guard = 11, 7, 6, 3, 64
    vel, lam = inputs(n, S, 41)
    wc, wp, wstate = model_run(vel, lam, [n], L, omega, 4, 1.0, 0.95)
    sizes = {'c': n * S, 'p': n * S, 'sc': (L - 1) * S, 'sq': (L - 1) * S, 'sl': L - 1}
    total = sum(v + 2 * guard for v in sizes.values())
    arena = torch.full((total,), -777.0, dtype=torch.float64, device=dev)
    views, at = {}, 0
    for k, v in sizes.items():
        views[k] = arena[at + guard:at + guard + v]
        at += v + 2 * guard
    for k in ('sc', 'sq', 'sl'):
        views[k].zero_()
    taps = torch.from_numpy(host.online_taps(omega)).to(dev)
    d_vel, d_lam = torch.from_numpy(vel).to(dev), torch.from_numpy(lam).to(dev)
    ptr = ops._ptr
    _lib.check(_lib.lib.mf_online_smooth_f64(ptr(d_vel), ptr(d_lam), ptr(taps), n, S, omega, L, 4, 1.0, 0.95, 0, ptr(views['sc']), ptr(views['sq']),
                                             ptr(views['sl']), ptr(views['c']), ptr(views['p']), ops._stream()))
    got = arena.cpu().numpy()
    inside = np.zeros(total, dtype=bool)
    at = 0
    for k, v in sizes.items():
        inside[at + guard:at + guard + v] = True
        at += v + 2 * guard
    assert (got[~inside] == -777.0).all()
    same(views['c'].cpu().numpy().reshape(n, S), wc, 'c')
    same(views['p'].cpu().numpy().reshape(n, S), wp, 'p')
    same(views['sc'].cpu().numpy().reshape(L - 1, S), wstate.c, 'state.c')
    same(views['sq'].cpu().numpy().reshape(L - 1, S), wstate.q, 'state.q')
    same(views['sl'].cpu().numpy(), wstate.lam, 'state.lam')


def test_one_block_path_equals_vertex_motion(dev):
    """A whole clip in one block: c is `ops.vertex_motion`'s displacements bit for bit."""
    import torch
    from meshflow_amd import host, ops
    P, R, C, W, H = 23, 4, 6, 128, 96
    rng = np.random.default_rng(2)
    hom = np.tile(np.identity(3), (P, 1, 1))
    hom[:, :2, 2] = rng.uniform(-4.0, 4.0, (P, 2))
    hom[:, 0, 1] = rng.uniform(-0.01, 0.01, P)
    pairs = []
    for p in range(P):
        e = rng.uniform(0.0, 1.0, (20, 2)) * (W - 1, H - 1)
        pairs.append((e, e + hom[p, :2, 2] + rng.normal(0.0, 0.5, e.shape)))
    early, late, offsets, kmax = host.pack_features(pairs)
    disp, vel, status = ops.vertex_motion(*(torch.from_numpy(a).to(dev) for a in (early, late, offsets, hom)), kmax, W, H, R, C, 10, 10)
    ops.vertex_motion_check(status)
    S = (R + 1) * (C + 1) * 2
    state = ops.OnlineState(S, 10, dev)
    block = torch.cat([torch.zeros((1, S), dtype=torch.float32, device=dev), vel.reshape(P, S)])
    lam = torch.full((P + 1,), 0.5, dtype=torch.float64, device=dev)
    c, p = ops.online_smooth(block, lam, state, torch.from_numpy(host.online_taps(5)).to(dev), 5, 3, 1.0, 0.5)
    assert float(vel.abs().max()) > 1.0
    assert c.cpu().numpy().tobytes() == disp.reshape(P + 1, S).cpu().numpy().tobytes()
    assert torch.isfinite(p).all()
