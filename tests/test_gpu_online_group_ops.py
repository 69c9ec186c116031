"""The three group ops against their single forms, bit for bit: `ops.online_smooth_group` (mf_online_smooth_group_f64) against
`ops.online_smooth` on a separate `OnlineState` per stream and against tests/online_model.py, with the streams at the four places of the ring
-- empty, one frame, the state's last free row, past the wrap --; `ops.path_limit_group` against one-frame `ops.path_limit` calls with the
row's carried step; `ops.cut_distance_pairs` against `ops.cut_distances` on two-row stacks."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import online_model as om  # noqa: E402
import path_limit_fields as pf  # noqa: E402

pytestmark = pytest.mark.gpu

S, L, OMEGA, B = 5, 8, 4, 4
ITERS, BETA, LAM_NEWEST = 10, 1.0, 0.95
HISTORY = (0, 1, L - 2, L + 3)                    # frames each stream has seen before the push under test
ORDER = [3, 0, 2]                                 # the pushed streams, out of order; stream 1 stays out


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), (what, got, want)


def stream_inputs(b, n):
    """Stream b's whole life: HISTORY[b] + n frames of velocities and weights."""
    rng = np.random.default_rng(40 + b)
    frames = HISTORY[b] + n
    lam = rng.uniform(0.0, 0.95, frames)
    lam[::5] = 0.0
    return (rng.standard_normal((frames, S)) * 3.0).astype(np.float32), lam


class Rig:
    """A group state and, per stream, an `OnlineState` and a model state, all fed the same history ONE FRAME PER CALL through their own
    smoother -- the group by single-stream pushes (K = 1) --, so that what the test compares afterwards is three independent routes."""

    def __init__(self, dev, n):
        import torch
        from meshflow_amd import host, ops
        self.dev, self.n = dev, n
        self.taps = torch.from_numpy(host.online_taps(OMEGA)).to(dev)
        self.group = ops.OnlineGroupState(B, S, L, dev)
        self.singles = [ops.OnlineState(S, L, dev) for _ in range(B)]
        self.models = [om.State(S, L) for _ in range(B)]
        self.inputs = [stream_inputs(b, n) for b in range(B)]
        for b in range(B):
            vel, lam = self.inputs[b]
            for t in range(HISTORY[b]):
                self.push_group([b], vel[None, t:t + 1], lam[None, t:t + 1])
                self.push_single(b, vel[t:t + 1], lam[t:t + 1])
                om.online_smooth(vel[t:t + 1], lam[t:t + 1], self.models[b], om.taps_for(OMEGA), OMEGA, ITERS, BETA, LAM_NEWEST)
        assert self.group.seen == list(HISTORY)

    def push_group(self, streams, vel, lam):
        import torch
        from meshflow_amd import ops
        c, p = ops.online_smooth_group(torch.from_numpy(np.ascontiguousarray(vel)).to(self.dev), torch.from_numpy(np.ascontiguousarray(lam)).to(self.dev),
                                       self.group, streams, self.taps, OMEGA, ITERS, BETA, LAM_NEWEST)
        return c.cpu().numpy(), p.cpu().numpy()

    def push_single(self, b, vel, lam):
        import torch
        from meshflow_amd import ops
        c, p = ops.online_smooth(torch.from_numpy(np.ascontiguousarray(vel)).to(self.dev), torch.from_numpy(np.ascontiguousarray(lam)).to(self.dev),
                                 self.singles[b], self.taps, OMEGA, ITERS, BETA, LAM_NEWEST)
        return c.cpu().numpy(), p.cpu().numpy()

    def new(self, b):
        vel, lam = self.inputs[b]
        return vel[HISTORY[b]:], lam[HISTORY[b]:]

    def state_of(self, b):
        return tuple(t[b].cpu().numpy() for t in (self.group.c, self.group.q, self.group.lam))


@pytest.mark.parametrize('n', [1, 3])
def test_rows_equal_the_single_call_and_the_model(dev, n):
    rig = Rig(dev, n)
    # (the history itself: a group fed one stream at a time left what the single call left)
    for b in range(B):
        for got, want, what in zip(rig.state_of(b), (rig.singles[b].c, rig.singles[b].q, rig.singles[b].lam), 'cql'):
            same(got, want.cpu().numpy(), ('history', b, what))
    idle = rig.state_of(1)
    vel = np.stack([rig.new(b)[0] for b in ORDER])
    lam = np.stack([rig.new(b)[1] for b in ORDER])
    c, p = rig.push_group(ORDER, vel, lam)
    assert c.shape == p.shape == (len(ORDER), n, S)
    assert rig.group.seen == [HISTORY[0] + n, HISTORY[1], HISTORY[2] + n, HISTORY[3] + n]
    for r, b in enumerate(ORDER):
        wc, wp = rig.push_single(b, *rig.new(b))
        mc, mp = om.online_smooth(*rig.new(b), rig.models[b], om.taps_for(OMEGA), OMEGA, ITERS, BETA, LAM_NEWEST)
        for got, single, model, what in ((c[r], wc, mc, 'c'), (p[r], wp, mp, 'p')):
            same(got, single, ('single', b, what))
            same(got, model, ('model', b, what))
        single, model = rig.singles[b], rig.models[b]
        for got, one, two, what in zip(rig.state_of(b), (single.c, single.q, single.lam), (model.c, model.q, model.lam), 'cql'):
            same(got, one.cpu().numpy(), ('single state', b, what))
            same(got, two, ('model state', b, what))
        assert np.any(p[r] != c[r]) or HISTORY[b] == 0 and n == 1             # (something was smoothed, but for a lone first frame)
    for got, want, what in zip(rig.state_of(1), idle, 'cql'):
        same(got, want, ('the unpushed stream', what))


def test_seen_zero_over_a_used_state_is_a_fresh_stream(dev):
    rig = Rig(dev, 2)
    assert float(rig.group.c[3].abs().sum()) > 0 and float(rig.group.lam[3].abs().sum()) > 0       # there is something not to read
    rig.group.reset(3)
    assert rig.group.seen == [0, 1, L - 2, 0]
    vel, lam = rig.new(3)
    c, p = rig.push_group([3, 1], np.stack([vel, rig.new(1)[0]]), np.stack([lam, rig.new(1)[1]]))
    fresh = om.State(S, L)
    mc, mp = om.online_smooth(vel, lam, fresh, om.taps_for(OMEGA), OMEGA, ITERS, BETA, LAM_NEWEST)
    same(c[0], mc, 'c')
    same(p[0], mp, 'p')
    for got, want, what in zip(rig.state_of(3), (fresh.c, fresh.q, fresh.lam), 'cql'):
        same(got, want, ('state', what))
    mc, mp = om.online_smooth(*rig.new(1), rig.models[1], om.taps_for(OMEGA), OMEGA, ITERS, BETA, LAM_NEWEST)      # ... and its neighbour goes on
    same(p[1], mp, 'the other stream')


def test_a_nan_stays_in_its_stream(dev):
    rig = Rig(dev, 3)
    vel = np.stack([rig.new(b)[0] for b in ORDER])
    lam = np.stack([rig.new(b)[1] for b in ORDER])
    vel[1, 1, 2] = np.nan                                                # stream 0, its second new frame, series 2
    c, p = rig.push_group(ORDER, vel, lam)
    poisoned = np.isnan(p)
    assert poisoned[1, 1:, 2].all() and not poisoned[0].any() and not poisoned[2].any() and not np.delete(poisoned[1], 2, axis=1).any()
    for r, b in ((0, 3), (2, 2)):
        mc, mp = om.online_smooth(*rig.new(b), rig.models[b], om.taps_for(OMEGA), OMEGA, ITERS, BETA, LAM_NEWEST)
        same(p[r], mp, ('model', b))
    for b in (1, 2, 3):
        assert not any(np.isnan(t).any() for t in rig.state_of(b)), b


def test_a_row_with_an_id_out_of_range_touches_nothing(dev):
    """Through the C ABI, past `ops.online_smooth_group`'s host check: the kernels return before they form an address from such an id."""
    import ctypes
    import torch
    from meshflow_amd import _lib
    rig = Rig(dev, 1)
    before = [rig.state_of(b) for b in range(B)]
    vel = torch.from_numpy(np.stack([rig.new(b)[0] for b in (0, 2, 3, 0)])).to(dev)
    lam = torch.from_numpy(np.stack([rig.new(b)[1] for b in (0, 2, 3, 0)])).to(dev)
    ids = torch.tensor([B, 2, -1, 0], dtype=torch.int32, device=dev)    # one past the last stream, a good row, a negative id, a negative count
    seen = torch.tensor([0, HISTORY[2], 5, -3], dtype=torch.int64, device=dev)
    c, p = (torch.full((4, 1, S), 7.25, dtype=torch.float64, device=dev) for _ in range(2))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                       # noqa: E731
    _lib.check(_lib.lib.mf_online_smooth_group_f64(ptr(vel), ptr(lam), ptr(rig.taps), ptr(ids), ptr(seen), 4, B, 1, S, OMEGA, L, ITERS, BETA, LAM_NEWEST,
                                                   ptr(rig.group.c), ptr(rig.group.q), ptr(rig.group.lam), ptr(c), ptr(p),
                                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    c, p = c.cpu().numpy(), p.cpu().numpy()
    assert (c[[0, 2, 3]] == 7.25).all() and (p[[0, 2, 3]] == 7.25).all()  # their output rows are as they were
    wc, wp = rig.push_single(2, *rig.new(2))
    same(c[1], wc, 'c')
    same(p[1], wp, 'p')
    for b in (0, 1, 3):
        for got, want, what in zip(rig.state_of(b), before[b], 'cql'):
            same(got, want, ('state', b, what))
    for got, want, what in zip(rig.state_of(2), (rig.singles[2].c, rig.singles[2].q, rig.singles[2].lam), 'cql'):
        same(got, want.cpu().numpy(), ('the good row', what))


def test_path_limit_rows_equal_one_frame_calls(dev):
    import torch
    from meshflow_amd import ops
    steps, rise = pf.STEPS, pf.RISE
    cases = pf.cases()
    for R, C, margin, rect, c, p in (cases[0], cases[3], cases[-1]):                # the smallest mesh, a 1 x 2 one, the 16 x 16 one
        d_c, d_p = torch.from_numpy(c).to(dev), torch.from_numpy(p).to(dev)
        _, raw = ops.path_limit(d_c, d_p, pf.W, pf.H, R, C, rect, steps, pf.GUARD, steps)           # rise = steps: k is k_raw
        raw = raw.cpu().numpy()
        assert raw.min() < steps - rise - 1 and raw.max() > rise, 'the field must have frames both sides of a carried step'
        # per row a carried step: none, 0, steps, beyond steps (clamped), and both sides of k_raw - rise
        carried = np.array([(-1, 0, steps, steps + 9, -7, max(0, raw[t] - rise - 1), min(steps, max(0, raw[t] - rise + 1)))[t % 7] for t in range(len(c))],
                           dtype=np.int32)
        out, k = ops.path_limit_group(d_c, d_p, pf.W, pf.H, R, C, rect, steps, pf.GUARD, rise, torch.from_numpy(carried).to(dev))
        out, k = out.cpu().numpy(), k.cpu().numpy()
        below = above = 0
        for t in range(len(c)):
            k_prev = None if carried[t] < 0 else torch.tensor([carried[t]], dtype=torch.int32, device=dev)
            want, wk = ops.path_limit(d_c[t:t + 1], d_p[t:t + 1], pf.W, pf.H, R, C, rect, steps, pf.GUARD, rise, k_prev)
            assert int(k[t]) == int(wk[0]), (R, C, t, carried[t], raw[t], k[t])
            same(out[t], want.cpu().numpy()[0], ('path', R, C, t))
            if carried[t] >= 0:
                below += int(raw[t] < min(carried[t], steps) + rise)
                above += int(raw[t] > min(carried[t], steps) + rise)
        assert below and above, (below, above)


def test_cut_distance_pairs_equals_two_row_stacks(dev):
    import torch
    from meshflow_amd import ops
    rng = np.random.default_rng(5)
    prev = rng.integers(0, 5000, (3, 256)).astype(np.int32)
    sig = rng.integers(0, 5000, (3, 256)).astype(np.int32)
    sig[1] = prev[1]                                                     # a stream whose frame did not change
    d_prev, d_sig = torch.from_numpy(prev).to(dev), torch.from_numpy(sig).to(dev)
    got = ops.cut_distance_pairs(d_prev, d_sig).cpu().numpy()
    for r in range(3):
        want = ops.cut_distances(torch.stack([d_prev[r], d_sig[r]])).cpu().numpy()
        assert int(got[r]) == int(want[1]) == int(np.abs(sig[r].astype(np.int64) - prev[r]).sum()), r
        assert int(ops.cut_distances(d_sig[r:r + 1], d_prev[r]).cpu().numpy()[0]) == int(got[r])
    assert got[1] == 0 and got[0] > 0
