"""`ops.path_limit` (mf_path_limit_f64) against tests/path_limit_model.py, k and path bit for bit: every mesh shape that changes the boundary walk,
every step count at a lane boundary, clips longer than the 64-frame look-back, the carry, the hand-worked answers of
tests/test_path_limit_model.py, and -- through `ops.cell_table` + `ops.crop_scan` -- that the limited paths of the set proven on the CPU are
covered on the device too.  128 x 96 frames throughout."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import path_limit_fields as pf  # noqa: E402
import path_limit_model as pm  # noqa: E402
from tracker_clip import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = pf.W, pf.H
RECT = (10, 7, 117, 88)


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def device_limit(dev, c, p, R, C, rect, steps=32, guard=2.0, rise=2, k_prev=None, **kw):
    import torch
    from meshflow_amd import ops
    d_prev = None if k_prev is None else torch.tensor([k_prev], dtype=torch.int32, device=dev)
    limited, k = ops.path_limit(torch.from_numpy(np.ascontiguousarray(c)).to(dev), torch.from_numpy(np.ascontiguousarray(p)).to(dev), W, H, R, C, rect,
                                steps, guard, rise, d_prev, **kw)
    assert limited.is_cuda and limited.dtype == torch.float64 and k.is_cuda and k.dtype == torch.int32 and tuple(k.shape) == (len(c),)
    return limited.cpu().numpy(), k.cpu().numpy()


def against_model(dev, c, p, R, C, rect, steps=32, guard=2.0, rise=2, k_prev=None, what=None):
    want, want_k, raw = pm.limit(c, p, W, H, R, C, rect, steps, guard, rise, k_prev)
    got, got_k = device_limit(dev, c, p, R, C, rect, steps, guard, rise, k_prev)
    assert got_k.tolist() == want_k.tolist(), (what, got_k.tolist(), want_k.tolist())
    same_bits(got, want, what)
    return want_k, raw


@pytest.mark.parametrize('mesh', [(1, 1), (1, 2), (3, 1), (16, 16), (256, 256)])
def test_every_boundary_walk(dev, mesh):
    """1x1: 4 boundary vertices and 8 series, fewer than the lanes; 1x2 and 3x1: the order of the walk; 256x256: 1,024 vertices, the cap."""
    R, C = mesh
    c, p = pf.field(R, C, 7, frames=2 if R == 256 else 12)
    seen = []
    for margin in pf.MARGINS:
        k, _ = against_model(dev, c, p, R, C, pf.rectangle(margin), what=(mesh, margin))
        seen += k.tolist()
    assert R == 256 or (min(seen) < 32 and max(seen) > 0)                # (the case limits something and does not throw everything away)


@pytest.mark.parametrize('steps', [1, 2, 32, 63, 64])
def test_every_step_count_at_a_lane_boundary(dev, steps):
    """Lane 63 is candidate 64; K = 63 leaves it idle; K = 1 has the one candidate."""
    c, p = pf.field(4, 4, 11, frames=16)
    p[5] = c[5]                                                          # one frame that passes every candidate
    k, raw = against_model(dev, c, p, 4, 4, RECT, steps=steps, rise=1, what=steps)
    assert raw[5] == steps and raw.min() < steps


@pytest.mark.parametrize('n', [1, 2, 65, 130])
def test_the_recovery_crosses_the_look_back(dev, n):
    """rise 1, K 64, k_raw = 0 planted at frame 0 and K everywhere else: k_t = min(t, 64), which needs all 64 terms and then none of them."""
    R, C = 2, 3
    c, _ = pf.field(R, C, 13, frames=n)
    p = c.copy()
    p[0, 0:2] = np.nan                                                   # vertex (0, 0)
    k, raw = against_model(dev, c, p, R, C, RECT, steps=64, rise=1, what=n)
    assert raw.tolist() == [0] + [64] * (n - 1) and k.tolist() == [min(t, 64) for t in range(n)]


def test_rise_K_is_k_raw_and_guard_0(dev):
    c, p = pf.field(16, 16, 17, frames=12)
    for guard in (0.0, 2.0, 3.5):
        k, raw = against_model(dev, c, p, 16, 16, RECT, rise=32, guard=guard, what=guard)
        assert k.tolist() == raw.tolist()
    assert pm.limit(c, p, W, H, 16, 16, RECT, 32, 0.0, 32)[1].sum() > pm.limit(c, p, W, H, 16, 16, RECT, 32, 3.5, 32)[1].sum()


def test_the_hand_worked_answers(dev):
    """tests/test_path_limit_model.py's: the four translations stop at k = 15 of 32, no correction is K and p's bits, a NaN in a boundary
    vertex is 0 and c's bits, a NaN inside changes nothing, a mirrored mesh stops at 2."""
    R, C = 4, 4
    S = (R + 1) * (C + 1) * 2
    base = np.linspace(-3.0, 4.0, S)
    rows_c, rows_p, want = [], [], []
    for dx, dy in ((16, 0), (-16, 0), (0, 10), (0, -10)):
        p = base.reshape(-1, 2) + np.array([dx, dy], np.float64)
        rows_c.append((p - np.array([dx, dy], np.float64)).reshape(-1))
        rows_p.append(p.reshape(-1))
        want.append(15)
    rows_c.append(base), rows_p.append(base.copy()), want.append(32)                       # no correction
    for (row, col), k in (((0, 2), 0), ((2, 4), 0), ((4, 1), 0), ((3, 0), 0), ((0, 0), 0), ((2, 2), 32), ((1, 3), 32)):
        p = (base + 1.0).reshape(R + 1, C + 1, 2).copy()
        p[row, col] = np.nan
        rows_c.append(base), rows_p.append(p.reshape(-1)), want.append(k)
    xs, _ = pm.grid(W, H, R, C)
    mirror = np.zeros((R + 1, C + 1, 2))
    mirror[..., 0] = (W - 1) - 2 * xs[None, :]
    rows_c.append(np.zeros(S)), rows_p.append(mirror.reshape(-1)), want.append(2)
    c, p = np.stack(rows_c), np.stack(rows_p)
    k, raw = against_model(dev, c, p, R, C, RECT, rise=32, what='hand')
    assert k.tolist() == want
    got, _ = device_limit(dev, c, p, R, C, RECT, rise=32)
    for t, kt in enumerate(want):
        if kt in (0, 32):
            assert got[t].tobytes() == (c if kt == 0 else p)[t].tobytes(), t


def test_the_carry_chains_calls_into_one(dev):
    import torch
    from meshflow_amd import ops
    R, C = 16, 16
    c, p = pf.field(R, C, 19, frames=20)
    d_c, d_p = torch.from_numpy(c).to(dev), torch.from_numpy(p).to(dev)
    whole, whole_k = ops.path_limit(d_c, d_p, W, H, R, C, RECT, 32, 2.0, 1)
    again, again_k = ops.path_limit(d_c, d_p, W, H, R, C, RECT, 32, 2.0, 1)               # two launches: the same bytes
    same_bits(again.cpu().numpy(), whole.cpu().numpy(), 'again')
    same_bits(again_k.cpu().numpy(), whole_k.cpu().numpy(), 'again k')
    parts, ks, k_prev, at = [], [], None, 0
    for b in (1, 3, 16):
        out, k = ops.path_limit(d_c[at:at + b], d_p[at:at + b], W, H, R, C, RECT, 32, 2.0, 1, k_prev)
        parts.append(out), ks.append(k)
        k_prev, at = k[-1:], at + b
    same_bits(torch.cat(parts).cpu().numpy(), whole.cpu().numpy(), 'chain')
    same_bits(torch.cat(ks).cpu().numpy(), whole_k.cpu().numpy(), 'chain k')
    assert np.diff(whole_k.cpu().numpy()).max() == 1                     # (the slew limit was at work somewhere)
    # a carry of the caller's own, the values past either end clamped; `out=`; the 4-d layout
    for carried in (0, 5, 32, -3, 99):
        against_model(dev, c[:6], p[:6], R, C, RECT, rise=1, k_prev=carried, what=carried)
    into = torch.full((20, c.shape[1]), -1.0, dtype=torch.float64, device=dev)
    out, k = ops.path_limit(d_c.view(20, R + 1, C + 1, 2), d_p.view(20, R + 1, C + 1, 2), W, H, R, C, RECT, 32, 2.0, 1, out=into)
    assert out is into
    same_bits(into.cpu().numpy(), whole.cpu().numpy(), 'out=')


def test_the_proven_set_is_covered_on_the_device(dev):
    """What tests/test_path_limit_model.py asserts through the C oracle, through the device's own cell table and crop scan."""
    import torch
    from meshflow_amd import ops
    before, after = [], []
    for R, C, margin, rect, c, p in pf.cases():
        d_c, d_p = torch.from_numpy(c).to(dev), torch.from_numpy(p).to(dev)
        limited, k = ops.path_limit(d_c, d_p, W, H, R, C, rect, pf.STEPS, pf.GUARD, pf.STEPS)
        want, want_k, _ = pm.limit(c, p, W, H, R, C, rect, pf.STEPS, pf.GUARD, pf.STEPS)
        same_bits(limited.cpu().numpy(), want, (R, C, margin))
        assert k.cpu().numpy().tolist() == want_k.tolist()
        for path, into in ((d_p, before), (limited, after)):
            table = ops.cell_table(d_c, path, W, H, R, C)
            crop = ops.crop_scan(table).cpu().numpy()
            table.check()
            into.append(pf.covered(crop, rect))
    before, after = np.concatenate(before), np.concatenate(after)
    assert (~before).mean() >= 0.25 and after.all(), ((~before).sum(), np.nonzero(~after)[0].tolist())
