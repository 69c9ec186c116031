"""The two ops of a lagged group against their specifications, bit for bit: `ops.online_smooth_group_lag` (mf_online_smooth_group_lag_f64)
against `ops.online_smooth_lag` on a separate `OnlineState` per stream -- outputs, `final` and the three state tensors after every block, with
blocks of one and three frames, subsets in turning order, a stream that joins late and one that is reset, until the ring has wrapped --, with
lag = 0 against `ops.online_smooth_group`, and with rows that must touch nothing; `ops.ring_exchange` (mf_ring_exchange_u8) against
tests/ring_model.py on both paths of the kernel, with canaries around the ring and the output."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ring_model  # noqa: E402

pytestmark = pytest.mark.gpu

S, L, OMEGA, B = 5, 8, 4, 4
ITERS, BETA, LAM_NEWEST = 10, 1.0, 0.95
# (the streams pushed, the frames of each): stream 3 joins at block 2, stream 1 is reset in front of block 5
BLOCKS = (([0, 1], 1), ([1, 2, 0], 3), ([2, 3], 1), ([3, 0, 1], 3), ([0, 1, 2, 3], 1), ([1, 2, 3, 0], 3), ([2, 0], 1), ([3, 1, 2], 3),
          ([0, 1, 2, 3], 1))
RESET = (5, 1)


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def same(got, want, what):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.tobytes() == want.tobytes(), (what, got, want)


def inputs():
    """Per stream 32 frames of velocities and weights, more than any stream is pushed."""
    out = []
    for b in range(B):
        rng = np.random.default_rng(70 + b)
        lam = rng.uniform(0.0, 0.95, 32)
        lam[::5] = 0.0
        out.append(((rng.standard_normal((32, S)) * 3.0).astype(np.float32), lam))
    return out


def run(dev, lag, grouped):
    """BLOCKS through one group state with `grouped(state, vel, lam, ids)` -> (c, p, final or None) and through an `OnlineState` per stream
    with `ops.online_smooth_lag`; everything is compared block by block.  Returns the `final` of every block and the last counts."""
    import torch
    from meshflow_amd import host, ops
    taps = torch.from_numpy(host.online_taps(OMEGA)).to(dev)
    group, singles = ops.OnlineGroupState(B, S, L, dev), [ops.OnlineState(S, L, dev) for _ in range(B)]
    data, at, finals = inputs(), [0] * B, []
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)    # noqa: E731
    for block, (ids, n) in enumerate(BLOCKS):
        if block == RESET[0]:
            group.reset(RESET[1])
            singles[RESET[1]].reset()
        idle = {b: [t[b].cpu().numpy() for t in (group.c, group.q, group.lam)] for b in range(B) if b not in ids}
        vel = np.stack([data[b][0][at[b]:at[b] + n] for b in ids])
        lam = np.stack([data[b][1][at[b]:at[b] + n] for b in ids])
        before = [group.seen[b] for b in ids]
        c, p, final = grouped(group, up(vel), up(lam), ids, taps)
        assert tuple(c.shape) == tuple(p.shape) == (len(ids), n, S)
        c, p = c.cpu().numpy(), p.cpu().numpy()
        for r, b in enumerate(ids):
            wc, wp = ops.online_smooth_lag(up(vel[r]), up(lam[r]), singles[b], taps, OMEGA, ITERS, BETA, LAM_NEWEST, lag)
            m = int(wc.shape[0])
            assert m == max(0, before[r] + n - lag) - max(0, before[r] - lag) and (final is None or final[r] == m), (block, b, final, m)
            same(c[r, n - m:], wc.cpu().numpy(), ('c', block, b))
            same(p[r, n - m:], wp.cpu().numpy(), ('p', block, b))
            assert not c[r, :n - m].any() and not p[r, :n - m].any(), ('the rows of frames that do not exist are zeros', block, b)
            for got, want, what in zip((group.c, group.q, group.lam), (singles[b].c, singles[b].q, singles[b].lam), 'cql'):
                same(got[b].cpu().numpy(), want.cpu().numpy(), ('state', block, b, what))
            at[b] += n
            assert group.seen[b] == singles[b].seen == before[r] + n
        for b, kept in idle.items():
            for got, want, what in zip((group.c, group.q, group.lam), kept, 'cql'):
                same(got[b].cpu().numpy(), want, ('the unpushed stream', block, b, what))
        finals.append(final)
    return finals, list(group.seen)


@pytest.mark.parametrize('lag', [1, 3, L - 1])
def test_rows_equal_the_single_lagged_call(dev, lag):
    from meshflow_amd import ops

    def grouped(state, vel, lam, ids, taps):
        return ops.online_smooth_group_lag(vel, lam, state, ids, taps, OMEGA, ITERS, BETA, LAM_NEWEST, lag)

    finals, seen = run(dev, lag, grouped)
    assert max(seen) > L and seen == [13, 7, 13, 12]                      # the ring has wrapped
    # rows of one call differ in how many frames they hand out: a stream with no more than `lag` frames beside one past it
    assert any(len(set(final)) > 1 for final in finals), finals
    assert any(0 in final and max(final) == n for final, (_, n) in zip(finals, BLOCKS)), finals


def test_lag_zero_gives_the_plain_group_calls_bytes(dev):
    from meshflow_amd import ops
    outputs = {}

    def lagged(state, vel, lam, ids, taps):
        c, p, final = ops.online_smooth_group_lag(vel, lam, state, ids, taps, OMEGA, ITERS, BETA, LAM_NEWEST, 0)
        outputs.setdefault('lagged', []).append((c.cpu().numpy(), p.cpu().numpy()))
        assert final == [vel.shape[1]] * len(ids)
        return c, p, final

    def plain(state, vel, lam, ids, taps):
        c, p = ops.online_smooth_group(vel, lam, state, ids, taps, OMEGA, ITERS, BETA, LAM_NEWEST)
        outputs.setdefault('plain', []).append((c.cpu().numpy(), p.cpu().numpy()))
        return c, p, None

    run(dev, 0, lagged)
    run(dev, 0, plain)
    assert len(outputs['lagged']) == len(outputs['plain']) == len(BLOCKS)
    for block, ((c, p), (wc, wp)) in enumerate(zip(outputs['lagged'], outputs['plain'])):
        same(c, wc, ('c', block))
        same(p, wp, ('p', block))


def test_a_row_with_an_id_out_of_range_touches_nothing(dev):
    """Through the C ABI, past `ops.online_smooth_group_lag`'s host checks: the kernels return before they form an address from such a row."""
    import torch
    from meshflow_amd import _lib, host, ops
    lag, history = 3, 5
    taps = torch.from_numpy(host.online_taps(OMEGA)).to(dev)
    group, single = ops.OnlineGroupState(B, S, L, dev), ops.OnlineState(S, L, dev)
    data = inputs()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)    # noqa: E731
    for b in range(B):                                                   # every stream has a history, so there are bytes to keep
        ops.online_smooth_group_lag(up(data[b][0][None, :history]), up(data[b][1][None, :history]), group, [b], taps, OMEGA, ITERS, BETA, LAM_NEWEST, lag)
    ops.online_smooth_lag(up(data[2][0][:history]), up(data[2][1][:history]), single, taps, OMEGA, ITERS, BETA, LAM_NEWEST, lag)
    before = [[t[b].cpu().numpy() for t in (group.c, group.q, group.lam)] for b in range(B)]
    order = (0, 2, 3, 0)
    vel = up(np.stack([data[b][0][history:history + 1] for b in order]))
    lam = up(np.stack([data[b][1][history:history + 1] for b in order]))
    ids = torch.tensor([B, 2, -1, 0], dtype=torch.int32, device=dev)    # one past the last stream, a good row, a negative id, a negative count
    seen = torch.tensor([0, history, 5, -3], dtype=torch.int64, device=dev)
    c, p = (torch.full((4, 1, S), 7.25, dtype=torch.float64, device=dev) for _ in range(2))
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                       # noqa: E731
    _lib.check(_lib.lib.mf_online_smooth_group_lag_f64(ptr(vel), ptr(lam), ptr(taps), ptr(ids), ptr(seen), 4, B, 1, S, OMEGA, L, lag, ITERS, BETA,
                                                       LAM_NEWEST, ptr(group.c), ptr(group.q), ptr(group.lam), ptr(c), ptr(p),
                                                       ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    c, p = c.cpu().numpy(), p.cpu().numpy()
    assert (c[[0, 2, 3]] == 7.25).all() and (p[[0, 2, 3]] == 7.25).all()  # their output rows are as they were
    wc, wp = ops.online_smooth_lag(vel[1], lam[1], single, taps, OMEGA, ITERS, BETA, LAM_NEWEST, lag)
    same(c[1], wc.cpu().numpy(), 'c')
    same(p[1], wp.cpu().numpy(), 'p')
    for b in (0, 1, 3):
        for got, want, what in zip((group.c, group.q, group.lam), before[b], 'cql'):
            same(got[b].cpu().numpy(), want, ('state', b, what))
    for got, want, what in zip((group.c, group.q, group.lam), (single.c, single.q, single.lam), 'cql'):
        same(got[2].cpu().numpy(), want.cpu().numpy(), ('the good row', what))


def test_pending_rows_are_each_streams_own(dev):
    from meshflow_amd import ops

    def grouped(state, vel, lam, ids, taps):
        return ops.online_smooth_group_lag(vel, lam, state, ids, taps, OMEGA, ITERS, BETA, LAM_NEWEST, 3)

    import torch
    from meshflow_amd import host
    taps = torch.from_numpy(host.online_taps(OMEGA)).to(dev)
    group, singles = ops.OnlineGroupState(B, S, L, dev), [ops.OnlineState(S, L, dev) for _ in range(B)]
    data = inputs()
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)    # noqa: E731
    for b, frames in enumerate((0, 2, 3, 9)):                            # nothing, fewer than the lag, the lag, past the wrap
        if frames:
            grouped(group, up(data[b][0][None, :frames]), up(data[b][1][None, :frames]), [b], taps)
            ops.online_smooth_lag(up(data[b][0][:frames]), up(data[b][1][:frames]), singles[b], taps, OMEGA, ITERS, BETA, LAM_NEWEST, 3)
    pending = ops.online_pending_group(group, [3, 0, 2, 1], 3)
    assert [int(c.shape[0]) for c, _ in pending] == [3, 0, 3, 2]
    for (c, p), b in zip(pending, (3, 0, 2, 1)):
        wc, wp = ops.online_pending(singles[b], 3)
        same(c.cpu().numpy(), wc.cpu().numpy(), ('c', b))
        same(p.cpu().numpy(), wp.cpu().numpy(), ('p', b))


# ---- the ring ----

STREAMS = 3
GUARD = 64                                                               # elements in front of and behind the ring and the output
FRAMES = {'uint8': (16, 48, 4096 + 16, 1, 15, 17, 4099),                 # bytes: three for the 16-byte path, four for the byte path
          'uint16': (8, 24, 2048 + 8, 1, 9)}                             # elements: 16, 48 and 4112 bytes; 2 and 18 bytes


def carve(torch, dev, content, fill, skew=0):
    """`content`, a (rows, frame) NumPy array, in the middle of a device buffer of `fill`, GUARD elements either side (`skew` more in front):
    (the buffer, the (rows, frame) view of its middle)."""
    rows, frame = content.shape
    host = np.full(2 * GUARD + skew + rows * frame, fill, dtype=content.dtype)
    host[GUARD + skew:GUARD + skew + rows * frame] = content.reshape(-1)
    buf = torch.from_numpy(host).to(dev)
    return buf, buf[GUARD + skew:GUARD + skew + rows * frame].view(rows, frame)


def guards_intact(buf, rows, frame, fill, skew=0):
    host = buf.cpu().numpy()
    return (host[:GUARD + skew] == fill).all() and (host[GUARD + skew + rows * frame:] == fill).all()


@pytest.mark.parametrize('lag', [1, 2, 5])
@pytest.mark.parametrize('dtype', ['uint8', 'uint16'])
def test_ring_exchange_equals_the_model(dev, dtype, lag):
    import torch
    from meshflow_amd import _lib, ops
    tdtype, top = getattr(torch, dtype), np.iinfo(dtype).max
    # stream 1 alone until it has `lag` frames (K = 1, nothing out), then everyone -- only stream 1 hands out: mixed rows --, everyone until
    # all hand out, and a single stream that does
    schedule = [[1]] * lag + [[2, 0, 1]] + [[0, 1, 2], [1, 2, 0]] * lag + [[2]]
    calls = []
    entry = _lib.lib.mf_ring_exchange_u8
    for frame in FRAMES[dtype]:
        for skew in ((0, 1) if frame in (16, 48, 8, 24) else (0,)):          # a `new` whose base is not 16-byte aligned: the byte path at a vector size
            rng = np.random.default_rng(frame * 10 + lag)
            model = rng.integers(0, top + 1, (STREAMS, lag, frame)).astype(dtype)      # whatever the memory held
            ring_buf, ring = carve(torch, dev, model.reshape(STREAMS * lag, frame), 0xA5)
            ring = ring.view(STREAMS, lag, frame)
            seen, kinds = [0] * STREAMS, set()
            for ids in schedule:
                K = len(ids)
                fresh = rng.integers(0, top + 1, (K, frame)).astype(dtype)
                _, new = carve(torch, dev, fresh, 0, skew)
                assert (new.data_ptr() % 16 != 0) == bool(skew)
                rows, M = ring_model.tick_rows(ids, seen, lag)
                kinds.add('all' if M == K else 'none' if M == 0 else 'mixed')
                out = ops.ring_exchange(ring, new, rows, M)
                model, want = ring_model.exchange(model, fresh, rows, M)
                assert tuple(out.shape) == (M, frame) and out.dtype == tdtype
                same(out.cpu().numpy(), want, ('out', frame, skew, ids))
                same(ring.cpu().numpy(), model, ('ring', frame, skew, ids))
                same(new.cpu().numpy(), fresh, ('new is only read', frame, skew, ids))
                for b in ids:
                    seen[b] += 1
            assert kinds == {'all', 'none', 'mixed'} and guards_intact(ring_buf, STREAMS * lag, frame, 0xA5), (frame, kinds)
            calls.append((frame, skew))
    # the output between canaries, through the C ABI (the op allocates its own): every row hands out, M = K = 3
    frame = FRAMES[dtype][2]
    size = frame * np.dtype(dtype).itemsize
    rng = np.random.default_rng(lag)
    held = rng.integers(0, top + 1, (STREAMS, lag, frame)).astype(dtype)
    fresh = rng.integers(0, top + 1, (STREAMS, frame)).astype(dtype)
    ring_buf, ring = carve(torch, dev, held.reshape(STREAMS * lag, frame), 0xA5)
    out_buf, out = carve(torch, dev, np.full((STREAMS, frame), 0x5A, dtype=dtype), 0x5A)
    new = torch.from_numpy(fresh).to(dev)
    rows = np.array([(2, lag - 1, 0), (0, 0, 2), (1, lag // 2, 1)], dtype=np.int32)
    d_rows = torch.from_numpy(rows).to(dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                       # noqa: E731
    _lib.check(entry(ptr(ring), ptr(new), ptr(out), ptr(d_rows), STREAMS, STREAMS, lag, size, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    model, want = ring_model.exchange(held, fresh, rows, STREAMS)
    same(out.cpu().numpy(), want, 'out between canaries')
    same(ring.view(STREAMS, lag, frame).cpu().numpy(), model, 'ring between canaries')
    assert guards_intact(out_buf, STREAMS, frame, 0x5A) and guards_intact(ring_buf, STREAMS * lag, frame, 0xA5)
    assert len(calls) == len(FRAMES[dtype]) + 2


def test_ring_rows_out_of_range_touch_nothing(dev):
    """Through the C ABI, past `ops.ring_exchange`'s host checks: an id, a slot or an out_row out of range."""
    import torch
    from meshflow_amd import _lib
    lag, frame = 2, 48
    rng = np.random.default_rng(3)
    held = rng.integers(0, 256, (STREAMS, lag, frame)).astype(np.uint8)
    fresh = rng.integers(0, 256, (4, frame)).astype(np.uint8)
    ring_buf, ring = carve(torch, dev, held.reshape(STREAMS * lag, frame), 0xA5)
    out_buf, out = carve(torch, dev, np.full((4, frame), 0x5A, dtype=np.uint8), 0x5A)
    new = torch.from_numpy(fresh).to(dev)
    rows = np.array([(STREAMS, 0, 0), (1, lag, 1), (0, 1, 4), (-1, 0, 2)], dtype=np.int32)       # id, slot, out_row past the end; a negative id
    d_rows = torch.from_numpy(rows).to(dev)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())                       # noqa: E731
    _lib.check(_lib.lib.mf_ring_exchange_u8(ptr(ring), ptr(new), ptr(out), ptr(d_rows), 4, STREAMS, lag, frame,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    same(ring.view(STREAMS, lag, frame).cpu().numpy(), held, 'ring')
    assert (out.cpu().numpy() == 0x5A).all() and guards_intact(out_buf, 4, frame, 0x5A) and guards_intact(ring_buf, STREAMS * lag, frame, 0xA5)
    # ... and a good row beside them does its work
    rows[2] = (0, 1, 3)
    _lib.check(_lib.lib.mf_ring_exchange_u8(ptr(ring), ptr(new), ptr(out), ptr(torch.from_numpy(rows).to(dev)), 4, STREAMS, lag, frame,
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    got = out.cpu().numpy()
    same(got[3], held[0, 1], 'the good row out')
    same(ring.view(STREAMS, lag, frame)[0, 1].cpu().numpy(), fresh[2], 'the good row in')
    assert (got[:3] == 0x5A).all()
