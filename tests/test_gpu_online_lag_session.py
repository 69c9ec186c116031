"""`online_session(lag=k)` and `OnlineSession.flush()` against the composition of the ops written out by hand -- `ops.online_smooth_lag` and
`ops.online_pending` into the cell table, the warp and the crop-resize -- on tests/online_clips.py's ten 128 x 96 frames: every form,
blocks against one push, pushes that hand out nothing, the path limit, cuts, a refused push, reset, and the promise that lag=0 is the session
without the keyword."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuts_clip  # noqa: E402
import cuts_model as cm  # noqa: E402
from online_clips import (BETA, GUARD, ITERS, LIMIT_SESSION, MARGIN, RISE, SESSION, WINDOW, C, H, K, R, S, W, forms, grey_clip,  # noqa: E402
                          limit_stabilizer, part, rectangle, same_frames, shaky_clip, to_dev)
from tracker_clip import MAX_PER, same_bits, stabilizer  # noqa: E402

pytestmark = pytest.mark.gpu

N, LAG = 10, 2


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def run(session, clip, blocks, flush=True):
    """The clip pushed in blocks of these sizes and, then, flushed: the list of (frames, report)."""
    at, parts = 0, []
    for b in blocks:
        parts.append(session.push(part(clip, at, at + b)))
        at += b
    if flush:
        parts.append(session.flush())
    return parts


def joined(parts):
    """(frames, report) of several, in order: planes and report tensors concatenated, `first` the first part's, `lost` joined."""
    import torch
    from meshflow_amd import online
    outs, reports = [p[0] for p in parts], [p[1] for p in parts]
    out = tuple(torch.cat([o[i] for o in outs]) for i in range(2)) if isinstance(outs[0], tuple) else torch.cat(outs)
    return out, online.OnlineReport(reports[0].first, torch.cat([r.d_unstab for r in reports]), torch.cat([r.d_stab for r in reports]),
                                    reports[0].rectangle, torch.cat([r.covered for r in reports]), [t for r in reports for t in r.lost])


def same_result(got, want, what):
    same_frames(got[0], want[0], (what, 'frames'))
    for field in ('d_unstab', 'd_stab', 'covered'):
        same_bits(getattr(got[1], field).cpu().numpy(), getattr(want[1], field).cpu().numpy(), (what, field))
    assert got[1].first == want[1].first and got[1].lost == want[1].lost and got[1].rectangle == want[1].rectangle, what


def luma_of(clip):
    import torch
    from meshflow_amd import ops
    if isinstance(clip, tuple):
        return ops.luma(clip[0]) if clip[0].dtype == torch.uint16 else clip[0]
    return ops.luma(clip) if ops.luma_source(clip) is not None else clip


def paths_by_hand(s, clip, lag, window=WINDOW):
    """(c, p) of all the clip's frames -- what the smoother hands out, then what is pending -- from the ops, one block from frame 0."""
    import torch
    from meshflow_amd import host, ops
    luma = luma_of(clip)
    dev, n = luma.device, luma.shape[0]
    early, late, offsets, kmax, hom, info = s.device_tracker(MAX_PER, 'device', 'device').track_stacks_resident(luma[:-1], luma[1:], 32)
    assert ops.fit_check(info) is None
    _, vel, status = ops.vertex_motion(early, late, offsets, hom, kmax, W, H, R, C, s.feature_ellipse_row_count, s.feature_ellipse_col_count)
    assert int(status.item()) == 0
    lam_newest = float(host.adaptive_weights(1, W, H, 0, np.identity(3)[None])[0])
    lam = np.concatenate([[lam_newest], host.adaptive_weights(n - 1, W, H, 0, hom.cpu().numpy())])
    state = ops.OnlineState(S, window, dev)
    block = torch.cat([torch.zeros((1, S), dtype=torch.float32, device=dev), vel.reshape(n - 1, S)])
    taps = torch.from_numpy(host.online_taps(s.temporal_smoothing_radius)).to(dev)
    c, p = ops.online_smooth_lag(block, torch.from_numpy(lam).to(dev), state, taps, s.temporal_smoothing_radius, ITERS, BETA, lam_newest, lag)
    pc, pp = ops.online_pending(state, lag)
    assert c.shape[0] == n - lag and pc.shape[0] == lag
    return torch.cat([c, pc]), torch.cat([p, pp])


def frames_by_hand(s, clip, c, p, rect):
    """(frames, covered) of paths (c, p): the cell table, the form's warp, the crop-resize to the fixed rectangle."""
    import torch
    from meshflow_amd import ops
    table = ops.cell_table(c, p, W, H, R, C)
    if isinstance(clip, tuple):
        p010 = clip[0].dtype == torch.uint16
        warped = (ops.warp_p010 if p010 else ops.warp_nv12)(clip[0], clip[1], table)
        out = (ops.crop_resize_p010 if p010 else ops.crop_resize_nv12)(*warped, rect)
    else:
        out = ops.crop_resize(ops.warp(clip, table, s.color_outside_image_area_bgr), rect)
    table.check()
    crop = table.crop
    left, top, right, bottom = rect
    return out, (crop[:, 0] <= left) & (crop[:, 1] <= top) & (crop[:, 2] >= right) & (crop[:, 3] >= bottom)


def by_hand(s, clip, lag, window=WINDOW):
    from meshflow_amd import online
    c, p = paths_by_hand(s, clip, lag, window)
    out, covered = frames_by_hand(s, clip, c, p, rectangle(MARGIN))
    shape = (c.shape[0], R + 1, C + 1, 2)
    return out, online.OnlineReport(0, c.view(shape), p.view(shape), rectangle(MARGIN), covered, [])


@pytest.fixture(scope='module')
def clips(dev):
    return {name: to_dev(clip, dev) for name, clip in forms(grey_clip()).items()}


def count(frames):
    return int((frames[0] if isinstance(frames, tuple) else frames).shape[0])


def is_empty_result(out, report, clip, first):
    import torch
    for o, src in zip(out if isinstance(out, tuple) else (out,), clip if isinstance(clip, tuple) else (clip,)):
        assert o.is_cuda and o.dtype == src.dtype and tuple(o.shape) == (0,) + tuple(src.shape[1:])
    assert isinstance(out, tuple) == isinstance(clip, tuple)
    assert report.first == first and report.rectangle == rectangle(MARGIN) and report.lost == []
    for t in (report.d_unstab, report.d_stab):
        assert t.is_cuda and t.dtype == torch.float64 and tuple(t.shape) == (0, R + 1, C + 1, 2)
    assert report.covered.is_cuda and report.covered.dtype == torch.bool and tuple(report.covered.shape) == (0,)


def test_lag_0_is_the_session_without_the_keyword(dev, clips):
    s = stabilizer(dev)
    for name in ('grey', 'nv12'):
        clip = clips[name]
        plain, zero = s.online_session(**SESSION), s.online_session(lag=0, **SESSION)
        assert zero.lag == plain.lag == 0
        for lo, hi in ((0, 1), (1, 4), (4, N)):
            same_result(zero.push(part(clip, lo, hi)), plain.push(part(clip, lo, hi)), (name, lo))
            assert zero.pending == 0 and zero.emitted == zero.seen == hi
        for session in (plain, zero):
            out, report = session.flush()
            is_empty_result(out, report, clip, N)            # (`first` is `emitted` where nothing came out)
            assert session.seen == 0 and session.pending == 0
        same_result(s.stabilize_online(clip, lag=0, **SESSION), s.stabilize_online(clip, **SESSION), (name, 'stabilize_online'))


@pytest.mark.parametrize('name', ['grey', 'bgr', 'nv12'])
def test_push_and_flush_equal_the_hand_composition_and_blocks_equal_one_push(dev, clips, name):
    s, clip = stabilizer(dev), clips[name]
    want = by_hand(s, clip, LAG)
    session = s.online_session(lag=LAG, **SESSION)
    (out, report), (tail, tail_report) = run(session, clip, [N])
    assert count(out) == report.d_stab.shape[0] == N - LAG and count(tail) == tail_report.d_stab.shape[0] == LAG
    assert report.first == 0 and tail_report.first == N - LAG
    assert session.seen == session.pending == session.emitted == 0       # (flush leaves the session as reset() does)
    same_result(joined([(out, report), (tail, tail_report)]), want, name)
    assert report.d_stab.cpu().numpy().tobytes() != report.d_unstab.cpu().numpy().tobytes()
    # look-ahead changes the path, not the unstabilized one
    plain = s.online_session(**SESSION).push(clip)[1]
    same_bits(want[1].d_unstab.cpu().numpy(), plain.d_unstab.cpu().numpy(), 'd_unstab')
    assert want[1].d_stab[:N - LAG].cpu().numpy().tobytes() != plain.d_stab[:N - LAG].cpu().numpy().tobytes()
    # blocks (1, 3, rest) and flush: the first push hands out nothing
    session = s.online_session(lag=LAG, **SESSION)
    parts, at = [], 0
    for b, first, m in ((1, 0, 0), (3, 0, 2), (N - 4, 2, N - 4)):
        out, report = session.push(part(clip, at, at + b))
        at += b
        assert report.first == first and count(out) == report.d_stab.shape[0] == report.covered.shape[0] == m
        assert session.seen == at and session.pending == min(LAG, at) and session.emitted == at - min(LAG, at)
        parts.append((out, report))
    is_empty_result(*parts[0], clip, 0)            # (the crop-resize scales back to the frame size: the input's trailing shape)
    parts.append(session.flush())
    same_result(joined(parts), want, (name, 'blocks'))


@pytest.mark.parametrize('name', ['bgr16', 'bgra', 'p010'])
def test_the_other_forms(dev, clips, name):
    s, clip = stabilizer(dev), clips[name]
    parts = run(s.online_session(lag=LAG, **SESSION), clip, [N])
    assert [count(p[0]) for p in parts] == [N - LAG, LAG]
    got = joined(parts)
    for o, src in zip(got[0] if isinstance(clip, tuple) else (got[0],), clip if isinstance(clip, tuple) else (clip,)):
        assert o.dtype == src.dtype and o.shape == src.shape
    same_result(got, by_hand(s, clip, LAG), name)


def test_a_first_push_of_one_frame_hands_out_nothing(dev, clips):
    s = stabilizer(dev)
    for name in ('grey', 'bgr', 'nv12', 'p010'):
        clip = clips[name]
        session = s.online_session(lag=LAG, **SESSION)
        out, report = session.push(part(clip, 0, 1))
        is_empty_result(out, report, clip, 0)
        assert session.seen == session.pending == 1 and session.emitted == 0
    # with another output size, that size
    session = s.online_session(lag=LAG, output_size=(96, 64), **SESSION)
    out, _ = session.push(clips['bgr'][:2])
    assert tuple(out.shape) == (0, 64, 96, 3) and out.dtype == clips['bgr'].dtype
    out, _ = session.push(clips['bgr'][2:3])
    assert tuple(out.shape) == (1, 64, 96, 3)
    session = s.online_session(lag=LAG, output_size=(96, 64), **SESSION)
    out, _ = session.push(part(clips['nv12'], 0, 2))
    assert [tuple(o.shape) for o in out] == [(0, 64, 96), (0, 32, 48, 2)]
    out, _ = session.push(part(clips['nv12'], 2, 3))
    assert [tuple(o.shape) for o in out] == [(1, 64, 96), (1, 32, 48, 2)]
    # the caller's buffers are free once push returns: the held frames are the session's own
    mine = clips['grey'][:3].clone()
    session = s.online_session(lag=LAG, **SESSION)
    session.push(mine[:2])
    mine[:2] = 0
    got = joined([session.push(clips['grey'][2:]), session.flush()])
    same_result(got, by_hand(s, clips['grey'], LAG), 'buffers reused')


def test_the_largest_lag(dev, clips):
    s, clip = stabilizer(dev), clips['grey']
    lag = WINDOW - 1
    want = by_hand(s, clip, lag)
    parts = run(s.online_session(lag=lag, **SESSION), clip, [N])
    assert [count(p[0]) for p in parts] == [N - lag, lag]
    same_result(joined(parts), want, 'one push')
    parts = run(s.online_session(lag=lag, **SESSION), clip, [2, 1, 1, 1, 5])
    assert [count(p[0]) for p in parts] == [0, 0, 1, 1, 5, 3]
    same_result(joined(parts), want, 'blocks')
    assert want[1].d_stab.cpu().numpy().tobytes() != by_hand(s, clip, LAG)[1].d_stab.cpu().numpy().tobytes()


def test_the_path_limit_runs_on_the_frames_handed_out(dev):
    """The path-limit suite's shaky clip, stabilizer and session (tests/online_clips.py): the lagged session with 'limit' against
    `ops.path_limit` applied by hand to what the lagged session without it hands out, the step carried from the push into the flush."""
    import torch
    from meshflow_amd import ops
    s = limit_stabilizer(dev)
    clip = torch.from_numpy(shaky_clip()).to(dev)
    n, session_kw = clip.shape[0], LIMIT_SESSION
    plain = run(s.online_session(lag=LAG, **session_kw), clip, [n])
    rect = plain[0][1].rectangle
    assert [count(p[0]) for p in plain] == [n - LAG, LAG] and rect == (10, 7, 117, 88)
    want_frames, want_k, want_p, want_covered, k_prev = [], [], [], [], None
    for lo, hi, (_, report) in ((0, n - LAG, plain[0]), (n - LAG, n, plain[1])):
        c, p = report.d_unstab.reshape(hi - lo, -1), report.d_stab.reshape(hi - lo, -1)
        p, k = ops.path_limit(c, p, W, H, R, C, rect, K, GUARD, RISE, k_prev)
        k_prev = k[-1:]
        out, covered = frames_by_hand(s, clip[lo:hi], c, p, rect)
        want_frames.append(out), want_k.append(k), want_p.append(p), want_covered.append(covered)
    for blocks in ([n], [1, 3, n - 4]):
        session = s.online_session(lag=LAG, on_uncovered='limit', **session_kw)
        at, parts, ks = 0, [], []
        for b in blocks:
            parts.append(session.push(clip[at:at + b]))
            ks.append(session.last_limit)
            assert tuple(session.last_limit.shape) == (count(parts[-1][0]),) and session.last_limit.dtype == torch.int32
            at += b
        parts.append(session.flush())
        ks.append(session.last_limit)
        assert tuple(session.last_limit.shape) == (LAG,) and session._k_prev is None
        out, report = joined(parts)
        steps = torch.cat(ks).cpu().numpy()
        print('k', steps.tolist(), 'covered', report.covered.cpu().numpy().astype(int).tolist())
        same_bits(steps, torch.cat(want_k).cpu().numpy(), ('k', blocks))
        same_bits(report.d_stab.cpu().numpy().reshape(n, -1), torch.cat(want_p).cpu().numpy(), ('d_stab', blocks))
        same_bits(report.d_unstab.cpu().numpy(), torch.cat([p[1].d_unstab for p in plain]).cpu().numpy(), ('d_unstab', blocks))
        same_bits(report.covered.cpu().numpy(), torch.cat(want_covered).cpu().numpy(), ('covered', blocks))
        same_bits(out.cpu().numpy(), torch.cat(want_frames).cpu().numpy(), ('frames', blocks))
        assert (np.diff(steps) <= RISE).all()               # (across the push and the flush too: the step is carried)


def test_a_cut_flushes_the_old_shot_in_front_of_the_new_one(dev):
    """tests/cuts_clip.py's clip of two scenes, the cut at frame 5 (tests/test_gpu_online_cuts.py builds its own the same way)."""
    import torch
    assert (cuts_clip.W, cuts_clip.H) == (W, H)
    s = stabilizer(dev)
    clip = torch.from_numpy(cuts_clip.one_cut()).to(dev)
    want_parts = []
    for lo, hi in ((0, 5), (5, N)):
        want_parts += run(s.online_session(lag=LAG, **SESSION), clip[lo:hi], [hi - lo])
    assert [count(p[0]) for p in want_parts] == [3, 2, 3, 2]
    want = joined(want_parts)
    # one push: the first shot whole (3 handed out + 2 flushed at the cut), 3 of the second; the flush has the other 2
    session = s.online_session(lag=LAG, on_cut='reset', **SESSION)
    out, report = session.push(clip)
    assert session.last_cuts == [5] and session.shots == 2 and session.seen == 5 and session.pending == LAG and session.emitted == 3
    assert count(out) == report.d_stab.shape[0] == 8 and report.first == 0
    tail = session.flush()
    assert count(tail[0]) == 2 and tail[1].first == 3 and session.seen == 0
    same_result(joined([(out, report), tail]), want, 'one push')
    c = want[1].d_unstab.cpu().numpy()
    assert c[5].tobytes() == c[0].tobytes() and c[4].tobytes() != c[0].tobytes()           # the path starts again at the cut
    # blocks: the cut inside a block, and between two
    for blocks, counts, firsts in (((3, 4, 3), [1, 2 + 2 + 0, 3, 2], [0, 1, 0, 3]), ((5, 5), [3, 2 + 3, 2], [0, 3, 3])):
        parts = run(s.online_session(lag=LAG, on_cut='reset', **SESSION), clip, blocks)
        assert [count(p[0]) for p in parts] == counts and [p[1].first for p in parts] == firsts, blocks
        same_result(joined(parts), want, blocks)


def one_cut_and_a_lost_pair():
    """tests/cuts_clip.py's clip with the cut at frame 5, the pixels of every tile of frame 8 sorted: its signature is frame 8's, so no cut is
    seen there, and too few features lead from it to frame 9."""
    g = cuts_clip.one_cut()
    rows, cols = cm.tile_edges(H), cm.tile_edges(W)
    for i in range(4):
        for j in range(4):
            tile = g[8, rows[i]:rows[i + 1], cols[j]:cols[j + 1]]
            tile[...] = np.sort(tile.reshape(-1)).reshape(tile.shape)
    assert cm.find_cuts(g)[0] == [5]
    return g


def test_a_refused_push_leaves_the_held_frames_as_they_were(dev):
    """on_lost='raise' under on_cut='reset' with frames pending: the push hands out frames, flushes the old shot at the cut and resets,
    then meets a pair that cannot be fitted (tests/test_gpu_online_cuts.py's device) -- and the session, held pixels, `emitted` and all, is
    where it was; a good push afterwards gives the bytes of a session that never saw the bad one."""
    import torch
    s = stabilizer(dev)
    clip = torch.from_numpy(one_cut_and_a_lost_pair()).to(dev)
    kw = dict(SESSION, lag=LAG, on_cut='reset', on_lost='raise', on_uncovered='limit')

    def snapshot(session):
        return (session.seen, session.emitted, session.pending, session.shots, int(session._k_prev.item()), session._held[0].cpu().numpy().tobytes(),
                session._last_luma.cpu().numpy().tobytes(), session._last_sig.cpu().numpy().tobytes(),
                [t.cpu().numpy().tobytes() for t in (session.state.c, session.state.q, session.state.lam)])

    session, other = s.online_session(**kw), s.online_session(**kw)
    for one in (session, other):
        out, _ = one.push(clip[:4])
        assert count(out) == 2 and one.pending == 2
    before = snapshot(session)
    with pytest.raises(ValueError, match='fewer than 4 features could be tracked'):
        session.push(clip[4:])
    assert snapshot(session) == before == snapshot(other)
    got, want = session.push(clip[4:5]), other.push(clip[4:5])
    assert count(got[0]) == 1 and got[1].first == 2
    same_result(got, want, 'after the refused push')
    same_bits(session.last_limit.cpu().numpy(), other.last_limit.cpu().numpy(), 'k')
    same_result(session.flush(), other.flush(), 'flush')
    # without cuts the refusal comes before anything has changed
    session = s.online_session(**dict(kw, on_cut='ignore', on_uncovered='report', cut_threshold=1.0))
    g2 = grey_clip()
    g2[5] = 128
    clip2 = torch.from_numpy(g2).to(dev)
    session.push(clip2[:4])
    held = session._held[0].cpu().numpy().tobytes()
    with pytest.raises(ValueError, match='fewer than 4 features could be tracked'):
        session.push(clip2[4:])
    assert (session.seen, session.emitted, session.pending) == (4, 2, 2) and session._held[0].cpu().numpy().tobytes() == held


@pytest.mark.parametrize('name', ['nv12', 'p010'])
def test_a_refused_push_restores_both_planes(dev, name):
    """The refused push above on a 4:2:0 pair, where the lag, the cut and the limiter all carry state at once: everything a shot carries,
    BOTH planes of the held frames included, is where it was, and a good push and the flush afterwards give the bytes -- frames and
    `last_limit` -- of a twin session that never saw the bad push."""
    s = stabilizer(dev)
    clip = to_dev(forms(one_cut_and_a_lost_pair())[name], dev)
    kw = dict(SESSION, lag=LAG, on_cut='reset', on_lost='raise', on_uncovered='limit')

    def snapshot(session):
        assert len(session._held) == 2
        return (session.seen, session.emitted, session.pending, session.shots, int(session._k_prev.item()),
                [plane.cpu().numpy().tobytes() for plane in session._held], session._last_luma.cpu().numpy().tobytes(),
                session._last_sig.cpu().numpy().tobytes(), [t.cpu().numpy().tobytes() for t in (session.state.c, session.state.q, session.state.lam)])

    session, twin = s.online_session(**kw), s.online_session(**kw)
    for one in (session, twin):
        out, _ = one.push(part(clip, 0, 4))
        assert count(out) == 2 and one.pending == 2
    before = snapshot(session)
    assert [len(b) for b in before[5]] == [clip[0][:2].numel() * clip[0].element_size(), clip[1][:2].numel() * clip[1].element_size()]
    limit_before = session.last_limit.cpu().numpy().tobytes()
    with pytest.raises(ValueError, match='fewer than 4 features could be tracked'):
        session.push(part(clip, 4, N))
    assert snapshot(session) == before == snapshot(twin)
    assert session.last_limit.cpu().numpy().tobytes() == limit_before                    # (a push that raises leaves `last_limit` too)
    got, want = session.push(part(clip, 4, 5)), twin.push(part(clip, 4, 5))
    assert count(got[0]) == 1 and got[1].first == 2
    same_result(got, want, (name, 'after the refused push'))
    same_bits(session.last_limit.cpu().numpy(), twin.last_limit.cpu().numpy(), (name, 'k'))
    same_result(session.flush(), twin.flush(), (name, 'flush'))
    same_bits(session.last_limit.cpu().numpy(), twin.last_limit.cpu().numpy(), (name, 'k of the flush'))
    assert tuple(session.last_limit.shape) == (LAG,)


def test_reset_drops_the_pending_frames(dev, clips):
    s, clip = stabilizer(dev), clips['grey']
    session = s.online_session(lag=LAG, **SESSION)
    out, _ = session.push(clip[3:8])
    assert count(out) == 3 and (session.seen, session.emitted, session.pending) == (5, 3, 2)
    session.reset()
    assert (session.seen, session.emitted, session.pending) == (0, 0, 0) and session._held is None
    out, report = session.flush()
    is_empty_result(out, report, clip, 0)
    same_result(joined(run(session, clip, [N])), by_hand(s, clip, LAG), 'after reset')


def test_stabilize_online_returns_the_whole_clip(dev, clips):
    s = stabilizer(dev)
    for name in ('grey', 'nv12'):
        clip = clips[name]
        out, report = s.stabilize_online(clip, lag=LAG, **SESSION)
        assert count(out) == N and report.first == 0 and tuple(report.d_stab.shape) == (N, R + 1, C + 1, 2) and tuple(report.covered.shape) == (N,)
        same_result((out, report), by_hand(s, clip, LAG), name)


def test_refusals(dev, clips):
    s = stabilizer(dev)
    for lag in (True, 1.0, -1, WINDOW):
        with pytest.raises(ValueError, match=r'lag must be an int in 0 \.\. window - 1 = %d' % (WINDOW - 1)):
            s.online_session(lag=lag, **SESSION)
    with pytest.raises(ValueError, match='flush before the first push'):
        s.online_session(lag=LAG, **SESSION).flush()
