"""-m gpu: a P210 (10-bit 4:2:2) pair through the callers that crop every frame they hand out -- `stabilize_scored`, `online_session` (plain,
with lag=2 plus `flush()`, with on_cut='reset', with on_uncovered='limit') and `online_group` -- on tests/online_clips.py's clips: d_y is
the grey clip's levels in the high byte (y = y8 << 8, so `ops.luma(d_y)`, the tracker's input, is y8 itself), d_uv (n, H, W/2, 2) seeded
16-bit noise.

Each output equals, bit for bit, the hand composition: the tracker on `ops.luma(d_y)` (through an NV16 session on y8, whose paths, rectangle
and `covered` flags the P210 session must report bit for bit), a cell table of the report's own paths, `ops.warp_p210`, then
`ops.crop_resize_p210` to the session's rectangle.  The group equals B separate sessions.  (uint16 planes are compared as NumPy arrays.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import luma_clip  # noqa: E402
import tracker_clip  # noqa: E402
from online_clips import (LIMIT_SESSION, SESSION, C, H, R, S, W, grey_clip, limit_stabilizer, part, shaky_clip, to_dev)  # noqa: E402
from tracker_clip import MAX_PER, stabilizer  # noqa: E402

pytestmark = pytest.mark.gpu

SIZE = (96, 65)                                                          # an even width, an odd height


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def pairs_of(g, dev, seed=35):
    """(the P210 pair with y = g << 8, the NV16 pair on g itself) on the device; chroma is noise of the format's own width."""
    uv16 = (luma_clip._noise((len(g), H, W // 2, 2), 65536, seed)).astype(np.uint16)
    uv8 = luma_clip._noise((len(g), H, W // 2, 2), 256, seed + 1).astype(np.uint8)
    y16 = (np.ascontiguousarray(g).astype(np.uint16) << 8).astype(np.uint16)
    return to_dev((y16, uv16), dev), to_dev((np.ascontiguousarray(g), uv8), dev)


@pytest.fixture(scope='module')
def clips(dev):
    return pairs_of(grey_clip(), dev)


def by_hand(pair, report, size, first):
    """The frames a report covers -- the clip's frames first .. first + n - 1 --: `ops.warp_p210` from a cell table of the report's own paths,
    then `ops.crop_resize_p210`."""
    from meshflow_amd import ops
    n = int(report.d_stab.shape[0])
    frames = part(pair, first, first + n)
    table = ops.cell_table(report.d_unstab.reshape(n, S).contiguous(), report.d_stab.reshape(n, S).contiguous(), W, H, R, C)
    warped = ops.warp_p210(frames[0], frames[1], table)
    table.check()
    return ops.crop_resize_p210(*warped, report.rectangle, size=size)


def same_reports(got, want, what):
    assert got.first == want.first and got.lost == want.lost and got.rectangle == want.rectangle, what
    for field in ('d_unstab', 'd_stab', 'covered'):
        tracker_clip.same_bits(getattr(got, field).cpu().numpy(), getattr(want, field).cpu().numpy(), (what, field))


def same_pair(got, want, what):
    for g, w, plane in zip(got, want, ('y', 'uv')):
        tracker_clip.same_bits(g.cpu().numpy(), w.cpu().numpy(), (what, plane))


def run_sessions(s, p210, nv16, blocks, size, flush=False, **kw):
    """Push both pairs through twin sessions block by block; every P210 block is the NV16 session's report and the hand composition."""
    import torch
    from meshflow_amd import ops
    assert torch.equal(ops.luma(p210[0]), nv16[0])                       # the tracker sees the same luma in both sessions
    wide, narrow = s.online_session(output_size=size, **kw), s.online_session(output_size=size, **kw)
    oW, oH = (W, H) if size is None else size
    at, done, outs, reports = 0, 0, [], []                              # frames pushed, frames handed out
    resets = kw.get('on_cut') == 'reset'                                 # (`first` and `seen` count from the last cut then)
    for b in blocks:
        (out_y, out_uv), rep = wide.push(part(p210, at, at + b))
        _, n_rep = narrow.push(part(nv16, at, at + b))
        at += b
        same_reports(rep, n_rep, ('block', at))
        assert wide.last_cuts == narrow.last_cuts and wide.shots == narrow.shots and wide.seen == narrow.seen      # (seen restarts at a cut)
        n = int(rep.d_stab.shape[0])
        assert tuple(out_y.shape) == (n, oH, oW) and tuple(out_uv.shape) == (n, oH, oW // 2, 2)
        assert out_y.dtype == torch.uint16 and out_uv.dtype == torch.uint16 and out_uv.is_cuda
        assert resets or rep.first == done
        if n:
            same_pair((out_y, out_uv), by_hand(p210, rep, size, done), ('by hand', at))
        done += n
        outs.append((out_y, out_uv))
        reports.append(rep)
    if flush:
        (out_y, out_uv), rep = wide.flush()
        _, n_rep = narrow.flush()
        same_reports(rep, n_rep, 'flush')
        same_pair((out_y, out_uv), by_hand(p210, rep, size, done), 'flush by hand')
        outs.append((out_y, out_uv))
        reports.append(rep)
    return outs, reports


@pytest.mark.parametrize('size', [None, SIZE])
def test_a_session_in_blocks(dev, clips, size):
    import torch
    p210, nv16 = clips
    n = int(p210[0].shape[0])
    s = stabilizer(dev)
    outs, reports = run_sessions(s, p210, nv16, (1, 4, n - 5), size, **SESSION)
    # ... and the blocks are one push
    (one_y, one_uv), one = s.online_session(output_size=size, **SESSION).push(p210)
    tracker_clip.same_bits(torch.cat([o[0] for o in outs]).cpu().numpy(), one_y.cpu().numpy(), 'blocks, luma')
    tracker_clip.same_bits(torch.cat([o[1] for o in outs]).cpu().numpy(), one_uv.cpu().numpy(), 'blocks, chroma')
    assert one.rectangle != (0, 0, W - 1, H - 1) and bool(one.covered.any())
    assert one.d_stab.cpu().numpy().tobytes() != one.d_unstab.cpu().numpy().tobytes()              # (something was smoothed)


def test_a_lagged_session_holds_owed_p210_frames_and_flushes_them(dev, clips):
    p210, nv16 = clips
    n = int(p210[0].shape[0])
    outs, reports = run_sessions(stabilizer(dev), p210, nv16, (2, 1, 5, n - 8), SIZE, flush=True, lag=2, **SESSION)
    counts = [int(r.d_stab.shape[0]) for r in reports]
    assert counts[0] == 0 and sum(counts[:-1]) == n - 2 and counts[-1] == 2 and reports[-1].first == n - 2
    assert tuple(outs[0][1].shape) == (0, SIZE[1], SIZE[0] // 2, 2)      # (the first push hands out an empty PAIR with the output's rows)


def test_a_session_that_resets_at_cuts(dev):
    """tests/cuts_clip.py's clip with one cut, at frame 5: both sessions restart there, and the P210 frames are still the hand composition."""
    import cuts_clip
    g = cuts_clip.one_cut()
    p210, nv16 = pairs_of(g, dev, seed=47)
    s = stabilizer(dev)
    run_sessions(s, p210, nv16, (3, 4, len(g) - 7), SIZE, on_cut='reset', **SESSION)
    probe = s.online_session(output_size=SIZE, on_cut='reset', **SESSION)
    probe.push(p210)
    assert list(probe.last_cuts) == [5] and probe.shots == 2


def test_a_session_that_limits_the_path_to_keep_the_crop_covered(dev):
    g = shaky_clip()
    p210, nv16 = pairs_of(g, dev, seed=41)
    s = limit_stabilizer(dev)
    kw = dict(LIMIT_SESSION, on_uncovered='limit')
    outs, reports = run_sessions(s, p210, nv16, (5, len(g) - 5), None, **kw)
    assert all(bool(r.covered.all()) for r in reports)
    # ... which the unlimited session on the same clip does not manage: the limiter had something to do
    _, free = s.online_session(**LIMIT_SESSION).push(p210)
    assert not bool(free.covered.all())


def test_a_group_of_three_streams_equals_three_sessions(dev, clips):
    import torch
    p210, _ = clips
    n = int(p210[0].shape[0])
    s = stabilizer(dev)
    other, _ = pairs_of(shaky_clip()[:n], dev, seed=43)
    backwards, _ = pairs_of(grey_clip()[::-1], dev, seed=45)             # (reversed on the host: torch flips few unsigned types on the device)
    streams = [p210, backwards, other]
    kw = dict(SESSION, output_size=SIZE)
    sessions, group = [s.online_session(**kw) for _ in streams], s.online_group(len(streams), **kw)
    for t in range(n):
        ids = [0, 1, 2] if t % 3 else [2, 0]
        stacked = tuple(torch.cat([streams[b][i][t:t + 1] for b in ids]) for i in range(2))
        (out_y, out_uv), reports = group.push(stacked, None if ids == [0, 1, 2] else ids)
        assert tuple(out_uv.shape) == (len(ids), SIZE[1], SIZE[0] // 2, 2) and len(reports) == len(ids) and out_uv.dtype == torch.uint16
        for r, b in enumerate(ids):
            # stream 1 sits out the ticks the subset leaves it out of: its session is pushed only when the group pushes it
            want_pair, want = sessions[b].push(part(streams[b], t, t + 1))
            same_reports(reports[r], want, ('group', t, b))
            same_pair((out_y[r:r + 1], out_uv[r:r + 1]), want_pair, ('group', t, b))
    assert list(group.seen) == [x.seen for x in sessions]


def test_stabilize_scored_on_a_p210_pair(dev, clips):
    from meshflow_amd import ops
    p210, nv16 = clips
    n = int(p210[0].shape[0])
    s = stabilizer(dev)
    d_y, d_uv = p210
    (out_y, out_uv), scores = s.stabilize_scored((d_y, d_uv), max_per_subframe=MAX_PER, chunk_pairs=5)
    d_disp, hom = s.estimate_motion(ops.luma(d_y), 5, MAX_PER, outliers='device', fit='device')
    want_y, want_uv, _ = s.stabilized_p210_cropped(d_y, d_uv, d_disp, hom)
    same_pair((out_y, out_uv), (want_y, want_uv), 'cropped')
    assert tuple(out_uv.shape) == (n, H, W // 2, 2)
    # the same motion, rectangle and scores as the NV16 clip on y8: the tracker saw the same luma, before the crop and after it
    (n_y, _), n_scores = s.stabilize_scored(nv16, max_per_subframe=MAX_PER, chunk_pairs=5)
    print('p210 scores', scores, 'nv16', n_scores)
    assert len(scores) == 3 and [type(v) for v in scores] == [type(v) for v in n_scores]
    assert scores[2] == n_scores[2]
