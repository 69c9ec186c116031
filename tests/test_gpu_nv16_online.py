"""-m gpu: an NV16 (4:2:2) pair through the three callers that crop every frame they hand out -- `online_session` (with lag=0 and with
lag=3 plus `flush()`), `online_group` and `stabilize_scored` -- on twelve 128 x 97 frames cut from tests/tracker_clip.py's canvas (an odd H:
4:2:2 has no rule about it).  Luma, the rectangle, the `covered` flags, the paths and the cuts are byte for byte those of a grey session on d_y;
chroma is, as in the NV12 session test, the hand composition: `ops.warp_nv16` from a cell table of the report's own paths, then
`ops.crop_resize_nv16` to the session's rectangle."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import luma_clip  # noqa: E402
import tracker_clip  # noqa: E402
from tracker_clip import MAX_PER, SHIFTS, stabilizer  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, R, C, N = 128, 97, 4, 4, 12
S = (R + 1) * (C + 1) * 2
MOVES = SHIFTS + ((-3, 2), (2, -4), (-5, 3), (4, 1), (1, -1), (-2, 2))
SESSION = dict(window=4, iters=6, beta=1.0, crop_margin=0.08, max_per_subframe=MAX_PER)
SIZE = (96, 65)                                                          # an even width, an odd height


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def luma_frames(seed=21, start=(20, 20)):
    big = tracker_clip.canvas(150, 170, seed, boxes=160)
    (ox, oy), frames = start, []
    for dx, dy in ((0, 0),) + MOVES:
        ox, oy = ox - dx, oy - dy
        frames.append(np.ascontiguousarray(big[oy:oy + H, ox:ox + W]))
    assert len(frames) == N
    return np.stack(frames)


@pytest.fixture(scope='module')
def clip(dev):
    """(d_y (N, 97, 128), d_uv (N, 97, 64, 2)) on the device."""
    import torch
    g = luma_frames()
    uv = luma_clip._noise((N, H, W // 2, 2), 256, 35).astype(np.uint8)
    return torch.from_numpy(g).to(dev), torch.from_numpy(np.ascontiguousarray(uv)).to(dev)


def part(pair, lo, hi):
    return tuple(p[lo:hi] for p in pair)


def chroma_by_hand(pair, report, size):
    """The chroma of the frames a report covers: `ops.warp_nv16` from a cell table of the report's own paths, `ops.crop_resize_nv16`."""
    from meshflow_amd import ops
    n = int(report.d_stab.shape[0])
    frames = part(pair, report.first, report.first + n)
    table = ops.cell_table(report.d_unstab.reshape(n, S).contiguous(), report.d_stab.reshape(n, S).contiguous(), W, H, R, C)
    warped = ops.warp_nv16(frames[0], frames[1], table)
    table.check()
    return ops.crop_resize_nv16(*warped, report.rectangle, size=size)


def same_reports(got, want, what):
    assert got.first == want.first and got.lost == want.lost and got.rectangle == want.rectangle, what
    for field in ('d_unstab', 'd_stab', 'covered'):
        tracker_clip.same_bits(getattr(got, field).cpu().numpy(), getattr(want, field).cpu().numpy(), (what, field))


@pytest.mark.parametrize('size', [None, SIZE])
def test_a_session_in_blocks_is_the_grey_session_plus_the_hand_chroma(dev, clip, size):
    import torch
    s = stabilizer(dev)
    kw = dict(SESSION, output_size=size, on_cut='reset')
    grey, pair = s.online_session(**kw), s.online_session(**kw)
    at, outs = 0, []
    for b in (1, 4, N - 5):
        g_out, g_rep = grey.push(clip[0][at:at + b])
        (out_y, out_uv), rep = pair.push(part(clip, at, at + b))
        same_reports(rep, g_rep, ('block', at))
        assert pair.last_cuts == grey.last_cuts and pair.shots == grey.shots and pair.seen == grey.seen == at + b
        tracker_clip.same_bits(out_y.cpu().numpy(), g_out.cpu().numpy(), ('luma', at))
        oW, oH = (W, H) if size is None else size
        assert tuple(out_y.shape) == (b, oH, oW) and tuple(out_uv.shape) == (b, oH, oW // 2, 2) and out_uv.dtype == torch.uint8
        want_y, want_uv = chroma_by_hand(clip, rep, size)
        tracker_clip.same_bits(out_uv.cpu().numpy(), want_uv.cpu().numpy(), ('chroma', at))
        tracker_clip.same_bits(out_y.cpu().numpy(), want_y.cpu().numpy(), ('luma by hand', at))
        outs.append((out_y, out_uv))
        at += b
    # ... and the blocks are one push
    (one_y, one_uv), one = s.online_session(**kw).push(clip)
    tracker_clip.same_bits(torch.cat([o[0] for o in outs]).cpu().numpy(), one_y.cpu().numpy(), 'blocks, luma')
    tracker_clip.same_bits(torch.cat([o[1] for o in outs]).cpu().numpy(), one_uv.cpu().numpy(), 'blocks, chroma')
    assert one.rectangle != (0, 0, W - 1, H - 1) and bool(one.covered.any())
    assert one.d_stab.cpu().numpy().tobytes() != one.d_unstab.cpu().numpy().tobytes()              # (something was smoothed)


def test_a_lagged_session_and_its_flush(dev, clip):
    import torch
    s = stabilizer(dev)
    kw = dict(SESSION, output_size=SIZE, lag=3)
    grey, pair = s.online_session(**kw), s.online_session(**kw)
    at, got, total = 0, [], 0
    for b in (2, 1, 5, N - 8):
        g_out, g_rep = grey.push(clip[0][at:at + b])
        (out_y, out_uv), rep = pair.push(part(clip, at, at + b))
        at += b
        same_reports(rep, g_rep, ('lag', at))
        n = int(rep.d_stab.shape[0])
        assert n == max(0, at - 3 - total) and tuple(out_y.shape) == (n, SIZE[1], SIZE[0]) and tuple(out_uv.shape) == (n, SIZE[1], SIZE[0] // 2, 2)
        assert out_uv.dtype == torch.uint8 and out_uv.is_cuda
        tracker_clip.same_bits(out_y.cpu().numpy(), g_out.cpu().numpy(), ('lag luma', at))
        if n:
            tracker_clip.same_bits(out_uv.cpu().numpy(), chroma_by_hand(clip, rep, SIZE)[1].cpu().numpy(), ('lag chroma', at))
        total += n
        got.append(n)
    assert got[0] == 0 and total == N - 3                                # (the first push hands out an empty PAIR with the output's rows)
    g_out, g_rep = grey.flush()
    (out_y, out_uv), rep = pair.flush()
    same_reports(rep, g_rep, 'flush')
    assert tuple(out_uv.shape) == (3, SIZE[1], SIZE[0] // 2, 2) and rep.first == N - 3
    tracker_clip.same_bits(out_y.cpu().numpy(), g_out.cpu().numpy(), 'flush luma')
    tracker_clip.same_bits(out_uv.cpu().numpy(), chroma_by_hand(clip, rep, SIZE)[1].cpu().numpy(), 'flush chroma')


def test_a_group_of_three_streams_equals_three_sessions(dev, clip):
    import torch
    s = stabilizer(dev)
    d_y, d_uv = clip
    streams = [clip, (d_y.flip(0).contiguous(), d_uv.flip(0).contiguous()),
               (torch.from_numpy(luma_frames(start=(24, 22))).to(dev), d_uv.flip(2).contiguous())]
    kw = dict(SESSION, output_size=SIZE)
    sessions, group = [s.online_session(**kw) for _ in streams], s.online_group(len(streams), **kw)
    for t in range(N):
        ids = [0, 1, 2] if t % 3 else [2, 0]
        stacked = tuple(torch.cat([streams[b][i][t:t + 1] for b in ids]) for i in range(2))
        (out_y, out_uv), reports = group.push(stacked, None if ids == [0, 1, 2] else ids)
        assert tuple(out_uv.shape) == (len(ids), SIZE[1], SIZE[0] // 2, 2) and len(reports) == len(ids)
        for r, b in enumerate(ids):
            # stream 1 sits out the ticks the subset leaves it out of: its session is pushed only when the group pushes it
            (want_y, want_uv), want = sessions[b].push(part(streams[b], t, t + 1))
            same_reports(reports[r], want, ('group', t, b))
            tracker_clip.same_bits(out_y[r:r + 1].cpu().numpy(), want_y.cpu().numpy(), ('group luma', t, b))
            tracker_clip.same_bits(out_uv[r:r + 1].cpu().numpy(), want_uv.cpu().numpy(), ('group chroma', t, b))
    assert list(group.seen) == [x.seen for x in sessions]


def test_stabilize_scored_on_an_nv16_pair(dev, clip):
    s = stabilizer(dev)
    d_y, d_uv = clip
    (out_y, out_uv), scores = s.stabilize_scored((d_y, d_uv), max_per_subframe=MAX_PER, chunk_pairs=5)
    d_disp, hom = s.estimate_motion(d_y, 5, MAX_PER, outliers='device', fit='device')
    want_y, want_uv, _ = s.stabilized_nv16_cropped(d_y, d_uv, d_disp, hom)
    tracker_clip.same_bits(out_y.cpu().numpy(), want_y.cpu().numpy(), 'cropped luma')
    tracker_clip.same_bits(out_uv.cpu().numpy(), want_uv.cpu().numpy(), 'cropped chroma')
    assert tuple(out_uv.shape) == (N, H, W // 2, 2)
    grey, grey_scores = s.stabilize_scored(d_y, max_per_subframe=MAX_PER, chunk_pairs=5)
    tracker_clip.same_bits(out_y.cpu().numpy(), grey.cpu().numpy(), "the grey clip's crop")
    print('nv16 scores', scores, 'grey', grey_scores)
    assert len(scores) == 3 and [type(v) for v in scores] == [type(v) for v in grey_scores]
    assert np.array(scores[:2], np.float32).tobytes() == np.array(grey_scores[:2], np.float32).tobytes() and scores[2] == grey_scores[2]
