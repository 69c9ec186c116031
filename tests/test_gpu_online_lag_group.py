"""`MeshFlowStabilizer.online_lag_group` against one `online_session(lag=k)` per stream pushed the same frames one at a time and flushed at
the end, byte for byte in every field of the contract -- per frame handed out: the pixels, d_unstab, d_stab, covered, the limiter's k and the
tick it came out at; per push: first, lost, how many frames came out, the cut decision and distance, shots, seen and pending --: three
streams of 128 x 96 frames (tests/online_clips.py) in the grey, BGR, NV12 and P210 forms, every stream per tick and subsets in turning order,
a reset mid-stream, the path limiter, a cut and a lost pair on one stream alone; the refusals of `push` and `flush`; and the library calls
of a steady tick, which do not grow with the streams pushed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuts_clip  # noqa: E402
import luma_clip  # noqa: E402
import tracker_clip  # noqa: E402
from online_clips import H, LIMIT_SESSION, SESSION, W, forms, grey_clip, limit_stabilizer, part, planes, shaky_clip, to_dev  # noqa: E402
from tracker_clip import stabilizer  # noqa: E402

pytestmark = pytest.mark.gpu

B, TICKS = 3, 10
EVERYONE = [[0, 1, 2]] * TICKS
FRAME_FIELDS = ('frames', 'd_unstab', 'd_stab', 'covered', 'k', 'tick')
PUSH_FIELDS = ('first', 'lost', 'rectangle', 'count', 'cut', 'distance', 'shots', 'seen', 'pending')


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def in_form(g, name):
    if name == 'p210':                                                   # 4:2:2, 16 bits: chroma with luma's rows
        uv = (luma_clip._noise((len(g), H, W // 2, 2), 1024, 37).astype(np.uint16)) << 6
        return luma_clip.p010(g)[0], uv
    return forms(g)[name]


def streams_of(dev, name, middle=None):
    """The three streams in form `name`: `grey_clip()`, the same frames reversed (or `middle`), `shaky_clip()[:10]`."""
    g = grey_clip()
    return [to_dev(in_form(np.ascontiguousarray(clip), name), dev) for clip in (g, g[::-1] if middle is None else middle, shaky_clip()[:TICKS])]


def frame_of(clip, t):
    return part(clip, t, t + 1)


def stacked(frames):
    import torch
    return tuple(torch.cat(p) for p in zip(*frames)) if isinstance(frames[0], tuple) else torch.cat(frames)


class Records:
    """frames[b]: the frames stream b was handed, in order, each a dict of FRAME_FIELDS; pushes[tick, b]: a dict of PUSH_FIELDS."""

    def __init__(self, streams):
        self.frames, self.pushes = [[] for _ in range(streams)], {}

    def take(self, tick, b, out, report, k, **push):
        """`out`, `report`, `k`: what stream b got at `tick` -- 0 or more frames."""
        n = int(report.d_stab.shape[0])
        assert n == int(report.d_unstab.shape[0]) == int(report.covered.shape[0]) == int(planes(out)[0].shape[0]) and (k is None or int(k.shape[0]) == n)
        host = [t.cpu().numpy() for t in (report.d_unstab, report.d_stab, report.covered)]
        pixels, k = planes(out), None if k is None else k.cpu().numpy()
        for j in range(n):
            self.frames[b].append(dict(frames=[p[j] for p in pixels], d_unstab=host[0][j], d_stab=host[1][j], covered=host[2][j],
                                       k=None if k is None else k[j], tick=tick))
        self.pushes[tick, b] = dict(first=report.first, lost=list(report.lost), rectangle=report.rectangle, count=n, **push)


def through_sessions(s, clips, schedule, lag, resets=(), **kw):
    sessions, at, rec = [s.online_session(lag=lag, **kw) for _ in clips], [0] * len(clips), Records(len(clips))
    for tick, ids in enumerate(schedule):
        for b in ids:
            if (tick, b) in resets:
                sessions[b].reset()
            x = sessions[b]
            out, report = x.push(frame_of(clips[b], at[b]))
            at[b] += 1
            d = x.last_cut_distances
            assert x.last_cuts in ([], [0])
            rec.take(tick, b, out, report, x.last_limit, cut=x.last_cuts == [0], distance=None if d is None else int(d[0]), shots=x.shots,
                     seen=x.seen, pending=x.pending)
    for b, x in enumerate(sessions):
        out, report = x.flush()
        rec.take('flush', b, out, report, x.last_limit, cut=False, distance=None, shots=x.shots, seen=x.seen, pending=x.pending)
    return rec


def through_a_group(s, clips, schedule, lag, resets=(), **kw):
    group, at, rec = s.online_lag_group(len(clips), lag, **kw), [0] * len(clips), Records(len(clips))
    assert group.pending == [0] * len(clips) and group.lag == lag

    def split(tick, ids, out, reports, **push):
        assert len(reports) == len(group.last_counts) == len(ids)
        lo = 0
        for r, b in enumerate(ids):
            n = group.last_counts[r]
            k = None if group.last_limit is None else group.last_limit[lo:lo + n]
            rec.take(tick, b, part(out, lo, lo + n), reports[r], k, shots=group.shots[b], seen=group.seen[b], pending=group.pending[b],
                     **{name: values[r] for name, values in push.items()})
            lo += n
        assert lo == int(planes(out)[0].shape[0]) and (group.last_limit is None or int(group.last_limit.shape[0]) == lo)

    for tick, ids in enumerate(schedule):
        for b in ids:
            if (tick, b) in resets:
                group.reset(b)
        out, reports = group.push(stacked([frame_of(clips[b], at[b]) for b in ids]), None if ids == list(range(len(clips))) else ids)
        for b in ids:
            at[b] += 1
        d = group.last_cut_distances
        split(tick, ids, out, reports, cut=[r in group.last_cuts for r in range(len(ids))],
              distance=[None if d is None else int(d[r]) for r in range(len(ids))])
    everyone = list(range(len(clips)))
    out, reports = group.flush()
    split('flush', everyone, out, reports, cut=[False] * len(clips), distance=[None] * len(clips))
    assert group.pending == group.seen == [0] * len(clips)
    return rec


def same_records(got, want, what):
    assert sorted(got.pushes, key=str) == sorted(want.pushes, key=str), what
    for key in want.pushes:
        for field in PUSH_FIELDS:
            g, w = got.pushes[key][field], want.pushes[key][field]
            assert g == w and type(g) is type(w), (what, key, field, g, w)
    for b, (mine, theirs) in enumerate(zip(got.frames, want.frames)):
        assert len(mine) == len(theirs), (what, b, len(mine), len(theirs))
        for t, (g, w) in enumerate(zip(mine, theirs)):
            assert len(g['frames']) == len(w['frames']) and g['tick'] == w['tick'], (what, b, t, g['tick'], w['tick'])
            for a, c in zip(g['frames'], w['frames']):
                tracker_clip.same_bits(a, c, (what, b, t, 'frames'))
            for field in ('d_unstab', 'd_stab', 'covered'):
                assert g[field].dtype == w[field].dtype
                tracker_clip.same_bits(np.asarray(g[field]), np.asarray(w[field]), (what, b, t, field))
            assert (g['k'] is None) == (w['k'] is None) and (g['k'] is None or int(g['k']) == int(w['k'])), (what, b, t, g['k'], w['k'])


def compare(s, clips, schedule, lag, what, resets=(), **kw):
    want = through_sessions(s, clips, schedule, lag, resets, **kw)
    got = through_a_group(s, clips, schedule, lag, resets, **kw)
    same_records(got, want, what)
    return got


@pytest.mark.parametrize('lag', [1, 3])
@pytest.mark.parametrize('name', ['grey', 'bgr', 'nv12'])
def test_every_stream_per_tick_equals_three_lagged_sessions(dev, name, lag):
    got = compare(stabilizer(dev), streams_of(dev, name), EVERYONE, lag, (name, lag), **SESSION)
    for b in range(B):
        # every frame came out once, in order, `lag` ticks after its own; the last `lag` at the flush
        assert [f['tick'] for f in got.frames[b]] == list(range(lag, TICKS)) + ['flush'] * lag
        assert [got.pushes[t, b]['count'] for t in range(TICKS)] == [0] * lag + [1] * (TICKS - lag) and got.pushes['flush', b]['count'] == lag
        assert [got.pushes[t, b]['first'] for t in range(TICKS)] == [0] * lag + list(range(TICKS - lag)) and got.pushes['flush', b]['first'] == TICKS - lag
        assert [got.pushes[t, b]['pending'] for t in range(TICKS)] == list(range(1, lag + 1)) + [lag] * (TICKS - lag)
    last = [got.frames[b][-1] for b in range(B)]
    assert len({f['d_unstab'].tobytes() for f in last}) == B and all(f['d_stab'].tobytes() != f['d_unstab'].tobytes() for f in last)


def test_a_422_pair_of_16_bit_planes(dev):
    got = compare(stabilizer(dev), streams_of(dev, 'p210'), EVERYONE, 3, 'p210', **SESSION)
    assert all(len(got.frames[b]) == TICKS and [p.dtype for p in got.frames[b][0]['frames']] == [np.uint16, np.uint16] for b in range(B))
    assert got.frames[0][0]['frames'][0].shape == (got.frames[0][0]['frames'][1].shape[0], got.frames[0][0]['frames'][1].shape[1] * 2)


@pytest.mark.parametrize('lag', [1, 3])
def test_subsets_in_any_order_equal_the_sessions(dev, lag):
    # stream 2 joins at tick 3, stream 1 skips ticks 5 and 6, and the order of the ids turns with the tick
    schedule = []
    for tick in range(TICKS):
        ids = [b for b in range(B) if not (b == 2 and tick < 3) and not (b == 1 and tick in (5, 6))]
        schedule.append(ids[tick % len(ids):] + ids[:tick % len(ids)])
    assert [len(ids) for ids in schedule] == [2, 2, 2, 3, 3, 2, 2, 3, 3, 3] and schedule[4] == [1, 2, 0] and schedule[5] == [2, 0]
    got = compare(stabilizer(dev), streams_of(dev, 'grey'), schedule, lag, ('subsets', lag), **SESSION)
    # a tick the stream sat out does not count: stream 1's frame 5 - lag comes out at tick 7, its first after the gap
    assert got.pushes[3, 2]['first'] == 0 and got.pushes[3, 2]['count'] == 0 and got.pushes[3 + lag, 2]['count'] == 1
    assert got.pushes[7, 1]['first'] == 5 - lag and got.pushes[7, 1]['count'] == 1 and got.pushes[9, 0]['first'] == 9 - lag
    assert [len(got.frames[b]) for b in range(B)] == [10, 8, 7]
    # ticks in which some rows hand a frame out and some do not
    assert any(len({got.pushes[t, b]['count'] for b in schedule[t]}) == 2 for t in range(TICKS))


def test_reset_of_one_stream_discards_its_pending_frames(dev):
    lag = 2
    got = compare(stabilizer(dev), streams_of(dev, 'grey'), EVERYONE, lag, 'reset', resets={(4, 1)}, **SESSION)
    assert [len(got.frames[b]) for b in range(B)] == [10, 10 - lag, 10]                  # frames 2 and 3 of stream 1 never came out
    assert [got.pushes[4, b]['count'] for b in range(B)] == [1, 0, 1] and [got.pushes[4, b]['pending'] for b in range(B)] == [2, 1, 2]
    assert [got.pushes[9, b]['shots'] for b in range(B)] == [1, 2, 1] and [got.pushes[6, b]['first'] for b in range(B)] == [4, 0, 4]
    assert got.frames[1][2]['tick'] == 6 and got.frames[1][2]['d_unstab'].tobytes() == got.frames[1][0]['d_unstab'].tobytes()       # frame 0's vertices again


def test_the_limiter_keeps_every_stream_covered(dev):
    kw = dict(LIMIT_SESSION, on_uncovered='limit')
    got = compare(limit_stabilizer(dev), streams_of(dev, 'grey'), EVERYONE, 2, 'limit', **kw)
    k = np.array([[int(f['k']) for f in got.frames[b]] for b in range(B)])
    assert k.shape == (B, TICKS) and all(f['covered'] for b in range(B) for f in got.frames[b])
    assert k.min() < 32 and k.max() == 32, k.tolist()                                  # (not vacuous: a stream's step was cut back)


def test_a_cut_on_one_stream_hands_out_its_tail_in_front(dev):
    lag = 2
    kw = dict(SESSION, on_cut='reset')
    got = compare(stabilizer(dev), streams_of(dev, 'grey', middle=cuts_clip.one_cut()), EVERYONE, lag, 'cuts', **kw)
    assert [key for key in got.pushes if got.pushes[key]['cut']] == [(5, 1)]
    # the old shot's frames 3 and 4 come out of the cut's tick; the other streams hand out one frame as ever
    assert [got.pushes[5, b]['count'] for b in range(B)] == [1, lag, 1] and [got.pushes[5, b]['first'] for b in range(B)] == [3, 3, 3]
    assert [f['tick'] for f in got.frames[1]] == [2, 3, 4, 5, 5, 7, 8, 9, 'flush', 'flush']
    assert [got.pushes[5, b]['pending'] for b in range(B)] == [2, 1, 2] and [got.pushes[9, b]['shots'] for b in range(B)] == [1, 2, 1]
    assert got.frames[1][5]['d_unstab'].tobytes() == got.frames[1][0]['d_unstab'].tobytes()          # the new shot starts at frame 0's vertices
    assert all(got.pushes[0, b]['distance'] == 0 for b in range(B))
    assert got.pushes[5, 1]['distance'] > max(got.pushes[5, 0]['distance'], got.pushes[5, 2]['distance'])


def test_a_lost_pair_is_reported_at_the_tick_of_the_push(dev):
    lag = 2
    flat = grey_clip()
    flat[5] = 128                                                        # no corner in frame 5: the pair (5, 6) cannot be fitted
    got = compare(stabilizer(dev), streams_of(dev, 'grey', middle=flat), EVERYONE, lag, 'lost', **SESSION)
    assert got.pushes[6, 1]['lost'] == [6] and got.pushes[6, 1]['first'] == 4            # ... while frame 4 is what that tick hands out
    assert all(got.pushes[key]['lost'] == [] for key in got.pushes if key != (6, 1))
    assert got.frames[1][6]['d_unstab'].tobytes() == got.frames[1][5]['d_unstab'].tobytes()          # zero motion into frame 6
    assert got.frames[1][7]['d_unstab'].tobytes() != got.frames[1][6]['d_unstab'].tobytes()


def test_refusals_leave_the_group_as_it_was(dev):
    import torch
    s, clips = stabilizer(dev), streams_of(dev, 'grey')
    group = s.online_lag_group(B, 2, **SESSION)
    assert group.seen == group.pending == [0] * B and group.form is None
    with pytest.raises(ValueError, match='flush before the first push'):
        group.flush()
    with pytest.raises(ValueError, match='flush before the first push'):
        group.flush(1)
    group.reset()                                                        # before the first push: nothing to forget
    group.reset(1)
    frames = stacked([frame_of(c, 0) for c in clips])
    out, reports = group.push(frames)
    assert int(out.shape[0]) == 0 and out.dtype == torch.uint8 and tuple(out.shape[1:]) == (H, W) and group.last_counts == [0] * B
    for bad, ids, match in ((frames, [0, 1], 'one frame per pushed stream: 2 streams, 3 frames'), (frames[:2], None, 'one frame per pushed stream'),
                            (frames, [0, 1, 1], 'must be distinct'), (frames, [0, 1, B], r'lie in 0 \.\. 2'), (frames, [0, True, 2], 'sequence of ints'),
                            (frames[:, :64].contiguous(), None, 'this group takes'), (frames.cpu(), None, 'CUDA/HIP'),
                            (torch.zeros((B, 96, 128, 3), dtype=torch.uint8, device=dev), None, 'this group takes')):
        with pytest.raises(ValueError, match=match):
            group.push(bad, ids)
    for stream in (B, -1, True):
        with pytest.raises(ValueError, match='stream must'):
            group.flush(stream)
        with pytest.raises(ValueError, match='stream must'):
            group.reset(stream)
    assert group.seen == group.pending == [1] * B and group.shots == [1] * B
    group.push(stacked([frame_of(c, 1) for c in clips]))
    # a flush of one stream leaves the others pending; a stream with nothing pending gives a 0-row report
    out, reports = group.flush(1)
    assert int(out.shape[0]) == 2 and len(reports) == 1 and reports[0].first == 0 and int(reports[0].d_stab.shape[0]) == 2
    assert group.pending == [2, 0, 2] and group.seen == [2, 0, 2] and group.last_counts == [2]
    out, reports = group.flush(1)
    assert int(out.shape[0]) == 0 and int(reports[0].d_stab.shape[0]) == 0 and reports[0].first == 0 and group.last_counts == [0]
    out, reports = group.push(stacked([frame_of(c, 2) for c in clips]))
    assert [r.first for r in reports] == [0, 0, 0] and group.last_counts == [1, 0, 1] and int(out.shape[0]) == 2


def test_the_library_calls_of_a_steady_tick_do_not_grow_with_the_streams(dev, monkeypatch):
    from meshflow_amd import _lib
    calls = []

    def counted(name, entry):
        def call(*args):
            calls.append(name)
            return entry(*args)
        return call

    lag = 2
    s, clips = limit_stabilizer(dev), streams_of(dev, 'nv12')
    group = s.online_lag_group(B, lag, **dict(LIMIT_SESSION, on_uncovered='limit', on_cut='reset'))
    for t in range(lag):                                                 # every stream has `lag` frames: from here on every row hands one out
        group.push(stacked([frame_of(c, t) for c in clips]))
    assert group.pending == [lag] * B
    for name in _lib.SIGNATURES:
        if hasattr(_lib.lib, name):
            monkeypatch.setattr(_lib.lib, name, counted(name, getattr(_lib.lib, name)))
    per_push, at = {}, [lag] * B
    for ids in ([2], [0, 1], [1, 2, 0]):
        del calls[:]
        out, reports = group.push(stacked([frame_of(clips[b], at[b]) for b in ids]), ids)
        assert all(r.lost == [] and r.first == at[b] - lag for r, b in zip(reports, ids)) and group.last_counts == [1] * len(ids)
        assert group.last_cuts == [] and int(group.last_limit.shape[0]) == int(out[0].shape[0]) == len(ids)
        for b in ids:
            at[b] += 1
        per_push[len(ids)] = sorted(calls)
    assert per_push[1] == per_push[2] == per_push[3], per_push
    for name, times in (('mf_online_smooth_group_lag_f64', 1), ('mf_ring_exchange_u8', 2), ('mf_path_limit_group_f64', 1),
                        ('mf_cut_distance_pairs_i32', 1), ('mf_frame_signature_u8', 1)):
        assert per_push[3].count(name) == times, (name, per_push[3])
    assert not {'mf_online_smooth_lag_f64', 'mf_online_smooth_f64', 'mf_online_smooth_group_f64', 'mf_path_limit_f64', 'mf_cut_distance_i32'} & set(per_push[3])
