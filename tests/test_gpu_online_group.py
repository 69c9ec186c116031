"""`MeshFlowStabilizer.online_group` against one `online_session` per stream pushed the same frames one at a time, byte for byte in every
field of the contract -- frames, d_unstab, d_stab, covered, first, lost, the limiter's k, the cut decisions and distances, shots --: three
streams of 128 x 96 frames (tests/online_clips.py) in the grey, BGR and NV12 forms, every stream per tick and subsets in varying order, a
reset mid-stream, the path limiter, a cut and a lost pair on one stream alone; the refusals of `push`; and the number of library calls of a
push, which does not grow with the streams pushed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuts_clip  # noqa: E402
import tracker_clip  # noqa: E402
from online_clips import LIMIT_SESSION, SESSION, forms, grey_clip, limit_stabilizer, planes, shaky_clip, to_dev  # noqa: E402
from tracker_clip import stabilizer  # noqa: E402

pytestmark = pytest.mark.gpu

B, TICKS = 3, 10
EVERYONE = [[0, 1, 2]] * TICKS
FIELDS = ('frames', 'd_unstab', 'd_stab', 'covered', 'first', 'lost', 'rectangle', 'k', 'cut', 'distance', 'shots')


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def streams_of(dev, name, middle=None):
    """The three streams in form `name`: `grey_clip()`, the same frames reversed (or `middle`), `shaky_clip()[:10]`."""
    g = grey_clip()
    return [to_dev(forms(np.ascontiguousarray(clip))[name], dev) for clip in (g, g[::-1] if middle is None else middle, shaky_clip()[:TICKS])]


def frame_of(clip, t):
    return tuple(p[t:t + 1] for p in clip) if isinstance(clip, tuple) else clip[t:t + 1]


def stacked(frames):
    import torch
    return tuple(torch.cat(p) for p in zip(*frames)) if isinstance(frames[0], tuple) else torch.cat(frames)


def record(out, report, k, cut, distance, shots):
    host = lambda t: None if t is None else t.cpu().numpy()             # noqa: E731
    return dict(frames=planes(out), d_unstab=host(report.d_unstab), d_stab=host(report.d_stab), covered=host(report.covered), first=report.first,
                lost=list(report.lost), rectangle=report.rectangle, k=host(k), cut=cut, distance=distance, shots=shots)


def through_sessions(s, clips, schedule, resets=(), **kw):
    """{(tick, stream): record}: a session per stream, each pushed its own frames in order, one per tick it takes part in."""
    sessions, at, records = [s.online_session(**kw) for _ in clips], [0] * len(clips), {}
    for tick, ids in enumerate(schedule):
        for b in ids:
            if (tick, b) in resets:
                sessions[b].reset()
            out, report = sessions[b].push(frame_of(clips[b], at[b]))
            at[b] += 1
            d = sessions[b].last_cut_distances
            records[tick, b] = record(out, report, sessions[b].last_limit, sessions[b].last_cuts == [0], None if d is None else int(d[0]),
                                      sessions[b].shots)
            assert sessions[b].last_cuts in ([], [0])
    return records, [x.seen for x in sessions]


def through_a_group(s, clips, schedule, resets=(), **kw):
    """The same records from one group, a push per tick."""
    group, at, records = s.online_group(len(clips), **kw), [0] * len(clips), {}
    for tick, ids in enumerate(schedule):
        for b in ids:
            if (tick, b) in resets:
                group.reset(b)
        out, reports = group.push(stacked([frame_of(clips[b], at[b]) for b in ids]), None if ids == list(range(len(clips))) else ids)
        assert len(reports) == len(ids)
        for r, b in enumerate(ids):
            at[b] += 1
            k = None if group.last_limit is None else group.last_limit[r:r + 1]
            d = group.last_cut_distances
            records[tick, b] = record(frame_of(out, r), reports[r], k, r in group.last_cuts, None if d is None else int(d[r]), group.shots[b])
    return records, group.seen


def same_records(got, want, what):
    assert sorted(got) == sorted(want)
    for key in sorted(want):
        g, w = got[key], want[key]
        for field in FIELDS:
            if field == 'frames':
                assert len(g[field]) == len(w[field])
                for a, b in zip(g[field], w[field]):
                    tracker_clip.same_bits(a, b, (what, key, field))
            elif isinstance(w[field], np.ndarray):
                assert g[field] is not None and g[field].dtype == w[field].dtype, (what, key, field)
                tracker_clip.same_bits(g[field], w[field], (what, key, field))
            else:
                assert g[field] == w[field] and type(g[field]) is type(w[field]), (what, key, field, g[field], w[field])


def compare(s, clips, schedule, what, resets=(), **kw):
    want, want_seen = through_sessions(s, clips, schedule, resets, **kw)
    got, got_seen = through_a_group(s, clips, schedule, resets, **kw)
    same_records(got, want, what)
    assert got_seen == want_seen, what
    return got


@pytest.mark.parametrize('name', ['grey', 'bgr', 'nv12'])
def test_every_stream_per_tick_equals_three_sessions(dev, name):
    got = compare(stabilizer(dev), streams_of(dev, name), EVERYONE, name, **SESSION)
    last = [got[TICKS - 1, b] for b in range(B)]
    assert all(r['first'] == TICKS - 1 and r['shots'] == 1 and r['k'] is None and r['distance'] is None for r in last)
    # three different streams came out: different paths, and something was smoothed
    assert len({r['d_unstab'].tobytes() for r in last}) == B and all(r['d_stab'].tobytes() != r['d_unstab'].tobytes() for r in last)


def test_subsets_in_any_order_equal_the_sessions(dev):
    # stream 2 joins at tick 3, stream 1 skips ticks 5 and 6, and the order of the ids turns with the tick
    schedule = []
    for tick in range(TICKS):
        ids = [b for b in range(B) if not (b == 2 and tick < 3) and not (b == 1 and tick in (5, 6))]
        schedule.append(ids[tick % len(ids):] + ids[:tick % len(ids)])
    assert [len(ids) for ids in schedule] == [2, 2, 2, 3, 3, 2, 2, 3, 3, 3] and schedule[4] == [1, 2, 0] and schedule[5] == [2, 0]
    got = compare(stabilizer(dev), streams_of(dev, 'grey'), schedule, 'subsets', **SESSION)
    assert got[3, 2]['first'] == 0 and got[7, 1]['first'] == 5 and got[9, 0]['first'] == 9


def test_reset_of_one_stream_equals_the_sessions_reset(dev):
    got = compare(stabilizer(dev), streams_of(dev, 'grey'), EVERYONE, 'reset', resets={(4, 1)}, **SESSION)
    assert [got[4, b]['first'] for b in range(B)] == [4, 0, 4] and [got[9, b]['shots'] for b in range(B)] == [1, 2, 1]
    assert got[4, 1]['d_unstab'].tobytes() == got[0, 1]['d_unstab'].tobytes()          # the path starts again: frame 0's vertices


def test_the_limiter_keeps_every_stream_covered(dev):
    kw = dict(LIMIT_SESSION, on_uncovered='limit')
    got = compare(limit_stabilizer(dev), streams_of(dev, 'grey'), EVERYONE, 'limit', **kw)
    k = np.array([[int(got[t, b]['k'][0]) for b in range(B)] for t in range(TICKS)])
    assert all(got[key]['covered'].all() for key in got)
    assert k.min() < 32 and k.max() == 32 and (k[0] == 32).all(), k.tolist()           # (not vacuous: a stream's step was cut back)


def test_a_cut_on_one_stream_restarts_that_stream_alone(dev):
    kw = dict(SESSION, on_cut='reset')
    got = compare(stabilizer(dev), streams_of(dev, 'grey', middle=cuts_clip.one_cut()), EVERYONE, 'cuts', **kw)
    assert [key for key in sorted(got) if got[key]['cut']] == [(5, 1)]
    assert [got[5, b]['first'] for b in range(B)] == [5, 0, 5] and [got[9, b]['shots'] for b in range(B)] == [1, 2, 1]
    assert got[5, 1]['d_unstab'].tobytes() == got[0, 1]['d_unstab'].tobytes() and got[4, 1]['d_unstab'].tobytes() != got[0, 1]['d_unstab'].tobytes()
    assert all(got[0, b]['distance'] == 0 for b in range(B)) and got[5, 1]['distance'] > max(got[5, 0]['distance'], got[5, 2]['distance'])


def test_a_lost_pair_stays_in_its_stream(dev):
    flat = grey_clip()
    flat[5] = 128                                                        # no corner in frame 5: the pair (5, 6) cannot be fitted
    got = compare(stabilizer(dev), streams_of(dev, 'grey', middle=flat), EVERYONE, 'lost', **SESSION)
    assert got[6, 1]['lost'] == [6] and all(got[t, b]['lost'] == [] for t in range(TICKS) for b in (0, 2))
    assert got[6, 1]['d_unstab'].tobytes() == got[5, 1]['d_unstab'].tobytes() and got[7, 1]['d_unstab'].tobytes() != got[6, 1]['d_unstab'].tobytes()


def test_refusals_leave_the_group_as_it_was(dev):
    import torch
    s, clips = stabilizer(dev), streams_of(dev, 'grey')
    group = s.online_group(B, **SESSION)
    assert group.seen == [0] * B and group.form is None
    group.reset()                                                        # before the first push: nothing to forget
    group.reset(1)
    frames = stacked([frame_of(c, 0) for c in clips])
    group.push(frames)
    for bad, ids, match in ((frames, [0, 1], 'one frame per pushed stream: 2 streams, 3 frames'), (frames[:2], None, 'one frame per pushed stream'),
                            (frames, [0, 1, 1], 'must be distinct'), (frames, [0, 1, B], r'lie in 0 \.\. 2'), (frames, [0, True, 2], 'sequence of ints'),
                            (frames[:, :64].contiguous(), None, 'this group takes'), (frames.cpu(), None, 'CUDA/HIP'),
                            (torch.zeros((B, 96, 128, 3), dtype=torch.uint8, device=dev), None, 'this group takes')):
        with pytest.raises(ValueError, match=match):
            group.push(bad, ids)
    with pytest.raises(ValueError, match=r'stream must lie in 0 \.\. 2'):
        group.reset(B)
    assert group.seen == [1] * B and group.shots == [1] * B
    _, reports = group.push(stacked([frame_of(c, 1) for c in clips]))
    assert [r.first for r in reports] == [1] * B


def test_the_library_calls_of_a_push_do_not_grow_with_the_streams(dev, monkeypatch):
    from meshflow_amd import _lib
    calls = []

    def counted(name, entry):
        def call(*args):
            calls.append(name)
            return entry(*args)
        return call

    s, clips = limit_stabilizer(dev), streams_of(dev, 'grey')
    group = s.online_group(B, **dict(LIMIT_SESSION, on_uncovered='limit', on_cut='reset'))
    group.push(stacked([frame_of(c, 0) for c in clips]))                 # every stream has a frame before: from here on every row is tracked
    for name in _lib.SIGNATURES:
        if hasattr(_lib.lib, name):
            monkeypatch.setattr(_lib.lib, name, counted(name, getattr(_lib.lib, name)))
    per_push, at = {}, [1] * B
    for ids in ([2], [0, 1], [1, 2, 0]):
        del calls[:]
        _, reports = group.push(stacked([frame_of(clips[b], at[b]) for b in ids]), ids)
        assert all(r.lost == [] and r.first == at[b] for r, b in zip(reports, ids))
        for b in ids:
            at[b] += 1
        per_push[len(ids)] = sorted(calls)
    assert per_push[1] == per_push[2] == per_push[3], per_push
    for name in ('mf_online_smooth_group_f64', 'mf_path_limit_group_f64', 'mf_cut_distance_pairs_i32', 'mf_frame_signature_u8'):
        assert per_push[3].count(name) == 1, (name, per_push[3])
    assert not {'mf_online_smooth_f64', 'mf_path_limit_f64', 'mf_cut_distance_i32'} & set(per_push[3])
