"""Online sessions that find the cuts themselves (`online_session(on_cut='reset')`) against plain sessions reset by hand at the same frames,
byte for byte, on clips made of two scenes (tests/cuts_clip.py); `MeshFlowStabilizer.find_cuts` on every form a clip takes; and the promise
that a session which ignores cuts is today's session."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuts_clip  # noqa: E402
import cuts_model as cm  # noqa: E402
import luma_clip  # noqa: E402
import luma_model  # noqa: E402
import tracker_clip  # noqa: E402
from online_clips import SESSION, forms, part, planes, to_dev  # noqa: E402
from tracker_clip import stabilizer  # noqa: E402

pytestmark = pytest.mark.gpu

W, H = cuts_clip.W, cuts_clip.H
FORMS = ['grey', 'bgr', 'nv12']


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def clips(dev):
    made = {}
    for clip, grey in (('A', cuts_clip.scene_a()), ('M', cuts_clip.one_cut()), ('M2', cuts_clip.two_cuts())):
        for name, frames in forms(grey).items():
            made[clip, name] = to_dev(frames, dev)
    return made


def pushed(session, clip, blocks):
    """The clip pushed in blocks of these sizes: (frames, reports, (last_cuts, shots) after each push)."""
    at, outs, reports, seen = 0, [], [], []
    for b in blocks:
        out, report = session.push(part(clip, at, at + b))
        outs.append(out)
        reports.append(report)
        seen.append((list(session.last_cuts), session.shots))
        at += b
    return outs, reports, seen


def by_hand(s, clip, shots, **kw):
    """A plain session, one push per shot [lo, hi), `reset()` between them."""
    session = s.online_session(**dict(SESSION, **kw))
    outs, reports = [], []
    for k, (lo, hi) in enumerate(shots):
        if k:
            session.reset()
        out, report = session.push(part(clip, lo, hi))
        outs.append(out)
        reports.append(report)
    return outs, reports


def same(got_outs, got_reports, want_outs, want_reports, what):
    """Frames byte for byte, paths bit for bit, equal covered and lost -- the joined results of either side."""
    got = [np.concatenate(p) for p in zip(*(planes(o) for o in got_outs))]
    want = [np.concatenate(p) for p in zip(*(planes(o) for o in want_outs))]
    assert len(got) == len(want)
    for g, w in zip(got, want):
        tracker_clip.same_bits(g, w, (what, 'frames'))
    for field in ('d_unstab', 'd_stab', 'covered'):
        tracker_clip.same_bits(np.concatenate([getattr(r, field).cpu().numpy() for r in got_reports]),
                               np.concatenate([getattr(r, field).cpu().numpy() for r in want_reports]), (what, field))
    assert [t for r in got_reports for t in r.lost] == [t for r in want_reports for t in r.lost], what
    assert got_reports[0].first == want_reports[0].first and got_reports[0].rectangle == want_reports[0].rectangle, what


@pytest.fixture(scope='module')
def hand(dev, clips):
    """The hand-reset plain sessions, once per form."""
    s = stabilizer(dev)
    return {name: by_hand(s, clips['M', name], ((0, 5), (5, 10))) for name in FORMS}


@pytest.mark.parametrize('name', FORMS)
def test_one_push_equals_two_pushes_and_a_reset(dev, clips, hand, name):
    import torch
    s, clip = stabilizer(dev), clips['M', name]
    session = s.online_session(on_cut='reset', **SESSION)
    out, report = session.push(clip)
    same([out], [report], *hand[name], name)
    assert session.last_cuts == [5] and session.shots == 2 and session.seen == 5
    assert tuple(report.d_stab.shape) == (10, 5, 5, 2) and tuple(report.covered.shape) == (10,) and report.covered.dtype == torch.bool
    luma = luma_model.luma(luma_clip.bgr(cuts_clip.one_cut())) if name == 'bgr' else cuts_clip.one_cut()
    tracker_clip.same_bits(session.last_cut_distances, cm.distances(cm.signatures(luma)), 'distances')
    # the path starts again at the cut: frame 5's vertices are where frame 0's are
    c = report.d_unstab.cpu().numpy()
    assert c[5].tobytes() == c[0].tobytes() and c[4].tobytes() != c[0].tobytes()


@pytest.mark.parametrize('name', FORMS)
@pytest.mark.parametrize('blocks', [(3, 4, 3), (5, 5)])
def test_blocks_equal_the_one_push(dev, clips, hand, name, blocks):
    s = stabilizer(dev)
    session = s.online_session(on_cut='reset', **SESSION)
    outs, reports, seen = pushed(session, clips['M', name], blocks)
    same(outs, reports, *hand[name], (name, blocks))
    if blocks == (3, 4, 3):                                             # the cut inside the second block
        assert seen == [([], 1), ([2], 2), ([], 2)] and [r.first for r in reports] == [0, 3, 2]
    else:                                                               # the cut between the pushes: the session is reset before the block
        assert seen == [([], 1), ([0], 2)] and [r.first for r in reports] == [0, 0]
    assert session.seen == 5


def test_two_cuts_equal_three_pushes_and_two_resets(dev, clips):
    s, clip = stabilizer(dev), clips['M2', 'grey']
    session = s.online_session(on_cut='reset', **SESSION)
    out, report = session.push(clip)
    assert session.last_cuts == [3, 7] and session.shots == 3 and session.seen == 3
    same([out], [report], *by_hand(s, clip, ((0, 3), (3, 7), (7, 10))), 'M2')


@pytest.mark.parametrize('name', FORMS)
def test_a_clip_without_cuts_is_the_plain_session_s(dev, clips, name):
    s, clip = stabilizer(dev), clips['A', name]
    session = s.online_session(on_cut='reset', **SESSION)
    out, report = session.push(clip)
    assert session.last_cuts == [] and session.shots == 1 and session.last_cut_distances.shape == (10,) and session.last_cut_distances[0] == 0
    same([out], [report], *by_hand(s, clip, ((0, 10),)), name)
    # and in blocks, the signature carried from push to push
    session = s.online_session(on_cut='reset', **SESSION)
    outs, reports, seen = pushed(session, clip, (1, 3, 6))
    assert seen == [([], 1)] * 3 and session.last_cut_distances[0] > 0
    plain = pushed(s.online_session(**SESSION), clip, (1, 3, 6))
    same(outs, reports, plain[0], plain[1], (name, 'blocks'))


def test_ignore_is_the_default_and_tracks_across_the_cut(dev, clips):
    s, clip = stabilizer(dev), clips['M', 'grey']
    default = s.online_session(**SESSION)
    out, report = default.push(clip)
    explicit = s.online_session(on_cut='ignore', **SESSION)
    out2, report2 = explicit.push(clip)
    same([out], [report], [out2], [report2], 'ignore')
    for session in (default, explicit):
        assert session.last_cuts == [] and session.last_cut_distances is None and session.shots == 1 and session.seen == 10
    reset = s.online_session(on_cut='reset', **SESSION)
    _, report3 = reset.push(clip)
    assert report3.d_unstab.cpu().numpy().tobytes() != report.d_unstab.cpu().numpy().tobytes()
    # a manual reset forgets the signature: the first frame after it is no cut, whatever came before
    reset.reset()
    reset.push(clips['A', 'grey'][:2])
    assert reset.last_cuts == [] and reset.shots == 3 and reset.last_cut_distances[0] == 0
    # a threshold of 1.0 finds nothing
    never = s.online_session(on_cut='reset', cut_threshold=1.0, **SESSION)
    _, report4 = never.push(clip)
    assert never.last_cuts == [] and report4.d_unstab.cpu().numpy().tobytes() == report.d_unstab.cpu().numpy().tobytes()


def test_raise_leaves_the_session_as_it_was(dev, clips):
    """on_lost='raise' under on_cut='reset': a push whose SECOND shot holds a pair that cannot be fitted raises after the first shot went
    through and the cut reset the session -- and the session, signature included, is where it was."""
    import torch
    s = stabilizer(dev)
    g = cuts_clip.one_cut()
    # frame 8 with the pixels of every tile sorted: its signature is frame 8's, so no cut is seen there, and the model pipeline
    # (tests/luma_clip.py, model_fit_records) finds too few features from it to frame 9
    rows, cols = cm.tile_edges(H), cm.tile_edges(W)
    for i in range(4):
        for j in range(4):
            tile = g[8, rows[i]:rows[i + 1], cols[j]:cols[j + 1]]
            tile[...] = np.sort(tile.reshape(-1)).reshape(tile.shape)
    assert cm.find_cuts(g)[0] == [5]
    clip = torch.from_numpy(g).to(dev)
    hold = s.online_session(on_cut='reset', **SESSION)
    _, report = hold.push(clip)
    assert hold.last_cuts == [5] and report.lost and set(report.lost) <= {3, 4}          # (in the second shot's own numbering)
    session = s.online_session(on_cut='reset', on_lost='raise', **SESSION)
    session.push(clip[:3])
    before = (session.seen, session.shots, list(session.last_cuts), session._last_sig.cpu().numpy().tobytes(), session._last_luma.cpu().numpy().tobytes(),
              [t.cpu().numpy().tobytes() for t in (session.state.c, session.state.q, session.state.lam)])
    with pytest.raises(ValueError, match='fewer than 4 features could be tracked'):
        session.push(clip[3:])
    after = (session.seen, session.shots, list(session.last_cuts), session._last_sig.cpu().numpy().tobytes(), session._last_luma.cpu().numpy().tobytes(),
             [t.cpu().numpy().tobytes() for t in (session.state.c, session.state.q, session.state.lam)])
    assert after == before
    _, r = session.push(clip[3:5])
    assert r.first == 3 and r.lost == [] and session.last_cuts == []


@pytest.mark.parametrize('name', ['grey', 'bgr', 'nv12', 'bgr16', 'bgra', 'p010'])
def test_find_cuts_on_every_form(dev, clips, name):
    s = stabilizer(dev)
    assert s.find_cuts(clips['M', name]) == [5]
    assert s.find_cuts(clips['A', name]) == []
    assert s.find_cuts(clips['M2', name]) == [3, 7]
    assert s.find_cuts(clips['M', name], threshold=1.0) == []


def test_find_cuts_at_a_low_threshold_and_red_first(dev, clips):
    s = stabilizer(dev)
    a = cuts_clip.scene_a()
    for threshold, count in ((0.05, 9), (0.07, 3)):                     # every pair of scene A is above 5 %, three of them above 7 %
        want = cm.find_cuts(a, threshold)[0]
        assert len(want) == count
        assert s.find_cuts(clips['A', 'grey'], threshold=threshold) == want
    # red_first reaches the luma: B = 255 - g read as red gives another luma, and the model's list for it
    colour = luma_clip.bgr(a)
    plain, swapped = (cm.find_cuts(luma_model.luma(colour, red_first=r), 0.05)[0] for r in (False, True))
    assert plain != swapped
    assert s.find_cuts(clips['A', 'bgr'], threshold=0.05) == plain
    assert s.find_cuts(clips['A', 'bgr'], threshold=0.05, red_first=True) == swapped
