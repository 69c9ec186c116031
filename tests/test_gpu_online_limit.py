"""Online sessions that limit the path (`online_session(on_uncovered='limit')`): on a clip whose offsets in tests/tracker_clip.py's canvas take
a 12-pixel step -- more than the 7 rows an 8 % margin leaves -- the default session reports uncovered frames and shows border colour, the
limiting one covers every frame; what it warped is `ops.path_limit` of the default session's paths; blocks equal one push; `reset()`, a cut
and a refused push treat the carried step as they treat the rest of the session.  And the promise that 'report' is today's session."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuts_clip  # noqa: E402
import cuts_model as cm  # noqa: E402
import online_clips  # noqa: E402
from online_clips import FLOOR, GUARD, LIMIT_SESSION, RISE, C, H, K, R, W, part, planes, shaky_clip, to_dev  # noqa: E402
from online_clips import limit_stabilizer as stabilizer  # noqa: E402
from tracker_clip import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

SESSION = LIMIT_SESSION
FORMS = ['grey', 'bgr', 'nv12']


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def forms(g):
    """grey and NV12 as every session suite has them; BGR with three equal channels, whose red border has B = G = 0, below FLOOR."""
    made = online_clips.forms(g)
    return {'grey': g, 'bgr': np.ascontiguousarray(np.stack([g, g, g], axis=-1)), 'nv12': made['nv12']}


def same_push(got, want, what):
    """(frames, report, last_limit) of either side, lists of them joined: frames byte for byte, paths bit for bit, covered, k."""
    g_out, g_rep, g_k = got
    w_out, w_rep, w_k = want
    for g, w in zip([np.concatenate(p) for p in zip(*(planes(o) for o in g_out))], [np.concatenate(p) for p in zip(*(planes(o) for o in w_out))]):
        same_bits(g, w, (what, 'frames'))
    for field in ('d_unstab', 'd_stab', 'covered'):
        same_bits(np.concatenate([getattr(r, field).cpu().numpy() for r in g_rep]), np.concatenate([getattr(r, field).cpu().numpy() for r in w_rep]),
                  (what, field))
    same_bits(np.concatenate([k.cpu().numpy() for k in g_k]), np.concatenate([k.cpu().numpy() for k in w_k]), (what, 'k'))


@pytest.fixture(scope='module')
def clips(dev):
    return {name: to_dev(clip, dev) for name, clip in forms(shaky_clip()).items()}


@pytest.fixture(scope='module')
def pushed(dev, clips):
    """Every form through a default session and through a limiting one, once: name -> ((out, report), (out, report, last_limit))."""
    s, made = stabilizer(dev), {}
    for name, clip in clips.items():
        plain = s.online_session(**SESSION).push(clip)
        session = s.online_session(on_uncovered='limit', **SESSION)
        out, report = session.push(clip)
        made[name] = plain, (out, report, session.last_limit)
    return made


def test_report_is_the_default_session(dev, clips):
    s, clip = stabilizer(dev), clips['grey']
    default, explicit = s.online_session(**SESSION), s.online_session(on_uncovered='report', **SESSION)
    out, report = default.push(clip)
    out2, report2 = explicit.push(clip)
    same_bits(out2.cpu().numpy(), out.cpu().numpy(), 'frames')
    for field in ('d_unstab', 'd_stab', 'covered'):
        same_bits(getattr(report2, field).cpu().numpy(), getattr(report, field).cpu().numpy(), field)
    for session in (default, explicit):
        assert session.on_uncovered == 'report' and session.last_limit is None and session._k_prev is None and session.limit_steps == K
    assert tuple(report._fields) == ('first', 'd_unstab', 'd_stab', 'rectangle', 'covered', 'lost')


@pytest.mark.parametrize('name', FORMS)
def test_the_limiter_keeps_the_crop_covered(dev, clips, pushed, name):
    import torch
    from meshflow_amd import ops
    (plain_out, plain), (out, report, k) = pushed[name]
    n = 14
    # the parent's behaviour first: without it the rest shows nothing
    uncovered = (~plain.covered).sum().item()
    print(name, 'default session: covered', plain.covered.cpu().numpy().astype(int).tolist())
    assert uncovered >= 3, plain.covered.cpu().numpy().tolist()
    print(name, "'limit' session: covered", report.covered.cpu().numpy().astype(int).tolist(), 'k', k.cpu().numpy().tolist())
    assert report.covered.all().item() and report.lost == plain.lost == [] and report.rectangle == plain.rectangle == (10, 7, 117, 88)
    assert k.is_cuda and k.dtype == torch.int32 and tuple(k.shape) == (n,)
    steps = k.cpu().numpy()
    assert steps.min() < K and steps.max() <= K and steps.min() >= 0 and (np.diff(steps) <= RISE).all() and steps[0] == K
    # what was warped, and reported, is the limiter's answer to the default session's paths; the unstabilized path is untouched
    same_bits(report.d_unstab.cpu().numpy(), plain.d_unstab.cpu().numpy(), 'd_unstab')
    want, want_k = ops.path_limit(plain.d_unstab, plain.d_stab, W, H, R, C, plain.rectangle, K, GUARD, RISE)
    same_bits(report.d_stab.cpu().numpy().reshape(n, -1), want.cpu().numpy(), 'd_stab')
    same_bits(steps, want_k.cpu().numpy(), 'k')
    assert report.d_stab.cpu().numpy().tobytes() != plain.d_stab.cpu().numpy().tobytes()
    if name != 'nv12':                                                   # (NV12's border luma, 81, is a level the canvas has)
        # bilinear taps of values >= FLOOR cannot make a value below it; the border's bytes are 0 (grey; B and G of the red border)
        got, shown = out.cpu().numpy(), plain_out.cpu().numpy()
        if name == 'bgr':
            got, shown = got[..., :2], shown[..., :2]
        assert got.min() >= FLOOR, int(got.min())
        assert shown.min() < FLOOR                                       # (and the default session does show border colour on this clip)


@pytest.mark.parametrize('name', FORMS)
def test_blocks_equal_one_push(dev, clips, pushed, name):
    s, clip = stabilizer(dev), clips[name]
    out, report, k = pushed[name][1]
    session, at, outs, reports, ks = s.online_session(on_uncovered='limit', **SESSION), 0, [], [], []
    for b in (1, 3, 10):
        o, r = session.push(part(clip, at, at + b))
        assert r.first == at and tuple(session.last_limit.shape) == (b,)
        outs.append(o), reports.append(r), ks.append(session.last_limit)
        at += b
    same_push((outs, reports, ks), ([out], [report], [k]), name)


def test_reset_and_a_cut_start_the_step_at_K_again(dev, clips, pushed):
    import torch
    s, clip = stabilizer(dev), clips['grey']
    k = pushed['grey'][1][2].cpu().numpy()
    assert k[6] + RISE < K                                               # frame 7 of a continuing session cannot be back at K
    # reset(): the next push is a fresh session's
    session = s.online_session(on_uncovered='limit', **SESSION)
    session.push(clip[:7])
    assert session._k_prev is not None and int(session._k_prev.item()) == k[6]
    session.reset()
    assert session._k_prev is None
    got = session.push(clip[7:11])
    fresh = s.online_session(on_uncovered='limit', **SESSION)
    want = fresh.push(clip[7:11])
    same_push(([got[0]], [got[1]], [session.last_limit]), ([want[0]], [want[1]], [fresh.last_limit]), 'reset')
    assert session.last_limit[0].item() == K
    # a cut found by on_cut='reset': scene B behind the first seven frames
    scene_b = torch.from_numpy(np.maximum(cuts_clip.scene_b()[:4], FLOOR)).to(dev)
    joined = torch.cat([clip[:7], scene_b])
    cutting = s.online_session(on_uncovered='limit', on_cut='reset', **SESSION)
    out, report = cutting.push(joined)
    assert cutting.last_cuts == [7] and tuple(cutting.last_limit.shape) == (11,)
    hand = s.online_session(on_uncovered='limit', **SESSION)
    first = hand.push(clip[:7])
    first_k = hand.last_limit
    hand.reset()
    second = hand.push(scene_b)
    same_push(([out], [report], [cutting.last_limit]), ([first[0], second[0]], [first[1], second[1]], [first_k, hand.last_limit]), 'cut')
    assert cutting.last_limit[6].item() == k[6] and cutting.last_limit[7].item() == K


def test_raise_restores_the_carried_step(dev, clips):
    """on_lost='raise' under on_cut='reset': a push whose first part went through, and moved the carried step, before a later part met a pair
    that cannot be fitted leaves the session, the step included, where it was."""
    import torch
    s, clip = stabilizer(dev), clips['grey']
    scene_b = np.maximum(cuts_clip.scene_b()[:4], FLOOR)
    # frame 2 with the pixels of every tile sorted (tests/test_gpu_online_cuts.py's device): its signature is frame 2's, so no cut is seen
    # there, and too few features lead out of it
    rows, cols = cm.tile_edges(H), cm.tile_edges(W)
    for i in range(4):
        for j in range(4):
            tile = scene_b[2, rows[i]:rows[i + 1], cols[j]:cols[j + 1]]
            tile[...] = np.sort(tile.reshape(-1)).reshape(tile.shape)
    block = torch.cat([clip[7:9], torch.from_numpy(scene_b).to(dev)])
    session = s.online_session(on_uncovered='limit', on_cut='reset', on_lost='raise', **SESSION)
    session.push(clip[:7])
    before = (session.seen, session.shots, int(session._k_prev.item()), session._last_luma.cpu().numpy().tobytes())
    with pytest.raises(ValueError, match='fewer than 4 features could be tracked'):
        session.push(block)
    assert (session.seen, session.shots, int(session._k_prev.item()), session._last_luma.cpu().numpy().tobytes()) == before
    got = session.push(clip[7:9])
    other = s.online_session(on_uncovered='limit', on_cut='reset', on_lost='raise', **SESSION)
    other.push(clip[:7])
    want = other.push(clip[7:9])
    same_push(([got[0]], [got[1]], [session.last_limit]), ([want[0]], [want[1]], [other.last_limit]), 'after the refused push')
    assert session.last_limit[0].item() <= before[2] + RISE


def test_refusals(dev, clips):
    import torch
    s = stabilizer(dev)
    for kw, match in ((dict(on_uncovered='crop'), "on_uncovered must be 'report' or 'limit'"), (dict(limit_steps=0), 'limit_steps must be an integer in 1 .. 64'),
                      (dict(limit_steps=65), 'limit_steps must be'), (dict(limit_rise=0), 'limit_rise must be an integer in 1 .. limit_steps = 32'),
                      (dict(limit_rise=33), 'limit_rise must be'), (dict(limit_guard=-1.0), 'limit_guard must be a finite number >= 0'),
                      (dict(limit_guard=float('nan')), 'limit_guard must be')):
        with pytest.raises(ValueError, match=match):
            s.online_session(**dict(SESSION, **kw))
    # a rectangle the guard does not fit into the untouched frame: floor(0.02 * 95) = 1 row above it, the guard needs 3
    session = s.online_session(on_uncovered='limit', **dict(SESSION, crop_margin=0.02))
    with pytest.raises(ValueError, match='widen crop_margin'):
        session.push(clips['grey'][:2])
    assert session.form is None and session.seen == 0
    s.online_session(**dict(SESSION, crop_margin=0.02)).push(clips['grey'][:2])             # ('report' takes that margin as before)
    out, report = s.stabilize_online(clips['grey'], on_uncovered='limit', **SESSION)
    assert report.covered.all().item() and out.shape == clips['grey'].shape
