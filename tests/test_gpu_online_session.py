"""`MeshFlowStabilizer.online_session` against the composition of the ops written out by hand, on tests/tracker_clip.py's canvas cut into ten
128 x 96 frames: every form a push takes, blocks against one push, the fixed rectangle and its `covered` flags, a lost pair, reset, and the
refusals."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracker_clip  # noqa: E402
from online_clips import (BETA, C, H, ITERS, MARGIN, R, S, SESSION, W, WINDOW, forms, grey_clip, host_of, part, rectangle,  # noqa: E402
                          same_frames, to_dev)
from tracker_clip import MAX_PER, SHIFTS, stabilizer  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def by_hand(s, clip, margin=MARGIN, output_size=None):
    """One push of a whole clip from frame 0, written out from the ops: (frames, c, p, table.crop)."""
    import torch
    from meshflow_amd import host, ops
    pair = isinstance(clip, tuple)
    if pair:
        fmt = ops._P010 if clip[0].dtype == torch.uint16 else ops._NV12
        luma = ops.luma(clip[0]) if fmt is ops._P010 else clip[0]
    else:
        luma = ops.luma(clip) if ops.luma_source(clip) is not None else clip
    dev, n = luma.device, luma.shape[0]
    early, late, offsets, kmax, hom, info = s.device_tracker(MAX_PER, 'device', 'device').track_stacks_resident(luma[:-1], luma[1:], 32)
    assert ops.fit_check(info) is None
    _, vel, status = ops.vertex_motion(early, late, offsets, hom, kmax, W, H, R, C, s.feature_ellipse_row_count, s.feature_ellipse_col_count)
    assert int(status.item()) == 0
    lam_newest = float(host.adaptive_weights(1, W, H, 0, np.identity(3)[None])[0])
    assert lam_newest == 0.95
    lam = np.concatenate([[lam_newest], host.adaptive_weights(n - 1, W, H, 0, hom.cpu().numpy())])
    state = ops.OnlineState(S, WINDOW, dev)
    block = torch.cat([torch.zeros((1, S), dtype=torch.float32, device=dev), vel.reshape(n - 1, S)])
    taps = torch.from_numpy(host.online_taps(s.temporal_smoothing_radius)).to(dev)
    c, p = ops.online_smooth(block, torch.from_numpy(lam).to(dev), state, taps, s.temporal_smoothing_radius, ITERS, BETA, lam_newest)
    table = ops.cell_table(c, p, W, H, R, C)
    rect = rectangle(margin)
    if pair:
        warped = (ops.warp_p010 if fmt is ops._P010 else ops.warp_nv12)(clip[0], clip[1], table)
        out = warped if margin == 0 else (ops.crop_resize_p010 if fmt is ops._P010 else ops.crop_resize_nv12)(*warped, rect, size=output_size)
    else:
        warped = ops.warp(clip, table, s.color_outside_image_area_bgr)
        out = warped if margin == 0 else ops.crop_resize(warped, rect, size=output_size)
    table.check()
    return out, c, p, table.crop.clone()


@pytest.fixture(scope='module')
def clips(dev):
    return {name: to_dev(clip, dev) for name, clip in forms(grey_clip()).items()}


@pytest.fixture(scope='module')
def hand(dev, clips):
    """The hand composition of every form, once."""
    s = stabilizer(dev)
    return {name: by_hand(s, clip) for name, clip in clips.items()}


def check_push(out, report, want, n, first=0):
    import torch
    frames, c, p, crop = want
    same_frames(out, frames, 'frames')
    assert report.first == first and report.lost == [] and report.rectangle == rectangle(MARGIN)
    for got, path, what in ((report.d_unstab, c, 'd_unstab'), (report.d_stab, p, 'd_stab')):
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (n, R + 1, C + 1, 2), what
        tracker_clip.same_bits(got.cpu().numpy().reshape(n, S), path.cpu().numpy(), what)
    left, top, right, bottom = rectangle(MARGIN)
    crop = crop.cpu().numpy()
    covered = (crop[:, 0] <= left) & (crop[:, 1] <= top) & (crop[:, 2] >= right) & (crop[:, 3] >= bottom)
    assert report.covered.is_cuda and report.covered.dtype == torch.bool
    assert report.covered.cpu().numpy().tolist() == covered.tolist()
    return covered


@pytest.mark.parametrize('name', ['grey', 'bgr', 'nv12'])
def test_push_equals_the_hand_composition_and_blocks_equal_one_push(dev, clips, hand, name):
    import torch
    s, clip = stabilizer(dev), clips[name]
    n = 10
    out, report = s.online_session(**SESSION).push(clip)
    covered = check_push(out, report, hand[name], n)
    assert report.d_stab.cpu().numpy().tobytes() != report.d_unstab.cpu().numpy().tobytes()       # (something was smoothed)
    assert covered.any()                                                 # (an 8 % margin holds this clip's few pixels of correction somewhere)
    # the path is the clip's: content moves by SHIFTS, so frame 1's vertices sit about (3, -2) from frame 0's
    first = report.d_unstab[1].cpu().numpy().reshape(-1, 2).mean(axis=0)
    assert abs(first[0] - SHIFTS[0][0]) < 0.5 and abs(first[1] - SHIFTS[0][1]) < 0.5
    # the whole clip through `stabilize_online`, and as blocks (1, 3, rest): byte for byte
    again, report2 = s.stabilize_online(clip, **SESSION)
    same_frames(again, out, 'stabilize_online')
    session, at, outs, reports = s.online_session(**SESSION), 0, [], []
    for b in (1, 3, n - 4):
        o, r = session.push(part(clip, at, at + b))
        assert r.first == at and session.seen == at + b
        outs.append(o)
        reports.append(r)
        at += b
    joined = tuple(torch.cat([o[i] for o in outs]) for i in range(2)) if isinstance(out, tuple) else torch.cat(outs)
    same_frames(joined, out, 'blocks')
    for field in ('d_unstab', 'd_stab', 'covered'):
        tracker_clip.same_bits(torch.cat([getattr(r, field) for r in reports]).cpu().numpy(), getattr(report, field).cpu().numpy(), field)


@pytest.mark.parametrize('name', ['bgr16', 'bgra', 'p010'])
def test_the_other_forms(dev, clips, hand, name):
    s, clip = stabilizer(dev), clips[name]
    out, report = s.online_session(**SESSION).push(clip)
    if isinstance(clip, tuple):
        assert isinstance(out, tuple) and [o.dtype for o in out] == [p.dtype for p in clip] and [o.shape for o in out] == [p.shape for p in clip]
    else:
        assert out.dtype == clip.dtype and out.shape == clip.shape
    check_push(out, report, hand[name], 10)


def test_red_first_reaches_the_luma(dev, clips):
    s = stabilizer(dev)
    _, plain = s.online_session(**SESSION).push(clips['bgr'])
    _, swapped = s.online_session(red_first=True, **SESSION).push(clips['bgr'])
    assert plain.d_unstab.cpu().numpy().tobytes() != swapped.d_unstab.cpu().numpy().tobytes()


@pytest.mark.parametrize('name', ['grey', 'nv12'])
def test_no_margin_returns_the_warp_and_output_size_is_honoured(dev, clips, name):
    s, clip = stabilizer(dev), clips[name]
    out, report = s.online_session(**dict(SESSION, crop_margin=0)).push(clip)
    want = by_hand(s, clip, margin=0)
    same_frames(out, want[0], 'uncropped')
    assert report.rectangle == (0, 0, W - 1, H - 1)
    assert host_of(out)[0].shape == host_of(clip)[0].shape
    out, report = s.online_session(output_size=(96, 64), **SESSION).push(clip)
    same_frames(out, by_hand(s, clip, output_size=(96, 64))[0], 'output_size')
    assert tuple((out[0] if isinstance(out, tuple) else out).shape[1:3]) == (64, 96)


def test_a_lost_pair_is_reported_and_holds_the_path(dev):
    import torch
    s = stabilizer(dev)
    g = grey_clip()
    g[5] = 128                                                           # no corner in frame 5: pair (5, 6) cannot be fitted
    clip = torch.from_numpy(g).to(dev)
    out, report = s.online_session(**SESSION).push(clip)
    assert 6 in report.lost and set(report.lost) <= {5, 6}              # (the pair INTO the flat frame yields whatever LK makes of it)
    c = report.d_unstab.cpu().numpy()
    for t in report.lost:
        assert c[t].tobytes() == c[t - 1].tobytes()
    assert c[7].tobytes() != c[6].tobytes() and torch.isfinite(report.d_stab).all() and out.shape == clip.shape
    # the same when the flat frame ends one push and the lost pair spans two
    session = s.online_session(**SESSION)
    _, first = session.push(clip[:6])
    _, second = session.push(clip[6:])
    assert first.lost + second.lost == report.lost and second.first == 6
    tracker_clip.same_bits(torch.cat([first.d_stab, second.d_stab]).cpu().numpy(), report.d_stab.cpu().numpy(), 'd_stab')
    # 'raise': today's ValueError, and the session is where it was
    session = s.online_session(on_lost='raise', **SESSION)
    session.push(clip[:4])
    with pytest.raises(ValueError, match='fewer than 4 features could be tracked from frame %d to frame %d' % (report.lost[0] - 1, report.lost[0])):
        session.push(clip[4:])
    assert session.seen == 4
    _, r = session.push(clip[4:5])
    assert r.first == 4 and r.lost == []


def test_reset_starts_a_fresh_session(dev, clips, hand):
    s, clip = stabilizer(dev), clips['grey']
    session = s.online_session(**SESSION)
    session.push(clip[3:8])
    assert session.seen == 5
    session.reset()
    assert session.seen == 0
    out, report = session.push(clip)
    check_push(out, report, hand['grey'], 10)


def test_refusals(dev, clips):
    import torch
    s, clip = stabilizer(dev), clips['grey']
    session = s.online_session(**SESSION)
    session.push(clip[:2])
    for bad, match in ((clip[:2, :64].contiguous(), 'this session takes'), (clips['bgr'][:2], 'this session takes'), (part(clips['nv12'], 0, 2), 'this session takes'),
                       (clip.cpu()[:2], 'CUDA/HIP'), (torch.zeros((2, H, W), dtype=torch.uint16, device=dev), 'pass the pair')):
        with pytest.raises(ValueError, match=match):
            session.push(bad)
    assert session.seen == 2
    for kw, match in ((dict(crop_margin=0.5), r'crop_margin must lie in \[0, 0.5\)'), (dict(crop_margin=-0.01), 'crop_margin must lie'),
                      (dict(window=1), 'window must be in 2 .. 64'), (dict(window=65), 'window must be in 2 .. 64'),
                      (dict(iters=0), 'iters must be in 1 .. 1000'), (dict(beta=-1.0), 'beta must be finite'),
                      (dict(on_lost='skip'), "on_lost must be 'hold' or 'raise'"), (dict(adaptive_weights_definition=7), 'adaptive_weights_definition')):
        with pytest.raises(ValueError, match=match):
            s.online_session(**dict(SESSION, **kw))
    with pytest.raises(ValueError, match='leaves fewer than 2 x 2 pixels'):
        s.online_session(**SESSION).push(torch.zeros((1, 1, 8), dtype=torch.uint8, device=dev))     # (only a 1-pixel side can: floor(m (W - 1)) < (W - 1) / 2)
    with pytest.raises(ValueError, match='even width and height'):
        s.online_session(output_size=(95, 64), **SESSION).push(part(clips['nv12'], 0, 2))
