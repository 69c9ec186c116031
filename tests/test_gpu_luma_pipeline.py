"""Colour, BGRA, 16-bit and P010 clips through `estimate_motion` and `stabilize_scored`, byte for byte against the same calls on the MODEL luma
(tests/luma_model.py) uploaded as a grey clip, and against the compositions the new forms are documented as.  The clip is tests/luma_clip.py's:
tests/tracker_clip.py's 6-frame 128 x 96 clip g as B = 255 - g, G = g, R = g.  tests/test_luma_clip.py checks on the CPU that its model luma
and that of its cropped version fit a homography for every pair, so no call here ends in the tracker's ValueError."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import luma_clip as lc  # noqa: E402
import luma_model as lm  # noqa: E402
from tracker_clip import MAX_PER, stabilizer  # noqa: E402

pytestmark = pytest.mark.gpu

DEVICE = dict(max_per_subframe=MAX_PER, outliers='device', fit='device')


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def sources():
    """name -> (the clip as `ops.luma` takes it, its model luma)."""
    g = lc.grey()
    made = {'u8c3': lc.bgr(g), 'u8c4': lc.bgra(g), 'u16c3': lc.bgr16(g), 'p010 luma': lc.p010(g)[0]}
    return {name: (frames, lm.luma(frames)) for name, frames in made.items()}


def up(dev, array):
    import torch
    return torch.from_numpy(np.ascontiguousarray(array)).to(dev)


def motion(s, d_clip, **kw):
    """(d_disp, homographies) of `estimate_motion` as host arrays."""
    d_disp, hom = s.estimate_motion(d_clip, **kw)
    return d_disp.cpu().numpy(), hom


def same_bytes(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), what


def check_scores(s, dev, scores, luma_in, luma_cropped, stability):
    """The first two scores are those of the model lumas as grey stacks, the third is the stability score of the stabilized paths."""
    assert len(scores) == 3 and type(scores[0]) is np.float32 and type(scores[1]) is np.float32 and type(scores[2]) is float
    want = s.cropping_and_distortion_resident(up(dev, luma_in), up(dev, luma_cropped), max_per_subframe=MAX_PER)
    print('scores', scores, 'of the model lumas', want, 'stability', stability)
    same_bytes(np.array(scores[:2], np.float32), np.array(want, np.float32), 'cropping ratio and distortion score')
    assert scores[2] == stability


@pytest.mark.parametrize('name', ['u8c3', 'u8c4', 'u16c3', 'p010 luma'])
def test_estimate_motion_is_that_of_the_model_luma(dev, sources, name):
    s = stabilizer(dev)
    frames, y = sources[name]
    assert not np.array_equal(y, lc.grey()) or name == 'p010 luma'
    want = motion(s, up(dev, y), **DEVICE)
    got = motion(s, up(dev, frames), **DEVICE)
    same_bytes(got[0], want[0], (name, 'd_disp'))
    same_bytes(got[1], want[1], (name, 'homographies'))
    want = motion(s, up(dev, y), max_per_subframe=MAX_PER, outliers='host')
    got = motion(s, up(dev, frames), max_per_subframe=MAX_PER, outliers='host')
    same_bytes(got[0], want[0], (name, 'd_disp, outliers on the host'))
    same_bytes(got[1], want[1], (name, 'homographies, outliers on the host'))


@pytest.mark.parametrize('name', ['u8c3', 'u8c4', 'u16c3'])
def test_stabilize_scored_on_colour_frames(dev, sources, name):
    from meshflow_amd import ops
    s = stabilizer(dev)
    frames, y = sources[name]
    d_frames = up(dev, frames)
    cropped, scores = s.stabilize_scored(d_frames, max_per_subframe=MAX_PER)
    assert cropped.dtype == d_frames.dtype and tuple(cropped.shape) == frames.shape
    cropped = cropped.cpu().numpy()
    d_disp, hom = s.estimate_motion(d_frames, **DEVICE)
    _, _, d_stab, want_cropped = s.stabilize_resident(d_frames, d_disp, hom, crop=True)
    same_bytes(cropped, want_cropped.cpu().numpy(), (name, 'cropped clip'))
    check_scores(s, dev, scores, y, lm.luma(cropped), float(ops.stability_score(d_stab)[0].item()))
    same_bytes(d_frames.cpu().numpy(), frames, (name, 'the clip itself'))


def test_stabilize_scored_on_a_p010_pair(dev):
    import torch
    from meshflow_amd import ops
    s = stabilizer(dev)
    y, uv = lc.p010(lc.grey())
    d_y, d_uv = up(dev, y), up(dev, uv)
    (out_y, out_uv), scores = s.stabilize_scored((d_y, d_uv), max_per_subframe=MAX_PER, chunk_pairs=3)
    assert out_y.dtype == torch.uint16 and out_uv.dtype == torch.uint16
    out_y, out_uv = out_y.cpu().numpy(), out_uv.cpu().numpy()
    d_disp, hom = s.estimate_motion(up(dev, lm.luma(y)), **DEVICE)
    want_y, want_uv, _ = s.stabilized_p010_cropped(d_y, d_uv, d_disp, hom)
    same_bytes(out_y, want_y.cpu().numpy(), 'cropped luma')
    same_bytes(out_uv, want_uv.cpu().numpy(), 'cropped chroma')
    d_stab = s._stabilized_vertex_displacements_device(d_disp, lc.W, lc.H, s.ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, hom)
    check_scores(s, dev, scores, lm.luma(y), lm.luma(out_y), float(ops.stability_score(d_stab)[0].item()))


@pytest.mark.parametrize('name', ['u8c3', 'u8c4', 'u16c3'])
def test_red_first_on_the_reversed_clip_is_the_clip_itself(dev, sources, name):
    s = stabilizer(dev)
    frames, y = sources[name]
    flipped = lc.reversed_channels(frames)
    assert not np.array_equal(lm.luma(flipped), y) and np.array_equal(lm.luma(flipped, red_first=True), y)
    want = motion(s, up(dev, frames), **DEVICE)
    got = motion(s, up(dev, flipped), red_first=True, **DEVICE)
    same_bytes(got[0], want[0], (name, 'd_disp'))
    same_bytes(got[1], want[1], (name, 'homographies'))
    cropped, scores = s.stabilize_scored(up(dev, frames), max_per_subframe=MAX_PER)
    cropped = cropped.cpu().numpy()
    cropped_flipped, scores_flipped = s.stabilize_scored(up(dev, flipped), max_per_subframe=MAX_PER, red_first=True)
    same_bytes(lc.reversed_channels(cropped_flipped.cpu().numpy()), cropped, (name, 'cropped clip'))
    same_bytes(np.array(scores_flipped[:2], np.float32), np.array(scores[:2], np.float32), (name, 'scores'))
    assert scores_flipped[2] == scores[2]
    # read in the wrong order it is another clip
    other = motion(s, up(dev, flipped), **DEVICE)
    assert other[0].tobytes() != want[0].tobytes()


def test_a_grey_clip_gives_what_it_gave(dev):
    """The existing composition called directly, as tests/test_gpu_scores.py does; red_first means nothing to a grey clip."""
    from meshflow_amd import ops
    s = stabilizer(dev)
    g = lc.grey()
    d_grey = up(dev, g)
    for kw in ({}, {'red_first': True}):
        cropped, scores = s.stabilize_scored(d_grey, max_per_subframe=MAX_PER, **kw)
        cropped = cropped.cpu().numpy()
        d_disp, hom = s.estimate_motion(d_grey, **DEVICE, **kw)
        _, _, d_stab, want_cropped = s.stabilize_resident(d_grey, d_disp, hom, crop=True)
        same_bytes(cropped, want_cropped.cpu().numpy(), 'cropped clip')
        check_scores(s, dev, scores, g, cropped, float(ops.stability_score(d_stab)[0].item()))
