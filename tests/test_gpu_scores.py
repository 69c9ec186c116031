"""The device feature scores against their specification, tests/scores_model.py, bit for bit: `ops.feature_scores` (the two scores, every
pair's two values, the record) on launches of planted matrices whose lengths sit on the edges of the 256-lane fold, with fit records that
refuse the first, the last, a middle pair and all of them, and on the matrices where IEEE decides; then the stabilizer's
`cropping_and_distortion_resident` and `stabilize_scored` end to end on tests/tracker_clip.py's clip against the model pipeline on the same
bytes (tests/track_model.py corners and LK -> model RANSAC -> model fit -> model scores), as tests/test_gpu_hfit.py builds its own."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import homography_model as hm  # noqa: E402
import ransac_model as rm  # noqa: E402
import scores_cases as sc  # noqa: E402
import scores_model as sm  # noqa: E402
import tracker_clip  # noqa: E402
from tracker_clip import MAX_PER, model_corners, model_lk, same_bits, stabilizer  # noqa: E402

pytestmark = pytest.mark.gpu

PAIRS = (1, 63, 64, 65, 255, 256, 257, 513, 1000)
W, H = 128, 96
# inclusive (left, top, right, bottom): the whole frame and crops that scale by at most 1.15 per axis (a 1.33x crop of this small clip loses track)
RECTS = ((0, 0, 127, 95), (8, 6, 119, 89), (4, 3, 123, 92), (8, 0, 119, 95))
# |cropping_ratio - crop area / frame area| at the most: twice the model pipeline's own worst deviation on RECTS, measured on the CPU with
# the oracle's crop-resize (which the device's equals bit for bit): 0.00000, 0.01137, 0.00698, 0.00021 (rounded up) (profiles/feature_scores.md)
MARGIN = 2 * 0.01137


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def run(dev, homographies, info=None):
    import torch
    from meshflow_amd import ops
    d_h = torch.from_numpy(np.ascontiguousarray(homographies)).to(dev)
    d_info = None if info is None else torch.from_numpy(np.ascontiguousarray(info)).to(dev)
    out = ops.feature_scores(d_h, d_info)
    assert ops.feature_scores_check(out[2]) == sm.first_unscored(out[2].cpu().numpy())
    return tuple(t.cpu().numpy() for t in out)


def compare(got, want, what):
    """Record first, then pair by pair: a mismatch names its pair and its value."""
    same_bits(got[2], want[2], (what, 'record', got[2].tolist(), want[2].tolist()))
    for p in range(len(want[1])):
        for i, field in enumerate(('ratio', 'distortion')):
            same_bits(got[1][p, i:i + 1], want[1][p, i:i + 1], (what, 'pair', p, field, float(got[1][p, i]), float(want[1][p, i])))
    same_bits(got[0][:1], want[0][:1], (what, 'cropping_ratio', float(got[0][0]), float(want[0][0])))
    same_bits(got[0][1:], want[0][1:], (what, 'distortion_score', float(got[0][1]), float(want[0][1])))


@pytest.mark.parametrize('pairs', PAIRS)
def test_a_launch_equals_the_model(dev, pairs):
    h = sc.launch(pairs)
    compare(run(dev, h), sm.feature_scores(h), 'no record')
    compare(run(dev, h, sc.record(pairs, [])), sm.feature_scores(h), 'nothing refused')
    for name, refused in (('first', [0]), ('last', [pairs - 1]), ('middle', [pairs // 2]), ('three', sorted({0, pairs // 3, pairs - 1})),
                          ('all', list(range(pairs)))):
        info = sc.record(pairs, refused)
        want = sm.feature_scores(h, info)
        assert want[2].tolist() == [pairs - len(refused), refused[0]]
        compare(run(dev, h, info), want, name)


def test_every_planted_branch_and_ieee_case_equals_the_model(dev):
    for name, h in sc.planted() + sc.special():
        compare(run(dev, h[None]), sm.feature_scores(h[None]), name)
    special = np.stack([h for _, h in sc.special()])
    compare(run(dev, special), sm.feature_scores(special), 'the IEEE cases in one clip')
    mixed = np.concatenate([sc.launch(300), special])
    names = [n for n, _ in sc.special()]
    info = sc.record(len(mixed), [300 + i for i, n in enumerate(names) if 'NaN' in n or 'infinite' in n])
    want = sm.feature_scores(mixed, info)
    assert np.isfinite(want[0][1]) and np.isnan(want[0][0])               # inf and -inf among the ratios, no NaN among the scored distortions
    compare(run(dev, mixed, info), want, 'NaN pairs refused')


def test_two_launches_give_the_same_bytes(dev):
    h, info = sc.launch(1000), sc.record(1000, [3, 500])
    a, b = run(dev, h, info), run(dev, h, info)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_a_prefix_scored_alone_gives_the_same_pairs(dev):
    h = sc.launch(1000)
    info = sc.record(1000, [0, 64, 300])
    whole, whole_info = run(dev, h), run(dev, h, info)
    for n in (1, 64, 65, 257, 513):
        same_bits(run(dev, h[:n])[1], whole[1][:n], ('prefix', n))
        same_bits(run(dev, h[:n], info[:n])[1], whole_info[1][:n], ('prefix with a record', n))


# ---- end to end on the tracker's clip ----

@pytest.fixture(scope='module')
def clip():
    return tracker_clip.clip()


def model_scores(early_stack, late_stack):
    """The model pipeline on the pairs (early_stack[t], late_stack[t]): (scores, per_pair, record)."""
    from meshflow_amd import ops
    grid = ops.track_subframe_grid(W, H, 2, 2)
    fits = []
    for early, late in zip(early_stack, late_stack):
        points, counts, _ = model_corners(early, 2, 2, MAX_PER)
        moved, found = model_lk(early, late, 2, 2, points, counts)
        inlier, info = rm.ransac_inliers(points[None], counts[None], moved[None], found[None], 4)
        e, l, _, _ = rm.gather(points[None], moved[None], inlier, info, grid, 4)
        fits.append(hm.fit_pair(e, l))
    return sm.feature_scores(np.stack([f[0] for f in fits]), np.stack([f[1] for f in fits]))


@pytest.mark.parametrize('rect', RECTS, ids=['%d-%d-%d-%d' % r for r in RECTS])
def test_the_scores_of_a_crop_equal_the_model_pipeline(dev, clip, rect):
    import torch
    from meshflow_amd import ops
    s = stabilizer(dev)
    d_grey = torch.from_numpy(clip).to(dev)
    d_cropped = ops.crop_resize(d_grey, rect)
    want, per_pair, record = model_scores(clip, d_cropped.cpu().numpy())
    assert record.tolist() == [6, -1]
    for chunk_pairs in (32, 4):
        got = s.cropping_and_distortion_resident(d_grey, d_cropped, chunk_pairs=chunk_pairs, max_per_subframe=MAX_PER)
        assert len(got) == 2 and all(type(v) is np.float32 for v in got)
        print('rect', rect, 'scores', got, 'model', want, 'ratios', per_pair[:, 0])
        same_bits(np.array(got, np.float32), want, (rect, chunk_pairs, got, want.tolist()))
    geometric = (rect[2] - rect[0] + 1) * (rect[3] - rect[1] + 1) / (W * H)
    assert abs(float(got[0]) - geometric) <= MARGIN, (rect, got, geometric)
    assert 0.0 < got[1] <= 1.0
    if rect == (0, 0, W - 1, H - 1):
        assert got == (1.0, 1.0)                                         # the fits are the identity to 1e-13


def nv12_chroma(frames):
    from meshflow_amd import synthetic
    return (synthetic.hash32(np.arange(frames * (H // 2) * (W // 2) * 2), 5) % 256).astype(np.uint8).reshape(frames, H // 2, W // 2, 2)


def test_stabilize_scored_on_a_grey_clip(dev, clip):
    import torch
    from meshflow_amd import ops
    s = stabilizer(dev)
    d_grey = torch.from_numpy(clip).to(dev)
    cropped, scores = s.stabilize_scored(d_grey, max_per_subframe=MAX_PER)
    d_disp, hom = s.estimate_motion(d_grey, max_per_subframe=MAX_PER, outliers='device', fit='device')
    _, _, d_stab, want_cropped = s.stabilize_resident(d_grey, d_disp, hom, crop=True)
    same_bits(cropped.cpu().numpy(), want_cropped.cpu().numpy(), 'cropped clip')
    assert tuple(cropped.shape) == (6, H, W) and cropped.dtype == torch.uint8
    want, _, record = model_scores(clip, cropped.cpu().numpy())
    assert record.tolist() == [6, -1]
    print('grey scores', scores, 'model', want)
    assert len(scores) == 3 and type(scores[0]) is np.float32 and type(scores[1]) is np.float32 and type(scores[2]) is float
    same_bits(np.array(scores[:2], np.float32), want, ('grey', scores, want.tolist()))
    assert scores[2] == float(ops.stability_score(d_stab)[0].item())
    assert 0.5 < scores[0] <= 1.05 and 0.5 < scores[1] <= 1.0 and 0.0 < scores[2] <= 1.0


def test_stabilize_scored_on_an_nv12_clip(dev, clip):
    import torch
    from meshflow_amd import ops
    s = stabilizer(dev)
    d_y, d_uv = torch.from_numpy(clip).to(dev), torch.from_numpy(nv12_chroma(len(clip))).to(dev)
    (out_y, out_uv), scores = s.stabilize_scored((d_y, d_uv), max_per_subframe=MAX_PER, chunk_pairs=3)
    d_disp, hom = s.estimate_motion(d_y, max_per_subframe=MAX_PER, outliers='device', fit='device')
    want_y, want_uv, _ = s.stabilized_nv12(d_y, d_uv, d_disp, hom, crop=True)
    same_bits(out_y.cpu().numpy(), want_y.cpu().numpy(), 'cropped luma')
    same_bits(out_uv.cpu().numpy(), want_uv.cpu().numpy(), 'cropped chroma')
    want, _, record = model_scores(clip, out_y.cpu().numpy())
    assert record.tolist() == [6, -1]
    print('nv12 scores', scores, 'model', want)
    same_bits(np.array(scores[:2], np.float32), want, ('nv12', scores, want.tolist()))
    d_stab = s._stabilized_vertex_displacements_device(d_disp, W, H, s.ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, hom)
    assert type(scores[2]) is float and scores[2] == float(ops.stability_score(d_stab)[0].item())


def test_a_flat_frame_raises_and_names_it(dev, clip):
    """Frame 2 flat in both stacks (a clip that fades through grey keeps nothing of it in the crop either), and in the unstabilized stack
    alone: no corner, no fit, the ValueError names the frame.  A flat CROPPED frame under a textured unstabilized one is not refused by this
    tracker -- pyramidal LK takes its gradients from the early frame and reports every point found, and the outlier step finds a consensus
    among them --: the model pipeline scores it (ratio 1.45 on this clip), and so does the device, bit for bit."""
    import torch
    s = stabilizer(dev)
    flat = clip.copy()
    flat[2] = 128
    d_grey, d_flat = torch.from_numpy(clip).to(dev), torch.from_numpy(flat).to(dev)
    for early, late, d_early, d_late in ((flat, flat, d_flat, d_flat), (flat, clip, d_flat, d_grey)):
        assert model_scores(early, late)[2].tolist() == [5, 2]
        for chunk_pairs in (32, 2):
            with pytest.raises(ValueError, match='fewer than 4 features could be tracked from unstabilized frame 2 to cropped frame 2'):
                s.cropping_and_distortion_resident(d_early, d_late, chunk_pairs=chunk_pairs, max_per_subframe=MAX_PER)
    want, _, record = model_scores(clip, flat)
    assert record.tolist() == [6, -1]
    got = s.cropping_and_distortion_resident(d_grey, d_flat, max_per_subframe=MAX_PER)
    same_bits(np.array(got, np.float32), want, ('flat cropped frame', got, want.tolist()))


def test_unequal_shapes_raise_before_any_launch(dev, clip):
    import torch
    s = stabilizer(dev)
    d_grey = torch.from_numpy(clip).to(dev)
    torch.cuda.synchronize()
    for shape in ((6, 48, 64), (5, H, W), (6, W, H)):
        with pytest.raises(ValueError, match="need the crop at the clip's own size"):
            s.cropping_and_distortion_resident(d_grey, torch.zeros(shape, dtype=torch.uint8, device=dev))
