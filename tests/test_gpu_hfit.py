"""The device homography fit against its specification, tests/homography_model.py, bit for bit: `ops.fit_homographies` (H, all four info
fields and all eight diag fields) on the crafted launch of tests/hfit_cases.py -- pair sizes on the edges of the 256-lane reduction, an empty
pair between two full ones, collinear and identical clouds, exact fits, coordinates near 3,840, a vanishing h22 --, on one pair of 16,384
points, and `estimate_motion(outliers='device', fit='device')` end to end against the model pipeline (tests/track_model.py corners and LK ->
model RANSAC -> model fit).  diag carries both scales, so a device sqrt that is not correctly rounded on this range shows there first."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hfit_cases as hc  # noqa: E402
import homography_model as hm  # noqa: E402
import ransac_model as rm  # noqa: E402
import tracker_clip  # noqa: E402
from tracker_clip import MAX_PER, SHIFTS, model_corners, model_lk, same_bits, stabilizer  # noqa: E402

pytestmark = pytest.mark.gpu

# tests/test_homography_model.py's bar: ten times the worst distance measured on the CPU between the model and host.lsq_homography
BAR = 10 * 5.2e-6


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def crafted():
    names, early, late, offsets = hc.crafted()
    return names, early, late, offsets, hm.fit_homographies(early, late, offsets)


def run_fit(dev, early, late, offsets):
    import torch
    from meshflow_amd import ops
    out = ops.fit_homographies(*(torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (early, late, offsets)))
    return tuple(t.cpu().numpy() for t in out)


def compare(got, want, names):
    """diag first and field by field: a mismatch names its stage."""
    for p, name in enumerate(names):
        for i, field in enumerate(('early scale', 'late scale', 'early cx', 'early cy', 'late cx', 'late cy', 'smallest eigenvalue', 'second eigenvalue')):
            same_bits(got[2][p, i:i + 1], want[2][p, i:i + 1], (name, field, float(got[2][p, i]), float(want[2][p, i])))
        same_bits(got[1][p], want[1][p], (name, 'info', got[1][p].tolist(), want[1][p].tolist()))
        same_bits(got[0][p], want[0][p], (name, 'H'))
    for g, w, what in zip(got, want, ('H', 'info', 'diag')):
        same_bits(g, w, what)


def test_the_crafted_launch_equals_the_model(dev, crafted):
    names, early, late, offsets, want = crafted
    assert np.diff(offsets).tolist()[:9] == list(hc.CRAFTED_SIZES)
    assert sorted(set(want[1][:, 0].tolist())) == [hm.OK, hm.TOO_FEW, hm.COLLINEAR, hm.AT_INFINITY]
    compare(run_fit(dev, early, late, offsets), want, names)


def test_the_largest_pair_equals_the_model(dev):
    early, late, offsets = hc.largest()
    want = hm.fit_homographies(early, late, offsets)
    assert want[1][0].tolist()[:2] == [hm.OK, 16384]
    compare(run_fit(dev, early, late, offsets), want, ['16,384 points'])


def test_two_launches_give_the_same_bytes(dev, crafted):
    _, early, late, offsets, _ = crafted
    a, b = run_fit(dev, early, late, offsets), run_fit(dev, early, late, offsets)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_a_pair_does_not_depend_on_the_other_pairs(dev, crafted):
    """Pairs of the crafted launch alone, behind a prefix of other points, and with ranges around them that are no ranges of the inputs."""
    names, early, late, offsets, want = crafted
    for p in (5, 7, 8, names.index('after the empty pair'), names.index('h22 vanishes')):
        lo, hi = int(offsets[p]), int(offsets[p + 1])
        alone = run_fit(dev, early[lo:hi], late[lo:hi], np.array([0, hi - lo], np.int32))
        shifted = run_fit(dev, early[lo - 3:], late[lo - 3:], np.array([0, 3, 3 + hi - lo, len(early) - lo + 3], np.int32))
        for g, s, w in zip(alone, shifted, want):
            same_bits(g[0], w[p], (names[p], 'alone'))
            same_bits(s[1], w[p], (names[p], 'shifted'))
    bad = offsets.copy()
    bad[1], bad[12] = -7, len(early) + 100                                # pairs 0, 1 and 11, 12 lose their ranges; nothing is read outside
    got = run_fit(dev, early, late, bad)
    same_bits(got[1], hm.fit_homographies(early, late, bad)[1], 'info with bad ranges')
    for p in range(len(names)):
        if p not in (0, 1, 11, 12):
            same_bits(got[0][p], want[0][p], (names[p], 'H beside bad ranges'))
        else:
            assert got[1][p].tolist() == [hm.TOO_FEW, 0, 0, 0] and np.array_equal(got[0][p], np.identity(3)), p


@pytest.fixture(scope='module')
def clip():
    return tracker_clip.clip()


@pytest.fixture(scope='module')
def model_pairs(clip):
    """The model pipeline per pair: tests/track_model.py corners and LK -> model RANSAC and gather -> (early, late) or None."""
    from meshflow_amd import ops
    grid = ops.track_subframe_grid(128, 96, 2, 2)
    out = []
    for early, late in zip(clip[:-1], clip[1:]):
        points, counts, _ = model_corners(early, 2, 2, MAX_PER)
        moved, found = model_lk(early, late, 2, 2, points, counts)
        inlier, info = rm.ransac_inliers(points[None], counts[None], moved[None], found[None], 4)
        e, l, _, _ = rm.gather(points[None], moved[None], inlier, info, grid, 4)
        out.append((e, l))
    return out


def test_estimate_motion_with_the_device_fit_equals_the_model_pipeline(dev, clip, model_pairs):
    import torch
    from meshflow_amd import host, ops
    s = stabilizer(dev)
    d_grey = torch.from_numpy(clip).to(dev)
    want_h = np.stack([hm.fit_pair(e, l)[0] for e, l in model_pairs] + [np.identity(3)])
    for chunk_pairs in (32, 2):
        d_disp, hom = s.estimate_motion(d_grey, chunk_pairs=chunk_pairs, max_per_subframe=MAX_PER, outliers='device', fit='device')
        same_bits(hom, want_h, ('homographies', chunk_pairs))
        assert d_disp.is_cuda and d_disp.dtype == torch.float64 and tuple(d_disp.shape) == (6, 5, 5, 2)
        early, late, offsets, kmax = host.pack_features(model_pairs)
        want_disp, _, status = ops.vertex_motion(*(torch.from_numpy(a).to(dev) for a in (early, late, offsets, np.ascontiguousarray(want_h[:-1]))),
                                                 kmax, 128, 96, 4, 4, s.feature_ellipse_row_count, s.feature_ellipse_col_count)
        assert int(status.item()) == 0
        same_bits(d_disp.cpu().numpy(), want_disp.cpu().numpy(), ('d_disp', chunk_pairs))
    # the other mode's result: within the bar measured on the CPU, and the motion of the clip
    _, hom_host = s.estimate_motion(d_grey, max_per_subframe=MAX_PER, outliers='device')
    for t in range(5):
        assert hc.corner_distance(hom[t], hom_host[t], (128, 96)) <= BAR, t
        centre = hom[t] @ np.array([64.0, 48.0, 1.0])
        assert np.abs(centre[:2] / centre[2] - np.array([64.0, 48.0]) - np.array(SHIFTS[t])).max() < 0.5, (t, centre)
    # the tracker's own view of the same clip
    got = s.device_tracker(MAX_PER, outliers='device', fit='device').track_clip_resident(d_grey, chunk_pairs=3)
    assert got[3] == max(len(e) for e, _ in model_pairs) and ops.fit_check(got[5]) is None
    same_bits(got[4].cpu().numpy(), want_h[:-1], 'track_clip_resident')
    same_bits(got[2].cpu().numpy(), host.pack_features(model_pairs)[2], 'offsets')


def test_an_untrackable_pair_raises_todays_error(dev, clip):
    import torch
    s = stabilizer(dev)
    flat = clip.copy()
    flat[2] = 128                                                        # pair (2, 3) has no corner in any sub-frame
    d_flat = torch.from_numpy(flat).to(dev)
    got = s.device_tracker(MAX_PER, outliers='device', fit='device').track_clip_resident(d_flat, chunk_pairs=2)
    info = got[5].cpu().numpy()
    assert info[2].tolist() == [hm.TOO_FEW, 0, 0, 0] and info[0, 0] == hm.OK and info[4, 0] == hm.OK
    assert np.array_equal(got[4][2].cpu().numpy(), np.identity(3))
    first = int(np.nonzero(info[:, 0] != hm.OK)[0][0])
    assert first in (1, 2)                                               # (pair (1, 2), into the flat frame, yields what the model pipeline yields)
    with pytest.raises(ValueError, match='fewer than 4 features could be tracked from frame %d to frame %d' % (first, first + 1)):
        s.estimate_motion(d_flat, max_per_subframe=MAX_PER, outliers='device', fit='device')
    # ... the pair the host fit names as well
    with pytest.raises(ValueError, match='fewer than 4 features could be tracked from frame %d to frame %d' % (first, first + 1)):
        s.estimate_motion(d_flat, max_per_subframe=MAX_PER, outliers='device')
