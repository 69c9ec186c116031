"""Every case of tests/backend_edge_cases.py reaches the path it is named for -- asserted with the models alone (tests/ransac_model.py,
tests/homography_model.py), before tests/test_gpu_backend_edges.py looks at a kernel's result.  The figures are the models' on these
inputs; a case whose condition fails needs another seed, never a weaker condition.  Model results are computed once per module; the
slowest, the two runs of the 65,536-iteration sub-frame, take some 15 s of model time together."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backend_edge_cases as bc  # noqa: E402
import homography_model as hm  # noqa: E402
import ransac_cases as rc  # noqa: E402
import ransac_model as rm  # noqa: E402


# ---- a. threshold and confidence off their defaults -------------------------------------------------------------------------------------

# (threshold, confidence) -> (sub-frames of the crafted launch whose mask or record differs from the default set's, mask bytes that differ)
DIFFERS = {(1e-3, 0.995): (12, 643), (0.1, 0.995): (12, 510), (0.5, 0.995): (11, 21), (1.0, 0.995): (2, 2), (2.5, 0.995): (1, 0),
           (20.0, 0.995): (2, 4), (1e6, 0.995): (10, 192), (3.0, 1e-300): (10, 460), (3.0, 0.5): (10, 19), (3.0, 0.9): (10, 2),
           (3.0, 0.999999): (10, 0), (3.0, 1 - 2 ** -53): (10, 0), (0.5, 0.5): (11, 82), (1e6, 1e-300): (10, 191)}


@pytest.fixture(scope='module')
def crafted_models():
    arrays = rc.crafted()
    return {p: rm.ransac_inliers(*arrays, threshold=p[0], confidence=p[1]) for p in (bc.DEFAULT,) + bc.PARAM_SETS}


def test_the_parameter_sets_are_the_ones_listed():
    assert bc.THRESHOLDS == (1e-3, 0.1, 0.5, 1.0, 2.5, 20.0, 1e6) and bc.CONFIDENCES == (1e-300, 0.5, 0.9, 0.999999, 1 - 2 ** -53)
    assert set(bc.PARAM_SETS) == set(DIFFERS) and len(bc.PARAM_SETS) == 14 and bc.DEFAULT not in bc.PARAM_SETS
    assert 1.0 - 1e-300 == 1.0 and 1 - 2 ** -53 < 1.0 and np.nextafter(1 - 2 ** -53, 2.0) == 1.0
    # two thresholds whose square is not exact: the host's threshold * threshold rounds
    from fractions import Fraction
    assert [t for t in bc.THRESHOLDS if Fraction(t) * Fraction(t) != Fraction(t * t)] == [1e-3, 0.1]


@pytest.mark.parametrize('params', bc.PARAM_SETS)
def test_every_parameter_set_changes_the_result(crafted_models, params):
    base, got = crafted_models[bc.DEFAULT], crafted_models[params]
    subframes = int(((got[0] != base[0]).any(axis=2) | (got[1] != base[1]).any(axis=2)).sum())
    assert subframes >= 1
    assert (subframes, int((got[0] != base[0]).sum())) == DIFFERS[params]


def test_confidence_reaches_the_lower_saturation(crafted_models):
    """1.0 - 1e-300 == 1.0: no t > p1 holds, n = 0, and a sub-frame ends with the iteration of its first consensus."""
    assert rm.iterations_needed(5, 64, 1e-300, 2000) == 1 and rm.iterations_needed(5, 64, 0.995, 2000) == 2000
    info = crafted_models[(3.0, 1e-300)][1].reshape(-1, 4)
    ok = info[info[:, 0] == rm.OK]
    assert len(ok) == 13 and ok[:, 3].max() < 2000
    arrays = rc.crafted()
    for p, s in np.argwhere(info.reshape(3, 6, 4)[:, :, 0] == rm.OK):
        _, record = rm.ransac_subframe(arrays[0][p, s], arrays[2][p, s], arrays[1][p, s], arrays[3][p, s], confidence=1e-300,
                                       max_iters=int(info.reshape(3, 6, 4)[p, s, 3]) - 1)
        assert record[0] == rm.NO_CONSENSUS                              # no consensus before the iteration it ended with


@pytest.fixture(scope='module')
def cap_models():
    arrays = bc.cap_launch()
    return [rm.ransac_inliers(*arrays, threshold=t, confidence=c, max_iters=m) for t, c, m in bc.CAP_RUNS]


def test_the_iteration_rule_saturates_and_the_cap_binds(cap_models):
    assert bc.CAP_RUNS == ((0.5, 0.995, 65536), (0.5, 0.5, 65536))
    capped, descended = (m[1][0, 0].tolist() for m in cap_models)
    assert capped == [rm.OK, 64, 5, 65536] and capped[3] == bc.CAP_MAX_ITERS
    assert descended == [rm.OK, 64, 5, 55819] and 4 < descended[3] < bc.CAP_MAX_ITERS
    # 5 of 64 at the default confidence: every one of the 17 steps of the descent is taken, n = 2^17 - 1
    assert rm.iterations_needed(5, 64, 0.995, 1 << 30) == 3 * ((1 << 17) - 1) + 1
    assert rm.iterations_needed(5, 64, 0.5, 1 << 30) == 55819


# ---- b. the staging edge ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def staging_model():
    return rm.ransac_inliers(*bc.staging_launch())


def test_staging_launch_sits_on_both_sides_of_the_capacity(staging_model):
    points, counts, moved, found = bc.staging_launch()
    assert points.shape == (2, 3, 1100, 2) and bc.STAGING_MAX % 64 != 0 and bc.STAGING_MAX > 1024
    assert counts.reshape(-1).tolist() == [K for K, _ in bc.STAGING] == [1100, 1100, 1100, 1025, 1024, 1100]
    info = staging_model[1].reshape(-1, 4)
    assert info[:, 1].tolist() == [k for _, k in bc.STAGING] == [1023, 1024, 1025, 1025, 1024, 1100]
    assert (info[:, 0] == rm.OK).all()
    assert info[:, 2].tolist() == [715, 712, 727, 717, 717, 770] and info[:, 3].tolist() == [58, 58, 55, 58, 58, 58]
    # holes in `found` in front of candidates: the compacted position is not the slot index, in LDS (slots 0, 1) and in the workspace (slot 2)
    flat = found.reshape(6, -1)
    for slot in (0, 1, 2):
        at = np.nonzero(flat[slot])[0]
        assert (at != np.arange(len(at))).sum() > 900, slot
    assert [int((flat[slot] == 0).sum()) for slot in range(6)] == [77, 76, 75, 75, 76, 0]
    from meshflow_amd import ops
    grid = ops.track_subframe_grid(*bc.STAGING_GRID)
    assert grid[2] * grid[3] == points.shape[1] == 3                     # (the gather takes a grid of as many sub-frames as a pair has)
    assert rm.gather(points, moved, *staging_model, grid, 4)[2].tolist() == [0, 715 + 712 + 727, 715 + 712 + 727 + 717 + 717 + 770]


# ---- c. hostile sub-frame inputs --------------------------------------------------------------------------------------------------------

def test_hostile_launch_reaches_every_clamp():
    points, counts, moved, found = bc.hostile_launch()
    assert counts[0].tolist() == [72, 72, -1, -2 ** 31, 2 ** 31 - 1, 72]
    assert sorted(set(found[0, 1].tolist())) == [0, 51, 102, 153, 204] and set(found[0, [0, 2, 3, 4, 5]].reshape(-1).tolist()) == {1}
    bad = points[0, 0]
    assert np.isnan(bad[5, 0]) and bad[9].tolist() == [np.inf, -np.inf] and bad[20].tolist() == [np.float32(1e30)] * 2
    assert np.signbit(bad[33, 0]) and not np.signbit(bad[33, 1]) and (bad[33] == 0).all()
    assert (bad[40] > 0).all() and (bad[40] < np.finfo(np.float32).tiny).all()         # subnormals: neither zero nor normal
    assert np.isnan(moved[0, 5]).all() and np.isfinite(moved[0, :5]).all() and np.isfinite(points[0, 1:]).all()
    inlier, info = rm.ransac_inliers(points, counts, moved, found)
    assert info[0].tolist() == [[rm.OK, 72, 55, 37], [rm.OK, 57, 47, 25], [rm.TOO_FEW, 0, 0, 0], [rm.TOO_FEW, 0, 0, 0], [rm.OK, 72, 58, 28],
                                [rm.NO_CONSENSUS, 72, 0, 2000]]
    assert (inlier[0, 1][found[0, 1] == 0] == 0).all() and inlier[0, 1].sum() == 47
    assert inlier[0, 0][[5, 9, 20]].tolist() == [0, 0, 0] and inlier[0, 2:4].sum() == 0 and inlier[0, 5].sum() == 0


# ---- d. records that contradict their masks ---------------------------------------------------------------------------------------------

def test_untrusted_records_truncate_leave_gaps_and_drop_a_pair():
    from meshflow_amd import ops
    grid = ops.track_subframe_grid(*bc.UNTRUSTED_GRID)
    points, moved, inlier, info, honest = bc.untrusted_launch()
    n, S, size = points.shape[:3]
    assert (n, S, size) == (3, 4, 72) and grid[2] * grid[3] == S
    pop = (inlier != 0).sum(axis=2)
    assert pop.tolist() == [[58, 65, 42, 58], [65, 50, 58, 11], [50, 58, 65, 50]] and (honest[:, :, 0] == rm.OK).all()
    assert (honest[:, :, 2] == pop).all()
    # every edit of the list is there
    assert (info[0, :, 2] - pop[0]).tolist() == [0, -5, 9, 2 ** 31 - 1 - 58] and info[1, :, 2].tolist() == [0, -3, -2 ** 31, 11]
    assert info[2, :, 0].tolist() == [7, -1, rm.TOO_FEW, rm.OK] and (pop[2, :3] > 0).all()
    assert sorted(set(inlier[2, 3].tolist())) == [0, 2, 255] and sorted(set(inlier[:2].reshape(-1).tolist())) == [0, 1]
    # on honest records the contract is the model's gather, and everything behind the survivors keeps the sentinel
    for min_features in bc.UNTRUSTED_MIN_FEATURES + (200,):
        want = rm.gather(points, moved, inlier, honest, grid, min_features)
        got = bc.gather_untrusted(points, moved, inlier, honest, grid, min_features)
        total = int(want[2][-1])
        assert np.array_equal(got[0][:total], want[0]) and np.array_equal(got[1][:total], want[1])
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3])
        assert bc.is_sentinel(got[0][total:]).all() and bc.is_sentinel(got[1][total:]).all() and not bc.is_sentinel(got[0][:total]).any()
    assert rm.gather(points, moved, inlier, honest, grid, 200)[3].tolist() == [0, rm.PAIR_TOO_FEW, 0]
    # the edited records
    kept = [[58, 60, 51, 72], [0, 0, 0, 11], [0, 0, 0, 50]]
    for min_features, offsets, status in ((4, [0, 241, 252, 302], [0, 0, 0]), (20, [0, 241, 241, 291], [0, rm.PAIR_TOO_FEW, 0])):
        early, late, got_offsets, got_status = bc.gather_untrusted(points, moved, inlier, info, grid, min_features)
        assert got_offsets.tolist() == offsets and got_status.tolist() == status and len(early) == len(late) == n * S * size == 864
        untouched = bc.is_sentinel(early)
        assert np.array_equal(untouched, bc.is_sentinel(late))
        assert untouched[offsets[3]:].all() and int(untouched[:offsets[3]].sum()) == 23
        runs = {}
        for p in range(n):
            at = offsets[p]
            for s in range(S):
                if status[p] == 0:
                    runs[p, s] = untouched[at:at + kept[p][s]]
                    at += kept[p][s]
        # the honest run and the truncated one are full; the truncated one leaves 5 set mask entries out; two runs end in a sentinel gap
        assert not runs[0, 0].any() and not runs[0, 1].any() and kept[0][1] == pop[0, 1] - 5
        assert runs[0, 2].tolist() == [False] * 42 + [True] * 9 and runs[0, 3].tolist() == [False] * 58 + [True] * 14
        assert not runs[2, 3].any() and len(runs[2, 3]) == 50
        sub_w, sub_h, _, rows = grid
        first = np.nonzero(inlier[0, 1])[0][:60]
        assert np.array_equal(early[58:118], points[0, 1][first].astype(np.float64) + np.array([0.0, sub_h]))
    # pair 1 at min_features 20: its masks hold 184 bits and its honest records keep it; the clamped records alone drop it
    assert pop[1].sum() == 184 and rm.gather(points, moved, inlier, honest, grid, 20)[3][1] == 0 and sum(kept[1]) == 11 < 20


# ---- e. the fit outside pixel scale -----------------------------------------------------------------------------------------------------

# name -> the model's (status, sweeps, index of the chosen eigenvalue) at 40 and at 300 points
FIT_RECORDS = {
    'x 1e6': ((hm.OK, 7, 4), (hm.OK, 7, 0)),
    'x 1e70': ((hm.AT_INFINITY, 7, 4), (hm.AT_INFINITY, 7, 0)),
    'x 1e100': ((hm.COLLINEAR, 0, 0), (hm.COLLINEAR, 0, 0)),
    'x 1e-100': ((hm.COLLINEAR, 0, 0), (hm.COLLINEAR, 0, 0)),
    'x 1e-150': ((hm.COLLINEAR, 0, 0), (hm.COLLINEAR, 0, 0)),
    '2 micropixels at 100': ((hm.OK, 7, 4), (hm.OK, 7, 0)),
    '2 micropixels, y x 1e-5': ((hm.COLLINEAR, 0, 0), (hm.COLLINEAR, 0, 0)),
    'y x 3e-9': ((hm.OK, 6, 1), (hm.OK, 5, 1)),
    'y x 1e-9': ((hm.COLLINEAR, 0, 0), (hm.COLLINEAR, 0, 0)),
    'y x last accepted': ((hm.OK, 6, 1), (hm.COLLINEAR, 0, 0)),
    'y x first refused': ((hm.COLLINEAR, 0, 0), (hm.COLLINEAR, 0, 0)),
    'late mirrored': ((hm.OK, 7, 4), (hm.OK, 7, 0)),
    'late hashed': ((hm.OK, 6, 1), (hm.OK, 6, 1)),
    'early[7] NaN': ((hm.COLLINEAR, 0, 0), (hm.COLLINEAR, 0, 0)),
    'late[7] +inf': ((hm.COLLINEAR, 0, 0), (hm.COLLINEAR, 0, 0)),
}


@pytest.fixture(scope='module')
def fit_model():
    names, early, late, offsets = bc.fit_launch()
    with np.errstate(all='ignore'):
        return names, offsets, hm.fit_homographies(early, late, offsets)


def test_fit_launch_statuses(fit_model):
    names, offsets, (H, info, diag) = fit_model
    assert list(FIT_RECORDS) == list(bc.FIT_CASES) and len(names) == 2 * len(bc.FIT_CASES) == 30
    assert np.diff(offsets).tolist() == [40] * 15 + [300] * 15
    for i, name in enumerate(bc.FIT_CASES):
        for j, K in enumerate(bc.FIT_SIZES):
            p = j * len(bc.FIT_CASES) + i
            assert names[p] == '%s, K=%d' % (name, K)
            assert info[p].tolist() == [FIT_RECORDS[name][j][0], K] + list(FIT_RECORDS[name][j][1:]), names[p]
            assert info[p, 0] == bc.FIT_CASES[name][1 + j], names[p]
    assert sorted(set(info[:15, 0].tolist())) == sorted(set(info[15:, 0].tolist())) == [hm.OK, hm.COLLINEAR, hm.AT_INFINITY]
    assert set(info[:15, 2].tolist()) == {0, 6, 7} and set(info[15:, 2].tolist()) == {0, 5, 6, 7}
    # a refused pair gets the identity; a NaN appears only in diag of the pair with a NaN coordinate, an infinity only beside the infinity
    assert np.isfinite(H).all() and all(np.array_equal(H[p], np.identity(3)) for p in np.nonzero(info[:, 0] != hm.OK)[0])
    nan, inf = [names.index('%s, K=%d' % (bc.NON_FINITE[0], K)) for K in bc.FIT_SIZES], [names.index('%s, K=%d' % (bc.NON_FINITE[1], K)) for K in bc.FIT_SIZES]
    assert np.argwhere(np.isnan(diag)).tolist() == [[nan[0], 2], [nan[1], 2]] and np.argwhere(np.isinf(diag)).tolist() == [[inf[0], 4], [inf[1], 4]]
    assert (diag[inf, 4] > 0).all()


def test_the_flat_clouds_are_the_edge_of_the_collinearity_test():
    accepted, refused = bc.bisect_flat()
    assert (accepted, refused) == (bc.FLAT_ACCEPTED, bc.FLAT_REFUSED) and 1e-9 < refused < accepted < 3e-9
    assert np.nextafter(refused, 1.0) == accepted                        # adjacent doubles
    e, l = bc.fit_cloud(40)
    for factor, want in ((accepted, False), (refused, True)):
        fe, fl = bc.flattened(factor)(e, l)
        _, info, diag = hm.fit_pair(fe, fl)
        assert (info[0] == hm.COLLINEAR) == want
        # ... and it is hfit::collinear on the moments that decides, for one of the two clouds
        assert (hm.collinear(*second_moments(fe, diag[2:4])) or hm.collinear(*second_moments(fl, diag[4:6]))) == want


def second_moments(cloud, centre):
    d = cloud - centre
    return hm.ordered_sum(np.stack([d[:, 0] * d[:, 0], d[:, 0] * d[:, 1], d[:, 1] * d[:, 1]], 1))


@pytest.mark.parametrize('K', bc.FIT_SIZES)
def test_the_flat_micropixel_cloud_is_refused_by_the_floor_of_one(K):
    """larger eigenvalue about 1e-11, determinant between 1e-18 larger^2 and 1e-18 larger: collinear only because the test reads
    max(larger, 1)."""
    e, l = bc.FIT_CASES['2 micropixels, y x 1e-5'][0](*bc.fit_cloud(K))
    _, info, diag = hm.fit_pair(e, l)
    assert info[0] == hm.COLLINEAR
    for a, b, c in (second_moments(e, diag[2:4]), second_moments(l, diag[4:6])):
        big = (a + c) * 0.5 + np.sqrt(((a - c) * 0.5) ** 2 + b * b)
        det = a * c - b * b
        assert big < 1e-9 and 100 * ((1e-18 * big) * big) < det and 100 * det < 1e-18 * big and hm.collinear(a, b, c)     # (far from either bound)


def test_no_scale_reaches_not_converged():
    """NOT_CONVERGED stays unreached: none of the 122 fits of the search ends there, and none needs more than 7 of the 30 sweeps."""
    seen, reached, most = bc.not_converged_search()
    assert reached == [] and seen == {hm.COLLINEAR: 113, hm.AT_INFINITY: 6, hm.OK: 3} and most == 7


# ---- f. the chain -----------------------------------------------------------------------------------------------------------------------

def test_the_chain_hands_two_large_pairs_to_the_fit():
    from meshflow_amd import ops
    (inlier, info), (early, late, offsets, status), (H, fit_info, diag) = bc.chain_model(ops.track_subframe_grid(*bc.STAGING_GRID))
    assert bc.CHAIN_PARAMS == {'threshold': 1.0, 'confidence': 0.9}
    assert info.reshape(-1, 4).tolist() == [[rm.OK, 1023, 690, 33], [rm.OK, 1024, 701, 28], [rm.OK, 1025, 642, 40], [rm.OK, 1025, 717, 25],
                                            [rm.OK, 1024, 717, 46], [rm.OK, 1100, 770, 25]]
    assert offsets.tolist() == [0, 2033, 4237] and status.tolist() == [0, 0] and len(early) == len(late) == 4237
    assert fit_info.tolist() == [[hm.OK, 2033, 7, 0], [hm.OK, 2204, 7, 0]] and np.isfinite(H).all() and np.isfinite(diag).all()
