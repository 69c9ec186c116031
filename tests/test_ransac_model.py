"""tests/ransac_model.py, the specification of the device outlier step, against planted data and its own rules.  No GPU.

The planted recipe (tests/ransac_cases.py: k hashed in 20 .. 300, integer early points in a 480 x 270 sub-frame, a homography within 1 % of
the identity, +-0.25 px noise, 0 / 0.1 / 0.3 / 0.5 of the points displaced by 12 .. 60 px per axis, float32 storage) carries two caps, both
checked against the model alone: NO planted outlier is accepted, and at least 0.85 of the planted inliers are kept in every case.  They are
checked on 300 cases under each of five seed bases.  With cv2's iteration count alone (N = n + 1) the model misses the recall cap on two
of the five -- worst recalls 0.824, 0.905, 0.944, 0.862, 0.835 -- because the search ends on a first mediocre consensus that is never
refitted; with N = 3 n + 1, the rule of the model, the worst recalls are 0.961, 0.983, 0.957, 0.983, 0.983, no outlier is accepted, the
iterations run have a median of 35.5 and a maximum of 295, and no case ends without consensus.  (`host.ransac_inliers` on the 300 cases of
the second base: none accepted, worst recall 0.920.)"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_cases as rc  # noqa: E402
import ransac_model as rm  # noqa: E402


@pytest.mark.parametrize('base', rc.PLANTED_BASES)
def test_planted_no_outlier_accepted_and_recall(base):
    accepted, without, recall, ran = 0, 0, [], []
    for case in range(300):
        early, late, outlier = rc.planted_case(case, base)
        mask, (status, k, inliers, iterations) = rm.ransac_subframe(early, late, len(early), np.ones(len(early), np.uint8))
        mask = mask.astype(bool)
        accepted += int((mask & outlier).sum())
        without += status != rm.OK
        recall.append((mask & ~outlier).sum() / (~outlier).sum())
        ran.append(iterations)
        assert k == len(outlier) and inliers == mask.sum() and 1 <= iterations <= 2000
    print('base %d: outliers accepted %d, worst recall %.3f, iterations run median %g max %d, cases without consensus %d'
          % (base, accepted, min(recall), np.median(ran), max(ran), without))
    assert accepted == 0
    assert min(recall) >= 0.85, min(recall)
    assert without == 0


def test_four_exact_correspondences_are_all_kept():
    early = np.float32([[10, 10], [200, 30], [180, 220], [25, 190]])
    late = np.float32([[12, 9], [203, 31], [181, 224], [26, 188]])
    mask, info = rm.ransac_subframe(early, late, 4, np.ones(4, np.uint8))
    assert mask.tolist() == [1, 1, 1, 1] and info[:3] == (rm.OK, 4, 4) and info[3] == 1          # N(4, 4) = 1 ends the search


def test_collinear_identical_and_too_few():
    mask, info = rm.ransac_subframe(*rc.collinear(30), 30, np.ones(30, np.uint8), max_iters=300)
    assert not mask.any() and info == (rm.NO_CONSENSUS, 30, 0, 300)
    mask, info = rm.ransac_subframe(*rc.identical(10), 10, np.ones(10, np.uint8), max_iters=50)
    assert not mask.any() and info == (rm.NO_CONSENSUS, 10, 0, 50)
    early, late, _ = rc.planted(8, 0.0, 3)
    mask, info = rm.ransac_subframe(early[:3], late[:3], 3, np.ones(3, np.uint8))
    assert not mask.any() and info == (rm.TOO_FEW, 3, 0, 0)
    found = np.ones(8, np.uint8)
    found[2:7] = 0
    assert rm.ransac_subframe(early, late, 8, found)[1] == (rm.TOO_FEW, 3, 0, 0)                 # k = 3 of K = 8
    assert rm.ransac_subframe(early, late, 8, np.ones(8, np.uint8), min_features=9)[1] == (rm.TOO_FEW, 8, 0, 0)       # mfs.py:614
    assert rm.ransac_subframe(early, late, 8, np.ones(8, np.uint8))[1][0] == rm.OK
    found = np.ones(8, np.uint8)
    found[0] = 0
    assert rm.ransac_subframe(early, late, 8, found, min_features=8)[1] == (rm.TOO_FEW, 7, 0, 0)                      # mfs.py:626
    assert rm.ransac_subframe(early, late, 0, np.ones(8, np.uint8))[1] == (rm.TOO_FEW, 0, 0, 0)
    assert rm.ransac_subframe(early, late, 100, np.ones(8, np.uint8))[1][1] == 8                 # a count above the slots is read as the slots


def test_iteration_rule():
    from meshflow_amd import host
    for k, max_iters in ((100, 2000), (7, 2000), (300, 65536), (100, 5)):
        n = [rm.iterations_needed(c, k, 0.995, max_iters) for c in range(4, k + 1)]
        assert all(a >= b for a, b in zip(n, n[1:])), (k, n)
        assert all(1 <= v <= max_iters for v in n) and n[-1] == 1
    for c in (30, 50, 80, 100):                     # N = 3 n + 1 with n + 1 equal to or one more than cv2's formula, as host.py restates it
        n = (rm.iterations_needed(c, 100, 0.995, 2000) - 1) // rm.OVERSAMPLE
        assert (rm.iterations_needed(c, 100, 0.995, 2000) - 1) % rm.OVERSAMPLE == 0
        assert n + 1 - host._ransac_iterations(0.995, (100 - c) / 100, 2000) in (0, 1), c
    assert rm.iterations_needed(4, 100, 0.995, 2000) == rm.iterations_needed(10, 100, 0.995, 2000) == 2000
    assert rm.iterations_needed(100, 100, 0.995, 2000) == 1 and host._ransac_iterations(0.995, 0.0, 2000) == 0
    assert rm.iterations_needed(4, 4000, 0.5, 65536) == 65536             # the descent's 2^17 - 1 is beyond the largest max_iters


def test_same_bits_twice_and_the_seed_changes_the_samples():
    early, late, _ = rc.planted(150, 0.5, 9)
    found = np.ones(150, np.uint8)
    a, b = rm.ransac_subframe(early, late, 150, found), rm.ransac_subframe(early.copy(), late.copy(), 150, found.copy())
    assert a[0].tobytes() == b[0].tobytes() and a[1] == b[1]
    assert [rm.draw_sample(it, 0, 150) for it in range(8)] == [rm.draw_sample(it, 0, 150) for it in range(8)]
    assert [rm.draw_sample(it, 0, 150) for it in range(8)] != [rm.draw_sample(it, 1, 150) for it in range(8)]
    for it in range(50):
        for k in (4, 5, 150):
            s = rm.draw_sample(it, 3, k)
            assert s is None or (len(set(s)) == 4 and all(0 <= v < k for v in s))
    assert any(rm.draw_sample(it, 3, 4) is None for it in range(50))     # 16 draws among 4 values miss one now and then: the iteration is skipped
    assert rm.ransac_subframe(early, late, 150, found, seed=1)[1][0] == rm.OK
    # with the search cut to 3 iterations the result is whatever those samples gave: the seeds do not all agree
    assert len({rm.ransac_subframe(early, late, 150, found, max_iters=3, seed=seed)[0].tobytes() for seed in range(6)}) > 1


def test_huge_and_non_finite_positions_are_never_inliers():
    early, late, outlier = rc.planted(80, 0.1, 34)
    bad = [3, 17, 40, 41, 63, 64]
    late[3], late[17], late[40], late[41], late[63], late[64] = (1e7, 5), (np.inf, 3), (np.nan, np.nan), (-np.inf, np.inf), (4, -1e7), (1e7, 1e7)
    for seed in range(6):
        mask, info = rm.ransac_subframe(early, late, 80, np.ones(80, np.uint8), seed=seed)
        assert info[0] == rm.OK and not mask[bad].any() and not (mask.astype(bool) & outlier).any()
    everything = np.full((12, 2), np.nan, np.float32)
    assert rm.ransac_subframe(early[:12], everything, 12, np.ones(12, np.uint8), max_iters=40)[1] == (rm.NO_CONSENSUS, 12, 0, 40)
    everything[:] = np.inf
    assert rm.ransac_subframe(everything, late[:12], 12, np.ones(12, np.uint8), max_iters=40)[1] == (rm.NO_CONSENSUS, 12, 0, 40)
