"""tests/homography_model.py, the specification of the device homography fit, against `host.lsq_homography` on the planted cases of
tests/hfit_cases.py, and its refusals, records and invariances.  CPU only.

The measure is the largest distance in pixels between the two matrices' images of the frame's four corners.  Measured on the committed recipe
(180 cases: K = 4 .. 500, noise 0 / 0.3 / 1 px, a 1080p frame and one sub-frame in the corner of a 4K frame): worst 5.2e-6 px (4 points with
0.3 px noise in the 4K corner, where the smallest eigenvalue is rounding noise and the second one small), median 1e-11 px, at most 9 sweeps.
The bar is ten times that worst case -- the factor covers other LAPACK builds and the exact 4-point fits -- and lies below BASELINE's 1e-4."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hfit_cases as hc  # noqa: E402
import homography_model as hm  # noqa: E402
from meshflow_amd import host  # noqa: E402

WORST_MEASURED = 5.2e-6
BAR = 10 * WORST_MEASURED


@pytest.fixture(scope='module')
def planted():
    """[(name, frame, H, info, diag, host's H)] of the 180 planted cases, computed once."""
    return [(name, frame) + hm.fit_pair(e, l) + (host.lsq_homography(e, l),) for name, frame, e, l in hc.planted_cases()]


@pytest.fixture(scope='module')
def crafted():
    names, early, late, offsets = hc.crafted()
    return names, early, late, offsets, hm.fit_homographies(early, late, offsets)


def test_the_model_agrees_with_the_host_fit(planted):
    assert BAR < 1e-4
    distances = [hc.corner_distance(H, want, frame) for _, frame, H, _, _, want in planted]
    worst = int(np.argmax(distances))
    print('worst %.3g px (%s), median %.3g px' % (distances[worst], planted[worst][0], float(np.median(distances))))
    assert len(planted) == 180
    for (name, _, H, info, _, _), d in zip(planted, distances):
        assert info[0] == hm.OK and H[2, 2] == 1.0, name
        assert d <= BAR, (name, d)


def test_sweeps_and_records(planted, crafted):
    records = [(name, info, diag) for name, _, _, info, diag, _ in planted] + list(zip(crafted[0], crafted[4][1], crafted[4][2]))
    for name, info, diag in records:
        assert 0 <= info[2] <= hm.MAX_SWEEPS and 0 <= info[3] < 9, (name, info)
        if info[0] == hm.OK:
            assert 1 <= info[2] < hm.MAX_SWEEPS, (name, info)
            assert diag[0] > 0 and diag[1] > 0 and diag[6] <= diag[7], (name, diag)
            assert abs(diag[6]) <= 1e-3 * info[1], (name, diag)                  # the algebraic error of a planted pair is small
    assert max(info[2] for _, info, _ in records) <= 12


def test_scales_and_centroids_are_the_hosts(planted):
    """diag restates `host._normalisation` in another order of summation: equal to rounding."""
    for (name, _, _, _, diag, _), (_, _, e, l) in zip(planted, hc.planted_cases()):
        for cloud, scale, centre in ((e, diag[0], diag[2:4]), (l, diag[1], diag[4:6])):
            t = host._normalisation(cloud)
            assert abs(scale / t[0, 0] - 1) < 1e-13, name
            assert np.abs(centre + t[:2, 2] / t[0, 0]).max() < 1e-9, name


def test_every_refusal(crafted):
    names, early, late, offsets, (H, info, diag) = crafted
    status = dict(zip(names, info[:, 0].tolist()))
    want = {'K=0': hm.TOO_FEW, 'K=3': hm.TOO_FEW, 'empty': hm.TOO_FEW, 'collinear': hm.COLLINEAR, 'late collinear': hm.COLLINEAR,
            'identical': hm.COLLINEAR, 'h22 vanishes': hm.AT_INFINITY}
    for name in names:
        assert status[name] == want.get(name, hm.OK), (name, status[name])
    assert info[:, 1].tolist() == np.diff(offsets).tolist()
    for p, name in enumerate(names):
        if info[p, 0] != hm.OK:
            assert np.array_equal(H[p], np.identity(3)), name                    # identity + flag
        if info[p, 0] == hm.TOO_FEW:
            assert not diag[p].any() and not info[p, 2:].any(), name
        if info[p, 0] == hm.COLLINEAR:
            assert not diag[p, :2].any() and not diag[p, 6:].any() and diag[p, 2:6].all(), name
    at = names.index('h22 vanishes')
    assert diag[at, :6].all() and abs(diag[at, 6]) < 1e-12 and info[at, 2] > 0
    assert hm.first_refused(info) == 0 and hm.first_refused(info[4:9]) is None and hm.first_refused(info[2:]) == names.index('empty') - 2
    # the host refuses the same pairs
    for name in ('K=3', 'collinear', 'late collinear', 'identical', 'h22 vanishes'):
        p = names.index(name)
        with pytest.raises(ValueError):
            host.lsq_homography(early[offsets[p]:offsets[p + 1]], late[offsets[p]:offsets[p + 1]])


def test_not_converged_is_reported():
    """No planted pair gets there, so the loop's other exit is reached with a matrix that cannot converge: a NaN entry keeps rotating."""
    N = [[float(i == j) for j in range(9)] for i in range(9)]
    N[0][1] = N[1][0] = float('nan')
    _, sweeps, converged = hm.jacobi(N)
    assert sweeps == hm.MAX_SWEEPS and not converged


def test_the_exact_pairs_are_exact(crafted):
    names, early, late, offsets, (H, info, diag) = crafted
    for name, bar in (('exact 4', 1e-9), ('noise-free 100', 1e-9)):
        p = names.index(name)
        e, l = early[offsets[p]:offsets[p + 1]], late[offsets[p]:offsets[p + 1]]
        q = np.concatenate([e, np.ones((len(e), 1))], 1) @ H[p].T
        assert np.abs(q[:, :2] / q[:, 2:] - l).max() < bar, name
        assert abs(diag[p, 6]) < 1e-12 < diag[p, 7], (name, diag[p])


def test_empty_pairs_between_full_ones_and_bad_ranges(crafted):
    names, early, late, offsets, (H, info, diag) = crafted
    a, b = names.index('before the empty pair'), names.index('after the empty pair')
    assert info[a, 0] == info[b, 0] == hm.OK and info[a + 1, 0] == hm.TOO_FEW and b == a + 2
    # ranges that are not ranges of the inputs are read as empty, whatever stands around them
    bad = offsets.copy()
    bad[a + 1] = -5
    H2, info2, _ = hm.fit_homographies(early, late, bad)
    assert info2[a].tolist() == [hm.TOO_FEW, 0, 0, 0] and info2[a + 1].tolist() == [hm.TOO_FEW, 0, 0, 0]
    assert np.array_equal(H2[b], H[b]) and np.array_equal(H2[a - 1], H[a - 1])
    bad = offsets.copy()
    bad[-1] = len(early) + 1
    assert hm.fit_homographies(early, late, bad)[1][-1].tolist() == [hm.TOO_FEW, 0, 0, 0]
    bad = offsets.copy()
    bad[5], bad[6] = offsets[6], offsets[5]                                      # decreasing
    info3 = hm.fit_homographies(early, late, bad)[1]
    assert info3[5].tolist() == [hm.TOO_FEW, 0, 0, 0]


def test_a_pair_does_not_depend_on_its_surroundings(crafted):
    names, early, late, offsets, (H, info, diag) = crafted
    for p in (4, 7, names.index('near 3,840')):
        lo, hi = offsets[p], offsets[p + 1]
        pad = np.full((7, 2), 1e6)
        e, l = np.concatenate([pad, early[lo:hi], -pad]), np.concatenate([-pad, late[lo:hi], pad])
        H1, info1, diag1 = hm.fit_homographies(e, l, np.array([0, 7, 7 + hi - lo, len(e)], np.int32))
        assert H1[1].tobytes() == H[p].tobytes() and info1[1].tobytes() == info[p].tobytes() and diag1[1].tobytes() == diag[p].tobytes(), names[p]


def test_the_order_of_the_sums_is_the_stated_one():
    """`ordered_sum` against the order written out with scalars: 256 strided partials, a halving tree per 64, (w0 + w1) + (w2 + w3)."""
    from meshflow_amd import synthetic
    for k in (1, 63, 256, 257, 700):
        terms = (synthetic.uniform01(np.arange(2 * k), 7 + k).reshape(k, 2) - 0.5) * np.array([1.0, 1e6])
        for column in range(2):
            partial = [0.0] * 256
            for i in range(k):
                partial[i % 256] = partial[i % 256] + float(terms[i, column])
            waves = []
            for w in range(4):
                v = partial[64 * w:64 * w + 64]
                step = 32
                while step:
                    for j in range(step):
                        v[j] = v[j] + v[j + step]
                    step //= 2
                waves.append(v[0])
            assert hm.ordered_sum(terms)[column] == (waves[0] + waves[1]) + (waves[2] + waves[3]), (k, column)


def test_the_largest_pair_takes_the_model_milliseconds():
    import time
    early, late, offsets = hc.largest()
    start = time.perf_counter()
    H, info, _ = hm.fit_homographies(early, late, offsets)
    assert info[0].tolist()[:2] == [hm.OK, 16384] and time.perf_counter() - start < 2.0
