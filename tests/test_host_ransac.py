"""host.ransac_inliers and host.lsq_homography, the deterministic stand-ins for cv2.findHomography behind the device tracker."""
import numpy as np
import pytest

from meshflow_amd import host, synthetic

PLANTED = np.array([[1.01, 0.02, 5.0], [-0.015, 0.99, -3.0], [1e-5, -2e-5, 1.0]])


def apply(h, p):
    q = np.c_[p, np.ones(len(p))] @ h.T
    return q[:, :2] / q[:, 2:]


def planted(seed=1):
    """200 pairs under PLANTED (coordinates below 2,000, float64, no noise), then 60 pairs displaced by 20 .. 70 pixels."""
    idx = np.arange(260)
    early = np.stack([synthetic.uniform01(idx, seed) * 1900, synthetic.uniform01(idx, seed + 1) * 1000], 1)
    late = apply(PLANTED, early)
    angle, radius = synthetic.uniform01(idx[:60], seed + 2) * 2 * np.pi, 20 + synthetic.uniform01(idx[:60], seed + 3) * 50
    late[200:] += np.stack([radius * np.cos(angle), radius * np.sin(angle)], 1)
    return early, late


@pytest.mark.parametrize('seed', [1, 10, 20])
def test_the_planted_inliers_are_found_exactly_and_refitted(seed):
    early, late = planted(seed)
    mask = host.ransac_inliers(early, late)
    assert mask.dtype == bool and mask.shape == (260,)
    assert mask[:200].all() and not mask[200:].any()
    h = host.lsq_homography(early[mask], late[mask])
    assert h.shape == (3, 3) and h[2, 2] == 1.0
    error = np.abs(apply(h, early[:200]) - late[:200]).max()
    assert error < 1e-6, error                 # float64 DLT on normalised points: ~1e-12 relative on coordinates <= 2,000
    # the (K, 1, 2) arrays the tracker hands over, float32 or float64, are taken as they are
    assert np.array_equal(host.ransac_inliers(early[:, None, :], late[:, None, :]), mask)


def test_the_same_inputs_give_identical_bits():
    early, late = planted()
    a, b = host.ransac_inliers(early, late), host.ransac_inliers(early.copy(), late.copy())
    assert np.array_equal(a, b)
    ha, hb = host.lsq_homography(early[a], late[a]), host.lsq_homography(early[b], late[b])
    assert ha.tobytes() == hb.tobytes()
    shuffled = host.ransac_inliers(early, late, seed=5)            # another sample sequence, the same consensus
    assert np.array_equal(shuffled, a)


def test_too_few_and_collinear_points_are_refused():
    early, late = planted()
    line = np.c_[np.arange(12.0), 3.0 * np.arange(12.0) + 1]
    for fn in (host.ransac_inliers, host.lsq_homography):
        with pytest.raises(ValueError, match='at least 4'):
            fn(early[:3], late[:3])
        with pytest.raises(ValueError, match='one line'):
            fn(line, line + 2.0)
        with pytest.raises(ValueError, match='one line'):
            fn(early[:12], line)
        with pytest.raises(ValueError, match='same number'):
            fn(early[:10], late[:9])
        with pytest.raises(ValueError):
            fn(early[:, :1], late[:, :1])


def test_iteration_count_follows_cv2s_formula():
    assert host._ransac_iterations(0.995, 0.0, 2000) == 0
    assert host._ransac_iterations(0.995, 1.0, 2000) == 2000
    assert host._ransac_iterations(0.995, 0.5, 2000) == 82          # log(0.005) / log(1 - 0.5^4) = 82.09
    assert host._ransac_iterations(0.995, 60 / 260, 2000) == 12     # log(0.005) / log(1 - (200 / 260)^4) = 12.3
