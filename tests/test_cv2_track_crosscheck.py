"""tests/track_model.py against OpenCV itself, wherever `cv2` is importable (nowhere this project is built or tested today: the file skips).
FAST corners must agree exactly.  LK positions agree up to the float32 rounding of the five window sums, which cv2 accumulates in float32 in
a SIMD-dependent order and the model takes exactly: each sum carries a relative error of at most 441 x 2^-24 = 2.6e-5 in cv2, the update is a
ratio of such sums of at most a few pixels, and at most 30 updates per level over 4 levels add up -- well below TOLERANCE = 0.01 pixel, cv2's
own convergence threshold, which bounds how far two runs that stop one iteration apart can differ.  Measure the largest difference on the
first machine that has cv2 and record it in profiles/tracker.md."""
import os
import sys

import numpy as np
import pytest

cv2 = pytest.importorskip('cv2')
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_model as tm  # noqa: E402
from test_track_model import texture  # noqa: E402

TOLERANCE = 0.01


def frames():
    from meshflow_amd import synthetic
    noise = (synthetic.hash32(np.arange(48 * 64), 1) & 255).astype(np.uint8).reshape(48, 64)
    return [noise, texture(120, 160), texture(37, 61), synthetic.frames_numpy(1, 96, 128, seed=2)[0, :, :, 1].copy()]


def test_fast_corners_equal_cv2():
    for img in frames():
        want = cv2.KeyPoint_convert(cv2.FastFeatureDetector_create().detect(img))
        want = np.float32(want).reshape(-1, 2)
        assert np.array_equal(tm.fast_corners(img), want)


def test_pyramid_equals_cv2():
    for img in frames():
        for level, want in zip(tm.build_pyramid(img)[1:], (cv2.pyrDown(img), cv2.pyrDown(cv2.pyrDown(img)))):
            assert np.array_equal(level, want)


@pytest.mark.parametrize('dx,dy', [(2.25, -1.5), (6, -6), (0, 0), (-3.5, 4)])
def test_lk_agrees_with_cv2_up_to_the_float32_sums(dx, dy):
    early, late = texture(120, 160), texture(120, 160, dx, dy)
    ys, xs = np.mgrid[2:120:9, 3:160:11]
    points = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32)
    want, status, _ = cv2.calcOpticalFlowPyrLK(early, late, points[:, None, :], None)
    moved, found = tm.lk_track(early, late, points)
    assert np.array_equal(found, status.ravel())
    both = found.astype(bool)
    worst = np.abs(moved[both] - want[:, 0][both]).max()
    print('largest |model - cv2| over %d tracks: %.3g px' % (both.sum(), worst))
    assert worst <= TOLERANCE, worst
