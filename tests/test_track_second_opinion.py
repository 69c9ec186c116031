"""tests/track_model.py against tests/track_definition.py: FAST scores and corners, pyrDown and the Scharr derivative restated from their
definitions, exactly equal on every image of tests/track_edge_cases.py (sections a-e), at every threshold of section b, and on the sizes
7 x 7, 8 x 9 and 23 x 45.  CPU only.  Were they to differ, one of the two is wrong, and the kernel follows the model."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import track_definition as td  # noqa: E402
import track_edge_cases as ec  # noqa: E402
import track_model as tm  # noqa: E402


def images():
    out = {name: img for name, (img, _, _) in ec.tall_cases().items()}
    out['threshold frame'] = ec.threshold_frame()
    out['binary'], out['binary blocks'] = ec.binary_frame(), ec.binary_frame(3)
    for x, y in ec.QUADRANT_CORNERS:
        out['quadrant %d %d' % (x, y)] = ec.quadrant(x, y)
    for i, lit in enumerate(ec.fewer_lit_sets()):
        out['fewer %d' % i] = ec.fewer_frame(lit)
    for name in ec.MIXED:
        out['mixed early ' + name], out['mixed late ' + name] = ec.mixed_pair(name)
    out['depth early'], out['depth late'] = ec.depth_pair()
    for name, early, late in ec.steep_pairs():
        out['steep early ' + name], out['steep late ' + name] = early, late
    out['checker early'], out['checker late'], _ = ec.checker_pair()
    for h, w in ((7, 7), (8, 9), (23, 45)):
        out['noise %d x %d' % (h, w)] = ec.noise(h, w, 40 + h)
        out['binary %d x %d' % (h, w)] = ec.binary(h, w, 50 + h)
    return out


IMAGES = images()


def same(a, b, what):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b), (what, a.shape, b.shape, np.argwhere(a != b)[:5].tolist())


@pytest.mark.parametrize('name', list(IMAGES))
def test_fast_by_definition(name):
    img = IMAGES[name]
    thresholds = list(ec.THRESHOLDS) if name == 'threshold frame' else [10]
    if name.startswith('binary'):
        thresholds = [1, 10, 254]
    for t in thresholds:
        same(tm.fast_scores(img, t), td.fast_scores(img, t), (name, t, 'scores'))
        same(tm.fast_corners(img, t), td.fast_corners(img, t), (name, t, 'corners'))


@pytest.mark.parametrize('name', list(IMAGES))
def test_pyr_down_and_scharr_by_definition(name):
    """Every level the tracker makes of the image, and one more (pyrDown itself does not know where the pyramid stops)."""
    img = IMAGES[name]
    for level in range(tm.num_levels(img.shape[1], img.shape[0]) + 2):
        ix, iy = tm.scharr(img)
        dx, dy = td.scharr(img)
        same(ix, dx, (name, level, 'Ix'))
        same(iy, dy, (name, level, 'Iy'))
        down = tm.pyr_down(img)
        same(down, td.pyr_down(img), (name, level, 'pyrDown'))
        img = down


@pytest.mark.parametrize('h,w', [(3, 3), (3, 4), (4, 3), (5, 8), (6, 5)])
def test_the_smallest_sizes(h, w):
    for seed in (60, 61):
        img = ec.noise(h, w, seed)
        same(tm.pyr_down(img), td.pyr_down(img), ('pyrDown', h, w))
        for a, b in zip(tm.scharr(img), td.scharr(img)):
            same(a, b, ('scharr', h, w))
        same(tm.fast_scores(img), td.fast_scores(img), ('scores', h, w))


def test_the_definition_knows_the_hand_worked_answers():
    """The definition is not only compared with the model: the known answers of tests/test_track_model.py hold for it too."""
    img = np.full((15, 15), 50, np.uint8)
    img[7, 8] = 200
    assert td.fast_corners(img).tolist() == [[8.0, 7.0]] and td.fast_scores(img)[7, 8] == 149 and np.count_nonzero(td.fast_scores(img)) == 1
    img = np.full((15, 15), 100, np.uint8)
    img[7, 7] = 110
    assert len(td.fast_corners(img)) == 0 and len(td.fast_corners(img, 9)) == 1
    img = np.full((15, 15), 0, np.uint8)
    img[7, 7] = 255
    assert td.fast_scores(img)[7, 7] == 254
    five = np.array([[10, 20, 30, 40, 50], [60, 70, 80, 90, 100], [110, 120, 130, 140, 150], [160, 170, 180, 190, 200],
                     [210, 220, 230, 240, 250]], np.uint8)
    assert td.pyr_down(five).tolist() == [[55, 68, 80], [118, 130, 143], [180, 193, 205]]
    ramp = (np.arange(12)[None, :] * 3 + np.zeros((9, 1))).astype(np.uint8)
    ix, iy = td.scharr(ramp)
    assert (ix[:, 1:-1] == 96).all() and (ix[:, 0] == 0).all() and (ix[:, -1] == 0).all() and (iy == 0).all()
