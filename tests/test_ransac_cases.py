"""The crafted sub-frames of tests/ransac_cases.py hold what tests/test_gpu_ransac.py relies on: the model's own view of them.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_cases as rc  # noqa: E402
import ransac_model as rm  # noqa: E402


def test_the_crafted_launch_holds_what_it_says():
    """Every k of the lane-stride tails, every status, the cap on the iterations, the effect of the seed and of min_features."""
    crafted = rc.crafted()
    points, counts, moved, found = crafted
    crafted_model = {p: rm.ransac_inliers(points, counts, moved, found, min_features=p[2], max_iters=p[0], seed=p[1]) for p in rc.CRAFTED_PARAMS}
    _, info = crafted_model[(2000, 0, 4)]
    info = info.reshape(18, 4)
    assert info[:8, 1].tolist() == list(rc.CRAFTED_TAILS) and info[8, 1] == rc.CRAFTED_MAX and counts.reshape(-1)[8] > rc.CRAFTED_MAX
    assert info[9].tolist() == [rm.TOO_FEW, 0, 0, 0] and info[10, 1] == 50
    assert info[:, 0].tolist() == [rm.TOO_FEW, rm.TOO_FEW] + [rm.OK] * 7 + [rm.TOO_FEW, rm.OK, rm.OK, rm.NO_CONSENSUS, rm.NO_CONSENSUS] + [rm.OK] * 4
    assert info[12].tolist() == [rm.NO_CONSENSUS, 30, 0, 2000] and info[13].tolist() == [rm.NO_CONSENSUS, 10, 0, 2000]
    assert (crafted_model[(1, 0, 4)][1][..., 3] <= 1).all() and crafted_model[(7, 0, 4)][1][..., 3].max() == 7
    assert crafted_model[(2000, 0, 10)][1].reshape(18, 4)[16].tolist() == [rm.TOO_FEW, 8, 0, 0]
    assert not np.array_equal(crafted_model[(2000, 0, 4)][1], crafted_model[(2000, 5, 4)][1])


def test_the_case_beyond_the_staged_capacity():
    points, counts, moved, found = rc.beyond_staged(1024)
    assert points.shape == (1, 2, 1089, 2) and counts.tolist() == [[70, 1089]] and found[0, 1].all()
