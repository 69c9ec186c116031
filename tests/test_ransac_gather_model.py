"""The model gather (tests/ransac_model.py `gather`) on a 2-pair, 3 x 2 sub-frame grid whose last column and row are smaller: the order of
the survivors, the float64 offsets, empty sub-frames, a pair below min_features (empty range + flag), and equality with
`host.pack_features` over `finish_pair` with the model in place of `host.ransac_inliers`.  No GPU."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ransac_cases as rc  # noqa: E402
import ransac_model as rm  # noqa: E402

W, H, ROWS, COLS, MAX = 100, 75, 2, 3, 40


def launch():
    """Pair 0: five sub-frames with planted sets, one empty; pair 1: a single sub-frame with 6 candidates, the others empty or too few."""
    L = rc.Launch(2, 6, MAX)
    for s, (k, fraction) in enumerate(((30, 0.2), (12, 0.0), (0, 0.0), (40, 0.3), (3, 0.0), (25, 0.1))):
        e, l, _ = rc.planted(max(k, 1), fraction, 50 + s)
        L.add(e[:k], l[:k])
    for s, k in enumerate((0, 2, 6, 0, 3, 0)):
        e, l, _ = rc.planted(max(k, 1), 0.0, 60 + s)
        L.add(e[:k], l[:k])
    return L.arrays()


def grid():
    from meshflow_amd import ops
    g = ops.track_subframe_grid(W, H, ROWS, COLS)
    assert g == (34, 38, 3, 2)                                           # columns of 34, 34, 32 pixels; rows of 38 and 37
    return g


def test_order_offsets_and_empty_subframes():
    points, counts, moved, found = launch()
    inlier, info = rm.ransac_inliers(points, counts, moved, found)
    assert info[0, :, 0].tolist() == [rm.OK, rm.OK, rm.TOO_FEW, rm.OK, rm.TOO_FEW, rm.OK]
    assert info[1, :, 0].tolist() == [rm.TOO_FEW, rm.TOO_FEW, rm.OK, rm.TOO_FEW, rm.TOO_FEW, rm.TOO_FEW]
    early, late, offsets, status = rm.gather(points, moved, inlier, info, grid(), 4)
    assert early.dtype == late.dtype == np.float64 and offsets.dtype == np.int32 and status.tolist() == [0, 0]
    per = info[:, :, 2]
    assert offsets.tolist() == [0, per[0].sum(), per[0].sum() + per[1].sum()] and len(early) == len(late) == offsets[-1] and per[1].sum() == 6
    at = 0
    for p in range(2):
        for s in range(6):                                               # sub-frame s = column * 2 + row starts at (column * 34, row * 38)
            idx = np.nonzero(inlier[p, s])[0]
            assert (np.diff(idx) > 0).all()
            off = np.array([(s // 2) * 34, (s % 2) * 38], np.float64)
            assert np.array_equal(early[at:at + len(idx)], points[p, s, idx].astype(np.float64) + off)
            assert np.array_equal(late[at:at + len(idx)], moved[p, s, idx].astype(np.float64) + off)
            at += len(idx)
    assert at == offsets[-1]


def test_a_pair_below_min_features_is_empty_and_flagged():
    points, counts, moved, found = launch()
    inlier, info = rm.ransac_inliers(points, counts, moved, found, min_features=5)
    assert info[1, 2].tolist()[:3] == [rm.OK, 6, 6]
    total0 = int(info[0, :, 2].sum())
    early, _, offsets, status = rm.gather(points, moved, inlier, info, grid(), 7)          # 6 survivors < 7 (mfs.py:521)
    assert offsets.tolist() == [0, total0, total0] and status.tolist() == [0, rm.PAIR_TOO_FEW] and len(early) == total0
    early, _, offsets, status = rm.gather(points, moved, inlier, info, grid(), total0 + 1)
    assert offsets.tolist() == [0, 0, 0] and status.tolist() == [rm.PAIR_TOO_FEW] * 2 and early.shape == (0, 2)
    early, _, offsets, status = rm.gather(points[::-1], moved[::-1], inlier[::-1], info[::-1], grid(), 7)   # the flagged pair first
    assert offsets.tolist() == [0, 0, total0] and status.tolist() == [rm.PAIR_TOO_FEW, 0] and len(early) == total0


def test_equals_pack_features_of_finish_pair_with_the_model():
    from meshflow_amd import host
    points, counts, moved, found = launch()
    for min_features in (4, 7):
        inlier, info = rm.ransac_inliers(points, counts, moved, found, min_features)
        early, late, offsets, status = rm.gather(points, moved, inlier, info, grid(), min_features)
        pairs = [rm.finish_pair(grid(), points[p], counts[p], moved[p], found[p], min_features) for p in range(2)]
        want_early, want_late, want_offsets, _ = host.pack_features([(e, l) for e, l, _ in pairs])
        assert [h is None for _, _, h in pairs] == [bool(f) for f in status]
        assert early.tobytes() == want_early.tobytes() and late.tobytes() == want_late.tobytes() and offsets.tolist() == want_offsets.tolist()
