"""Cases for tools/ransac_body_check.cpp from tests/ransac_model.py: every crafted sub-frame of tests/ransac_cases.py under every parameter
set, the two sub-frames of the launch beyond the staged capacity, 60 cases of the planted recipe and the sub-frames of
tests/backend_edge_cases.py (the crafted ones again under 14 thresholds and confidences, the 64-candidate sub-frame at the iteration cap and
below it, the staging edge under two parameter sets, the hostile inputs), each with its threshold, confidence and the model's mask and info
record.
    python tools/ransac_dump_cases.py cases.bin"""
import os
import struct
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import backend_edge_cases as bc  # noqa: E402
import ransac_cases as rc  # noqa: E402
import ransac_model as rm  # noqa: E402


def main(path):
    cases = []                                      # (points, moved, count, found, min_features, threshold, confidence, max_iters, seed)
    points, counts, moved, found = rc.crafted()
    for max_iters, seed, min_features in rc.CRAFTED_PARAMS:
        for p in range(points.shape[0]):
            for s in range(points.shape[1]):
                cases.append((points[p, s], moved[p, s], counts[p, s], found[p, s], min_features, 3.0, 0.995, max_iters, seed))
    points, counts, moved, found = rc.beyond_staged(1024)
    for s in range(points.shape[1]):
        cases.append((points[0, s], moved[0, s], counts[0, s], found[0, s], 4, 3.0, 0.995, 2000, 0))
    for c in range(60):
        e, l, _ = rc.planted_case(c)
        cases.append((e, l, len(e), np.ones(len(e), np.uint8), 4, (3.0, 1.5)[c % 2], (0.995, 0.9)[c % 3 == 0], 2000, c))
    # tests/backend_edge_cases.py: thresholds and confidences off the defaults, the iteration cap, the staging edge (also under the chain's
    # parameters) and the hostile sub-frames
    points, counts, moved, found = rc.crafted()
    for threshold, confidence in bc.PARAM_SETS:
        for p in range(points.shape[0]):
            for s in range(points.shape[1]):
                cases.append((points[p, s], moved[p, s], counts[p, s], found[p, s], 4, threshold, confidence, 2000, 0))
    points, counts, moved, found = bc.cap_launch()
    for threshold, confidence, max_iters in bc.CAP_RUNS:
        cases.append((points[0, 0], moved[0, 0], counts[0, 0], found[0, 0], 4, threshold, confidence, max_iters, 0))
    for arrays, params in ((bc.staging_launch(), bc.DEFAULT), (bc.staging_launch(), tuple(bc.CHAIN_PARAMS[k] for k in ('threshold', 'confidence'))),
                           (bc.hostile_launch(), bc.DEFAULT)):
        points, counts, moved, found = arrays
        for p in range(points.shape[0]):
            for s in range(points.shape[1]):
                cases.append((points[p, s], moved[p, s], counts[p, s], found[p, s], 4, params[0], params[1], 2000, 0))
    with open(path, 'wb') as f:
        f.write(struct.pack('<ii', 0x43534e52, len(cases)))
        for e, l, count, fnd, min_features, threshold, confidence, max_iters, seed in cases:
            mask, info = rm.ransac_subframe(e, l, count, fnd, min_features, threshold, confidence, max_iters, seed)
            f.write(struct.pack('<iiiiIdd', len(e), int(count), min_features, max_iters, seed, threshold, confidence))
            for a in (np.asarray(e, np.float32), np.asarray(l, np.float32), np.asarray(fnd, np.uint8), mask, np.array(info, np.int32)):
                f.write(np.ascontiguousarray(a).tobytes())
    print('wrote %d cases to %s' % (len(cases), path))


if __name__ == '__main__':
    main(sys.argv[1])
