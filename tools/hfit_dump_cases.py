"""Cases for tools/hfit_body_check.cpp from tests/homography_model.py: every pair of the crafted launch of tests/hfit_cases.py, the 16,384-point
pair, the 180 planted cases and the pairs of tests/backend_edge_cases.py (the fit outside pixel scale, at 40 and at 300 points, and the two
pairs of its chain), each with the model's H, info and diag.
    python tools/hfit_dump_cases.py cases.bin"""
import os
import struct
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import backend_edge_cases as bc  # noqa: E402
import hfit_cases as hc  # noqa: E402
import homography_model as hm  # noqa: E402
from meshflow_amd import ops  # noqa: E402


def main(path):
    cases = []
    _, early, late, offsets = hc.crafted()
    cases += [(early[a:b], late[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]
    early, late, _ = hc.largest()
    cases.append((early, late))
    cases += [(e, l) for _, _, e, l in hc.planted_cases()]
    # tests/backend_edge_cases.py: the fit outside pixel scale, and the two pairs the chain packs
    for early, late, offsets in (bc.fit_launch()[1:], bc.chain_model(ops.track_subframe_grid(*bc.STAGING_GRID))[1][:3]):
        cases += [(early[a:b], late[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]
    with open(path, 'wb') as f:
        f.write(struct.pack('<ii', 0x54494648, len(cases)))
        for e, l in cases:
            with np.errstate(all='ignore'):
                H, info, diag = hm.fit_pair(e, l)
            f.write(struct.pack('<i', len(e)))
            for a, t in ((e, np.float64), (l, np.float64), (H, np.float64), (info, np.int32), (diag, np.float64)):
                f.write(np.ascontiguousarray(a, t).tobytes())
    print('wrote %d cases to %s' % (len(cases), path))


if __name__ == '__main__':
    main(sys.argv[1])
