"""Cases for tools/hfit_body_check.cpp from tests/homography_model.py: every pair of the crafted launch of tests/hfit_cases.py, the 16,384-point
pair and the 180 planted cases, each with the model's H, info and diag.
    python tools/hfit_dump_cases.py cases.bin"""
import os
import struct
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import hfit_cases as hc  # noqa: E402
import homography_model as hm  # noqa: E402


def main(path):
    cases = []
    _, early, late, offsets = hc.crafted()
    cases += [(early[a:b], late[a:b]) for a, b in zip(offsets[:-1], offsets[1:])]
    early, late, _ = hc.largest()
    cases.append((early, late))
    cases += [(e, l) for _, _, e, l in hc.planted_cases()]
    with open(path, 'wb') as f:
        f.write(struct.pack('<ii', 0x54494648, len(cases)))
        for e, l in cases:
            H, info, diag = hm.fit_pair(e, l)
            f.write(struct.pack('<i', len(e)))
            for a, t in ((e, np.float64), (l, np.float64), (H, np.float64), (info, np.int32), (diag, np.float64)):
                f.write(np.ascontiguousarray(a, t).tobytes())
    print('wrote %d cases to %s' % (len(cases), path))


if __name__ == '__main__':
    main(sys.argv[1])
