"""Cases for tools/scores_body_check.cpp from tests/scores_model.py: launches of planted matrices at the lengths on the edges of the 256-lane
fold, with and without a fit record (refused pairs first, last, in the middle, all of them), and the matrices whose scores are infinities
or NaNs -- each with the model's scores, per-pair values and record.
    python tools/scores_dump_cases.py cases.bin"""
import os
import struct
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tests'))
import scores_cases as sc  # noqa: E402
import scores_model as sm  # noqa: E402


def main(path):
    cases = []
    for pairs in (1, 2, 63, 64, 65, 255, 256, 257, 513, 1000):
        h = sc.launch(pairs)
        cases.append((h, None))
        for refused in ([0], [pairs - 1], [pairs // 2], sorted({0, pairs // 3, pairs - 1}), list(range(pairs))):
            cases.append((h, sc.record(pairs, refused)))
    special = np.stack([h for _, h in sc.special()])
    cases.append((special, None))
    cases += [(special[i:i + 1], None) for i in range(len(special))]
    cases.append((np.concatenate([sc.launch(300), special]), sc.record(300 + len(special), [5, 299])))
    with open(path, 'wb') as f:
        f.write(struct.pack('<ii', 0x524F4353, len(cases)))
        for h, info in cases:
            scores, per_pair, record = sm.feature_scores(h, info)
            f.write(struct.pack('<ii', len(h), 0 if info is None else 1))
            f.write(np.ascontiguousarray(h, np.float64).tobytes())
            if info is not None:
                f.write(np.ascontiguousarray(info, np.int32).tobytes())
            for a, t in ((scores, np.float32), (per_pair, np.float32), (record, np.int32)):
                f.write(np.ascontiguousarray(a, t).tobytes())
    print('wrote %d cases to %s' % (len(cases), path))


if __name__ == '__main__':
    main(sys.argv[1])
