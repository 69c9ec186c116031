"""Cases for tools/track_body_check.cpp from tests/track_model.py: image pairs of every pyramid depth and of the smallest sizes, with points
inside, on the edges and outside, the model's corners of the early image and its LK result.   python tools/track_dump_cases.py cases.bin"""
import os
import struct
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, 'tests'))
import track_model as tm  # noqa: E402
from meshflow_amd import synthetic  # noqa: E402


def canvas(h, w, seed):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    v = 128 + 30 * np.sin(x * 0.31 + 0.2) * np.cos(y * 0.23) + 25 * np.sin(x * 0.13 + y * 0.19 + 1) + 20 * np.cos(x * 0.07 - y * 0.11)
    for bx, by, bw, bh, val in synthetic.hash32(np.arange(300), seed).reshape(60, 5):
        x0, y0 = int(bx % w), int(by % h)
        v[y0:y0 + 5 + int(bh % 9), x0:x0 + 5 + int(bw % 9)] += int(val % 120) - 60
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def points(w, h):
    ys, xs = np.mgrid[2:h:7, 3:w:9]
    pts = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float32).tolist()
    pts += [[0, 0], [w - 1, h - 1], [w - 0.5, h / 2 + 0.25], [w / 2 + 0.5, 0], [-12.5, 5], [w + 10, 5], [5, -11.25], [5, h + 10.5], [1e7, 3], [3, -1e7]]
    return np.array(pts, np.float32)


def main(path):
    cases = []
    big = canvas(220, 260, 3)
    for (w, h), (dx, dy) in (((200, 180), (5, -3)), ((100, 90), (-2, 2)), ((67, 45), (1, 1)), ((48, 40), (14, 0)), ((31, 19), (0, 2)), ((7, 7), (1, 0)),
                             ((2, 9), (0, 1)), ((9, 1), (1, 0))):
        early = np.ascontiguousarray(big[20:20 + h, 20:20 + w])
        late = np.ascontiguousarray(big[20 - dy:20 - dy + h, 20 - dx:20 - dx + w])
        cases.append((early, late))
    noise = (synthetic.hash32(np.arange(64 * 48), 9) & 255).astype(np.uint8).reshape(48, 64)
    cases.append((noise, np.roll(noise, 2, axis=1)))
    flat = np.full((40, 50), 128, np.uint8)
    cases.append((cases[3][0][:40, :48].copy(), flat[:, :48].copy()))
    cases.append((flat, flat))
    with open(path, 'wb') as f:
        f.write(struct.pack('<ii', 0x4b545246, len(cases)))
        for early, late in cases:
            h, w = early.shape
            pts = points(w, h)
            corners = tm.fast_corners(early)
            moved, found = tm.lk_track(early, late, pts)
            f.write(struct.pack('<iiii', w, h, len(pts), len(corners)))
            for a in (early, late, pts, corners, moved, found):
                f.write(np.ascontiguousarray(a).tobytes())
    print('wrote %d cases to %s' % (len(cases), path))


if __name__ == '__main__':
    main(sys.argv[1])
