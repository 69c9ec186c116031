"""Point sets for the homography fit's tests and for tools/hfit_dump_cases.py: the planted recipe (a homography near the identity, float32
sub-frame coordinates plus integer sub-frame offsets as `ops.gather_inliers` produces them) and the crafted launch whose pair sizes sit on
the edges of the 256-lane reduction.  Everything comes from `synthetic.hash32`: the same on every platform."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meshflow_amd import synthetic  # noqa: E402

SIZES = (4, 5, 8, 30, 200, 500)
NOISES = (0.0, 0.3, 1.0)
SEEDS_PER_CELL = 5
FRAME, FRAME_4K = (1920, 1080), (3840, 2160)


def _uniform(n, seed, lo, hi):
    return lo + (hi - lo) * synthetic.uniform01(np.arange(n), seed)


def as_gathered(points, anchor, sub=(480, 270)):
    """float64 points -> float32 coordinate relative to the sub-frame of `anchor` (the early point) + that sub-frame's integer offset: exactly
    what the gather writes."""
    offset = np.floor(anchor / np.array(sub)) * np.array(sub)
    return (points - offset).astype(np.float32).astype(np.float64) + offset


def planted(k, noise, seed, frame=FRAME, box=None):
    """k correspondences under a homography within 2 % of the identity (translations up to 8 px, perspective terms up to 1e-5): early points
    hashed over the frame -- or over `box` = (left, top, width, height) --, uniform noise of +-`noise` px on the late ones.  Returns
    (early (k, 2) float64, late (k, 2) float64, H)."""
    seed = int(seed) * 16 + 500000
    r = _uniform(8, seed, -1.0, 1.0)
    H = np.array([[1 + 0.02 * r[0], 0.02 * r[1], 8 * r[2]], [0.02 * r[3], 1 + 0.02 * r[4], 8 * r[5]], [1e-5 * r[6], 1e-5 * r[7], 1.0]])
    left, top, width, height = box if box is not None else (0, 0) + tuple(frame)
    raw = np.stack([_uniform(k, seed + 1, left, left + width), _uniform(k, seed + 2, top, top + height)], 1)
    early = as_gathered(raw, raw)
    q = np.concatenate([early, np.ones((k, 1))], 1) @ H.T
    late = q[:, :2] / q[:, 2:] + np.stack([_uniform(k, seed + 3, -noise, noise), _uniform(k, seed + 4, -noise, noise)], 1)
    return early, as_gathered(late, raw), H


def planted_cases():
    """[(name, frame, early, late)]: every size x noise x 5 seeds over a 1080p frame, and the same again clustered in the bottom-right
    960 x 540 of a 4K frame -- one sub-frame of its 4 x 4 grid, the smallest region the tracker can be left with: 180 cases.  (The distance is
    taken at the FRAME's corners, so a cluster extrapolates: 4 points in 240 x 135 that both fits reproduce to 1e-12 px differ by 2e-5 px at the
    far corner, 16 widths away.  That measures the case, not the fit; profiles/homography_fit.md has the figures.)"""
    out, seed = [], 0
    for clustered in (False, True):
        for k in SIZES:
            for noise in NOISES:
                for _ in range(SEEDS_PER_CELL):
                    frame = FRAME_4K if clustered else FRAME
                    box = (2880, 1620, 960, 540) if clustered else None
                    e, l, _ = planted(k, noise, seed, frame, box)
                    out.append(('%s K=%d noise=%g seed=%d' % ('4K corner' if clustered else '1080p', k, noise, seed), frame, e, l))
                    seed += 1
    return out


def corner_distance(a, b, frame):
    """The largest distance in pixels between the images of the frame's four corners under the 3 x 3 matrices a and b."""
    w, h = frame
    corners = np.array([[0.0, 0.0, 1.0], [w - 1.0, 0.0, 1.0], [0.0, h - 1.0, 1.0], [w - 1.0, h - 1.0, 1.0]])
    pa, pb = corners @ np.asarray(a).T, corners @ np.asarray(b).T
    return float(np.sqrt((((pa[:, :2] / pa[:, 2:]) - (pb[:, :2] / pb[:, 2:])) ** 2).sum(axis=1)).max())


def collinear(k):
    """k points on a line, integer coordinates with an integer centroid for odd k: every centred coordinate is exact."""
    t = np.arange(k, dtype=np.float64)
    early = np.stack([10 + 3 * t, 20 + 2 * t], 1)
    return early, early + np.array([1.5, -2.0])


def identical(k):
    early = np.tile(np.array([[31.0, 47.0]]), (k, 1))
    return early, early + np.array([2.0, 1.0])


def origin_to_infinity():
    """12 exact correspondences of H = [[100, 0, 100], [0, 100, 50], [1, 1, 0]] -- x + y is a power of two, so every late coordinate is a
    binary fraction: the fitted matrix has h22 = 0 up to rounding."""
    early = np.array([[1, 1], [3, 1], [1, 3], [2, 6], [6, 2], [5, 11], [12, 4], [3, 13], [7, 1], [9, 23], [30, 2], [17, 15]], np.float64)
    den = early.sum(axis=1)
    assert all(int(d) & (int(d) - 1) == 0 for d in den)
    return early, np.stack([(100 * early[:, 0] + 100) / den, (100 * early[:, 1] + 50) / den], 1)


EXACT_EARLY = np.array([[10, 10], [200, 30], [180, 220], [25, 190]], np.float64)
EXACT_LATE = np.array([[12, 9], [203, 31], [181, 224], [26, 188]], np.float64)
CRAFTED_SIZES = (0, 3, 4, 5, 255, 256, 257, 513, 1000)


def crafted():
    """One launch: (names, early (K_total, 2) float64, late, offsets (P + 1,) int32).  Pair sizes 0, 3, 4, 5, 255, 256, 257, 513, 1,000 (the
    tails of the 256-lane stride, one and two trips); an empty pair between two full ones; a collinear cloud, a collinear late cloud alone,
    an identical-points cloud; 4 exact correspondences and 100 noise-free ones; a cloud at coordinates near 3,840; a pair whose h22 vanishes."""
    pairs = []
    for i, k in enumerate(CRAFTED_SIZES):
        e, l, _ = planted(max(k, 1), 0.3, 900 + i)
        pairs.append(('K=%d' % k, e[:k], l[:k]))
    e, l, _ = planted(40, 0.3, 920)
    pairs += [('before the empty pair', e, l), ('empty', e[:0], l[:0])]
    e, l, _ = planted(41, 1.0, 921)
    pairs.append(('after the empty pair', e, l))
    pairs.append(('collinear',) + collinear(31))
    pairs.append(('late collinear', planted(31, 0.0, 922)[0], collinear(31)[1]))
    pairs.append(('identical',) + identical(10))
    pairs.append(('exact 4', EXACT_EARLY, EXACT_LATE))
    e, _, H = planted(100, 0.0, 923)
    q = np.concatenate([e, np.ones((100, 1))], 1) @ H.T
    pairs.append(('noise-free 100', e, q[:, :2] / q[:, 2:]))
    e, l, _ = planted(300, 0.3, 924, FRAME_4K, (3600, 2025, 240, 135))
    pairs.append(('near 3,840', e, l))
    pairs.append(('h22 vanishes',) + origin_to_infinity())
    names = [p[0] for p in pairs]
    offsets = np.cumsum([0] + [len(p[1]) for p in pairs]).astype(np.int32)
    return names, np.ascontiguousarray(np.concatenate([p[1] for p in pairs])), np.ascontiguousarray(np.concatenate([p[2] for p in pairs])), offsets


def largest():
    """One pair of 16,384 points, cfg2's cap: (early, late, offsets)."""
    e, l, _ = planted(16384, 0.3, 930)
    return e, l, np.array([0, 16384], np.int32)
