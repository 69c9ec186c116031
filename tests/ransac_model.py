"""The specification of the device outlier step (csrc/ransac_body.h, csrc/track_ransac.hip; `ops.ransac_inliers`, `ops.gather_inliers`): RANSAC
per sub-frame and the gather of the survivors, written so that a kernel can equal it bit for bit.  Only float64 + - * /, comparisons and
integer arithmetic, every expression parenthesised as the kernel evaluates it; no LAPACK, no libm, no reduction of floats whose order a
parallel kernel would have to imitate (the only sums over candidates are integer counts).

One sub-frame of one pair (`ransac_subframe`):
  candidates   K = min(count, max); the points i < K with found[i] != 0, in index order, widened to float64; k of them.  K < min_features,
               k < min_features or k < 4: status TOO_FEW, no inliers, no iteration.
  iterations   it = 0, 1, ... while it < iterations, starting at iterations = max_iters; skipped iterations count.
  sample       hash32(16 it + j, seed) % k for j = 0 .. 15 (`synthetic.hash32`); the first four distinct values, in draw order; fewer than
               four distinct values: the iteration is skipped.  Stateless: no unbounded loop anywhere.
  degenerate   `host._degenerate_sample` on the early and on the late sample points, its right-hand sum as (|d1x| + |d1y|) + (|d2x| + |d2y|);
               a degenerate sample skips the iteration.
  fit          H = S2Q(late) adj(S2Q(early)) in float64: S2Q is Heckbert's unit-square -> quad map of the four sample points in draw order
               (the construction of csrc/cell_table.hip), adj the 3 x 3 adjugate, every entry of the product a left-to-right sum of three
               products.  No scaling to h22 = 1, no Hartley similarity.  An entry that is not finite skips the iteration.
  error test   X = (h00 x + h01 y) + h02, likewise Y and w; rx = X - lx w, ry = Y - ly w; inlier iff w w > 0 and
               rx rx + ry ry <= (threshold threshold)(w w).  Invariant to the sign and scale of H; a NaN is never an inlier.
  best         c > max(best_count, 3): keep H (the first best wins ties), then iterations = min(iterations, N(c, k)).
  N(c, k)      w = c / k, q = 1 - (w w)(w w), p1 = 1.0 - confidence; P[0] = q, P[j + 1] = P[j] P[j] (16 squarings); n = 0, r = 1; for
               j = 16 .. 0: t = r P[j]; t > p1: r = t, n += 2^j.  n + 1 is cv2's "enough samples that one is free of outliers with
               probability `confidence`" by greedy binary descent, without log or pow.  N = min(3 n + 1, max_iters): a sample free of
               outliers is necessary for a good hypothesis, not sufficient -- four noisy points fix H well only where they lie far apart
               -- and the consensus set is never refitted, so the search goes on for three times as long (1 at c = k all the same).
               The factor 3 is empirical, not derived: on the planted recipe of tests/test_ransac_model.py (5 x 300 cases) N = n + 1
               lost up to 18 % of the inliers of single cases, twice that count up to 7 %, 3 n + 1 up to 4 %, four times the count up to 2 %.
  result       the consensus set of the best hypothesis as a mask over the `max` slots (0 for non-candidates) and the record
               (status, k, inliers, iterations run): OK, TOO_FEW, or NO_CONSENSUS where best_count < 4 (no inliers then).  "Iterations run"
               is the value of `it` when the loop ends.

Where this deviates from cv2.findHomography(..., cv2.RANSAC) -- beyond what `host.py` already lists for its finisher (hash counters instead of
OpenCV's generator, no Levenberg-Marquardt refinement, the best sample's consensus set as the mask) -- and from `host.ransac_inliers`:
  * the 4-point fit is the closed form above, not a normalised DLT through an SVD: the two agree to rounding on a sample in general
    position, so a candidate within rounding of the threshold can fall on the other side;
  * the error test is the reprojection test multiplied through by w^2 instead of divided; a point mapped to infinity (w = 0) is an outlier
    in both;
  * the iteration count comes from the descent above: n + 1 is equal to or one more than `host._ransac_iterations` where both are below
    max_iters, and N is three times n, plus one -- 1 where the host's formula gives 0 (c = k);
  * sampling restarts its 16 draws in every iteration instead of consuming one stream of counters, and gives an iteration up after 16 draws:
    `host.ransac_inliers` loops until it has four distinct indices, which does not end for k < 4;
  * there is no all-collinear pre-check (the host's SVD): such a set yields only degenerate samples and ends as NO_CONSENSUS after max_iters
    iterations; fewer than 4 candidates are TOO_FEW.  Either way the sub-frame is skipped, which is what `tracker.finish_pair` does with the
    host's ValueError.
`gather` restates the packing of `tracker.finish_pair` + `host.pack_features` (mfs.py:521, 578), and `finish_pair` is `tracker.finish_pair`
with `host.ransac_inliers` replaced by this model."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from meshflow_amd import host, synthetic  # noqa: E402

OK, TOO_FEW, NO_CONSENSUS = 0, 1, 2
PAIR_TOO_FEW = 1
DRAWS, SQUARINGS, OVERSAMPLE = 16, 16, 3
F = np.float64


def draw_sample(it, seed, k):
    """The four distinct candidate indices of iteration `it`, in draw order, or None."""
    draws = synthetic.hash32(np.arange(DRAWS * it, DRAWS * it + DRAWS), seed) % k
    sample = []
    for v in draws.tolist():
        if v not in sample:
            sample.append(v)
            if len(sample) == 4:
                return sample
    return None


def degenerate_sample(p):
    """host._degenerate_sample with its right-hand sum parenthesised: p (4, 2) float64."""
    for i, j, k in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        d1x, d1y, d2x, d2y = p[j][0] - p[i][0], p[j][1] - p[i][1], p[k][0] - p[i][0], p[k][1] - p[i][1]
        if abs(d1x * d2y - d1y * d2x) <= F(1.1920929e-07) * ((abs(d1x) + abs(d1y)) + (abs(d2x) + abs(d2y))):
            return True
    return False


def square_to_quad(p):
    """Unit square (0,0), (1,0), (1,1), (0,1) -> p[0], p[1], p[2], p[3]: row-major [a, b, c, d, e, f, g, h, 1]."""
    sx = ((p[0][0] - p[1][0]) + p[2][0]) - p[3][0]
    sy = ((p[0][1] - p[1][1]) + p[2][1]) - p[3][1]
    dx1, dx2 = p[1][0] - p[2][0], p[3][0] - p[2][0]
    dy1, dy2 = p[1][1] - p[2][1], p[3][1] - p[2][1]
    den = dx1 * dy2 - dx2 * dy1
    g = (sx * dy2 - dx2 * sy) / den
    h = (dx1 * sy - sx * dy1) / den
    return [(p[1][0] - p[0][0]) + g * p[1][0], (p[3][0] - p[0][0]) + h * p[3][0], p[0][0],
            (p[1][1] - p[0][1]) + g * p[1][1], (p[3][1] - p[0][1]) + h * p[3][1], p[0][1], g, h, F(1.0)]


def adjugate(S):
    a, b, c, d, e, f, g, h = S[:8]                                # (the last entry is 1)
    return [e - f * h, c * h - b, b * f - c * e, f * g - d, a - c * g, c * d - a * f, d * h - e * g, b * g - a * h, a * e - b * d]


def fit4(early, late):
    """H (9 float64) of four correspondences, or None where an entry is not finite."""
    Sl, A = square_to_quad(late), adjugate(square_to_quad(early))
    H = []
    for i in range(3):
        for j in range(3):
            s = Sl[3 * i] * A[j]
            s = s + Sl[3 * i + 1] * A[3 + j]
            s = s + Sl[3 * i + 2] * A[6 + j]
            H.append(s)
    return H if all(np.isfinite(v) for v in H) else None


def inliers_of(H, early, late, threshold):
    """The error test over (k, 2) float64 arrays: a boolean mask."""
    x, y, lx, ly = early[:, 0], early[:, 1], late[:, 0], late[:, 1]
    X = (H[0] * x + H[1] * y) + H[2]
    Y = (H[3] * x + H[4] * y) + H[5]
    w = (H[6] * x + H[7] * y) + H[8]
    rx, ry = X - lx * w, Y - ly * w
    ww = w * w
    return (ww > 0) & (rx * rx + ry * ry <= (F(threshold) * F(threshold)) * ww)


def iterations_needed(c, k, confidence, max_iters):
    w = F(c) / F(k)
    q = F(1.0) - (w * w) * (w * w)
    p1 = F(1.0) - F(confidence)
    P = [q]
    for _ in range(SQUARINGS):
        P.append(P[-1] * P[-1])
    n, r = 0, F(1.0)
    for j in range(SQUARINGS, -1, -1):
        t = r * P[j]
        if t > p1:
            r, n = t, n + (1 << j)
    return min(OVERSAMPLE * n + 1, int(max_iters))


def ransac_subframe(points, moved, count, found, min_features=4, threshold=3.0, confidence=0.995, max_iters=2000, seed=0):
    """points, moved (max, 2) float32, found (max,) -> (mask (max,) uint8, (status, k, inliers, iterations run))."""
    points, moved, found = np.asarray(points, np.float32), np.asarray(moved, np.float32), np.asarray(found)
    size = points.shape[0]
    K = max(0, min(int(count), size))
    index = np.nonzero(found[:K] != 0)[0]
    k = len(index)
    mask = np.zeros(size, np.uint8)
    if K < min_features or k < min_features or k < 4:
        return mask, (TOO_FEW, k, 0, 0)
    early, late = points[index].astype(F), moved[index].astype(F)
    best, best_count = None, 0
    iterations, it = int(max_iters), 0
    with np.errstate(all='ignore'):
        while it < iterations:
            sample = draw_sample(it, seed, k)
            it += 1
            if sample is None:
                continue
            e, l = early[sample], late[sample]
            if degenerate_sample(e) or degenerate_sample(l):
                continue
            H = fit4(e, l)
            if H is None:
                continue
            inl = inliers_of(H, early, late, threshold)
            c = int(inl.sum())
            if c > max(best_count, 3):
                best, best_count = inl, c
                iterations = min(iterations, iterations_needed(c, k, confidence, max_iters))
    if best_count < 4:
        return mask, (NO_CONSENSUS, k, 0, it)
    mask[index[best]] = 1
    return mask, (OK, k, best_count, it)


def ransac_inliers(points, counts, moved, found, min_features=4, threshold=3.0, confidence=0.995, max_iters=2000, seed=0):
    """`ops.ransac_inliers` on NumPy arrays: points, moved (n, S, max, 2), counts (n, S), found (n, S, max) -> (inlier (n, S, max) uint8,
    info (n, S, 4) int32)."""
    n, S, size = points.shape[:3]
    inlier, info = np.zeros((n, S, size), np.uint8), np.zeros((n, S, 4), np.int32)
    for p in range(n):
        for s in range(S):
            inlier[p, s], info[p, s] = ransac_subframe(points[p, s], moved[p, s], counts[p, s], found[p, s], min_features, threshold, confidence,
                                                       max_iters, seed)
    return inlier, info


def gather(points, moved, inlier, info, grid, min_features):
    """`ops.gather_inliers` on NumPy arrays, `grid` = ops.track_subframe_grid(...): (early (total, 2) float64, late, offsets (n + 1,) int32,
    pair_status (n,) int32).  Sub-frame order outer, point order inner; a pair below min_features survivors is empty and flagged."""
    sub_w, sub_h, _, rows = grid
    n, S = points.shape[:2]
    early, late, offsets, status = [np.zeros((0, 2))], [np.zeros((0, 2))], [0], np.zeros(n, np.int32)
    for p in range(n):
        e_parts, l_parts = [], []
        for s in range(S):
            if info[p, s, 0] != OK:
                continue
            keep = inlier[p, s] != 0
            offset = np.array([(s // rows) * sub_w, (s % rows) * sub_h], F)
            e_parts.append(points[p, s][keep].astype(F) + offset)
            l_parts.append(moved[p, s][keep].astype(F) + offset)
        total = sum(len(e) for e in e_parts)
        if total < min_features:
            status[p] = PAIR_TOO_FEW
            total = 0
        else:
            early += e_parts
            late += l_parts
        offsets.append(offsets[-1] + total)
    return np.concatenate(early), np.concatenate(late), np.array(offsets, np.int32), status


def finish_pair(grid, points, counts, moved, found, min_features, **ransac):
    """`tracker.finish_pair` with `host.ransac_inliers` replaced by the model: (early, late, homography) or (None, None, None)."""
    sub_w, sub_h, _, rows = grid
    early_parts, late_parts = [], []
    for s in range(points.shape[0]):
        mask, (status, _, _, _) = ransac_subframe(points[s], moved[s], counts[s], found[s], min_features, **ransac)
        if status != OK:
            continue
        keep = mask.astype(bool)
        offset = [(s // rows) * sub_w, (s % rows) * sub_h]
        early_parts.append(points[s][keep][:, np.newaxis, :] + offset)
        late_parts.append(moved[s][keep][:, np.newaxis, :] + offset)
    if not early_parts:
        return None, None, None
    early, late = np.concatenate(early_parts), np.concatenate(late_parts)
    if len(early) < min_features:                                        # mfs.py:521
        return None, None, None
    try:
        homography = host.lsq_homography(early, late)
    except ValueError:
        return None, None, None
    return early, late, homography
