"""The specification of the device feature scores (csrc/scores_body.h, csrc/scores.hip; `ops.feature_scores`): the lines of mfs.py:1196-1212
after the homography -- the cropping ratio and the distortion score of a clip from its per-frame (unstabilized -> cropped) homographies --
written so that a kernel can equal it bit for bit.  Only float64 + - * /, sqrt (correctly rounded), comparisons, the correctly rounded
conversion to float32 and integers, every expression parenthesised as the kernel evaluates it, no fused operation.  It is NOT
np.linalg.eigvals (LAPACK's iteration, which no kernel equals bit for bit): the two eigenvalues of the 2 x 2 block come in closed form.

One pair with H = homographies[p] (`pair_scores`):
  a, b, c, d   H00, H01, H10, H11
  ratio32      float32(1.0 / (a d)) -- IEEE like numpy at mfs.py:1203: a zero product gives an infinity, nothing is refused
  m, q         (a + d) 0.5, (a - d) 0.5
  disc, det    q q + b c, a d - b c
  real pair    disc >= 0: r = sqrt(disc); big = m + r where m >= 0, m - r below (no cancellation); small = det / big where big != 0,
               0.0 otherwise; u, v = |big|, |small|
  complex pair otherwise (a NaN disc comes here too): u = v = sqrt(det), the modulus of both
  order        the affine part [[a, b, tx], [c, d, ty], [0, 0, 1]] has the eigenvalue 1 and the two of its block: (x, y, z) = (u, v, 1.0),
               then three compare-and-swaps: x, y if x > y; y, z if y > z; x, y if x > y.  A NaN goes wherever these comparisons send it.
  distortion32 float32(y / z): the second largest magnitude over the largest (mfs.py:1208-1209)
  NaN          every float32 NaN this specification yields is THE quiet NaN 0x7FC00000: a NaN's sign and payload are the processor's
               (sqrt(-1) is negative on x86 and positive on the device), so `to_f32` replaces them.
Which pairs are scored: all of them without a fit record; with info (P, 4) int32 as `ops.fit_homographies` returns it, the pairs whose
status info[p][0] is OK (0).  A pair that is not scored gets (NaN, NaN) in the per-pair output and counts nowhere.
The clip:
  count        the number of scored pairs
  sum          the float64 sum of the scored ratio32 in the fit's order (profiles/homography_fit.md): partial j of 256 adds the pairs j,
               j + 256, ... in that order from +0.0 (a pair that is not scored adds nothing); partials 64 w .. 64 w + 63 fold in a halving
               tree (step = 32 .. 1: v[j] = v[j] + v[j + step]); total (w0 + w1) + (w2 + w3).  No atomics.
  cropping     float32(sum / count) (mfs.py:1212's np.mean, in float64)
  distortion   the smallest scored distortion32 (mfs.py:1212 takes np.min although its docstring says "greatest"; the code's choice is
               kept, as frontend_cv2 keeps it), NaN where any scored one is NaN.  "Smallest" in the same order: partial j starts at +inf and
               takes a pair's value where value < partial; the tree and the total take v[j + step] where v[j + step] < v[j] (only the sign of a
               zero can depend on that order).
  count == 0   two NaNs.
  record       int32[2]: {count, the first pair that was not scored or -1}.
Result: (scores (2,) float32 {cropping_ratio, distortion_score}, per_pair (P, 2) float32 {ratio32, distortion32}, record (2,) int32)."""
import math

import numpy as np

OK = 0
LANES, WAVE = 256, 64
MAX_PAIRS = 1 << 20
F = np.float64
NAN32 = np.array([0x7FC00000], np.uint32).view(np.float32)[0]


def to_f32(value):
    """The correctly rounded float32 of a float64; a NaN becomes the quiet NaN 0x7FC00000."""
    with np.errstate(all='ignore'):
        out = np.float32(value)
    return NAN32 if out != out else out


def div(x, y):
    """x / y as IEEE defines it (Python raises where numpy and the device do not)."""
    with np.errstate(all='ignore'):
        return float(F(x) / F(y))


def root(x):
    with np.errstate(all='ignore'):
        return float(np.sqrt(F(x)))


def pair_scores(H):
    """H (3, 3) float64 -> (ratio32, distortion32) as np.float32."""
    H = np.asarray(H, F).reshape(3, 3)
    a, b, c, d = float(H[0, 0]), float(H[0, 1]), float(H[1, 0]), float(H[1, 1])
    ratio = to_f32(div(1.0, a * d))
    m = (a + d) * 0.5
    q = (a - d) * 0.5
    disc = q * q + b * c
    det = a * d - b * c
    if disc >= 0.0:
        r = root(disc)
        big = m + r if m >= 0.0 else m - r
        small = div(det, big) if big != 0.0 else 0.0
        u, v = abs(big), abs(small)
    else:
        u = v = root(det)
    x, y, z = u, v, 1.0
    if x > y:
        x, y = y, x
    if y > z:
        y, z = z, y
    if x > y:
        x, y = y, x
    return ratio, to_f32(div(y, z))


def ordered_sum(terms):
    """terms (P,) float64 -> their sum in the specification's order."""
    terms = np.asarray(terms, F)
    trips = -(-len(terms) // LANES)
    padded = np.zeros(trips * LANES, F)                         # (a partial is never -0.0, so adding +0.0 changes nothing)
    padded[:len(terms)] = terms
    with np.errstate(all='ignore'):
        acc = np.zeros(LANES, F)
        for t in range(trips):
            acc = acc + padded[t * LANES:(t + 1) * LANES]
        w = acc.reshape(LANES // WAVE, WAVE).copy()
        step = WAVE // 2
        while step:
            w[:, :step] = w[:, :step] + w[:, step:2 * step]
            step //= 2
        return float((w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0]))


def ordered_min(values, scored):
    """The smallest scored float32 in the specification's order (NaNs never win a comparison: the caller looks for them)."""
    part = np.full(LANES, np.inf, np.float32)
    for p in np.nonzero(scored)[0]:
        if values[p] < part[p % LANES]:
            part[p % LANES] = values[p]
    w = part.reshape(LANES // WAVE, WAVE).copy()
    step = WAVE // 2
    while step:
        for j in range(step):
            take = w[:, j + step] < w[:, j]
            w[take, j] = w[take, j + step]
        step //= 2
    lo = w[1, 0] if w[1, 0] < w[0, 0] else w[0, 0]
    hi = w[3, 0] if w[3, 0] < w[2, 0] else w[2, 0]
    return hi if hi < lo else lo


def feature_scores(homographies, info=None):
    """`ops.feature_scores` on NumPy arrays: (scores (2,) float32, per_pair (P, 2) float32, record (2,) int32)."""
    homographies = np.asarray(homographies, F).reshape(-1, 3, 3)
    P = len(homographies)
    scored = np.ones(P, bool) if info is None else np.asarray(info, np.int32).reshape(P, 4)[:, 0] == OK
    per_pair = np.full((P, 2), NAN32, np.float32)
    for p in np.nonzero(scored)[0]:
        per_pair[p] = pair_scores(homographies[p])
    count = int(scored.sum())
    missing = np.nonzero(~scored)[0]
    record = np.array([count, int(missing[0]) if len(missing) else -1], np.int32)
    total = ordered_sum(np.where(scored, per_pair[:, 0].astype(F), 0.0))
    cropping = to_f32(div(total, float(count)))
    if count == 0 or np.isnan(per_pair[scored, 1]).any():
        distortion = NAN32
    else:
        distortion = ordered_min(per_pair[:, 1], scored)
    return np.array([cropping, distortion], np.float32), per_pair, record


def first_unscored(record):
    """`ops.feature_scores_check` on a NumPy array."""
    return None if int(record[1]) < 0 else int(record[1])
