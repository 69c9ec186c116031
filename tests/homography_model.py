"""The specification of the device homography fit (csrc/hfit_body.h, csrc/track_fit.hip; `ops.fit_homographies`): one normalised DLT per pair
over the packed survivors, written so that a kernel can equal it bit for bit.  Only float64 + - * /, sqrt (correctly rounded), comparisons and
integers, every expression parenthesised as the kernel evaluates it, no fused operation, and EVERY SUM OVER POINTS IN ONE STATED ORDER.

Input: early, late (K_total, 2) float64 and offsets (P + 1,) int32 as `ops.gather_inliers` leaves them; pair p owns points offsets[p] ..
offsets[p + 1] - 1.  A range that is not 0 <= offsets[p] <= offsets[p + 1] <= K_total is read as empty (K = 0).

The sum over a pair's K points (`ordered_sum`) -- the order is the same for every launch shape and uses no atomics:
  partials     256 of them; partial j adds the terms of points j, j + 256, j + 512, ... in that order, starting from +0.0;
  waves        partials 64 w .. 64 w + 63 (w = 0 .. 3) fold in a halving tree: for step = 32, 16, 8, 4, 2, 1: v[j] = v[j] + v[j + step], j < step;
  total        (w0 + w1) + (w2 + w3).
One pair with K points (`fit_pair`):
  refusal      K < 4: TOO_FEW.
  centroid     c = (sum x / K, sum y / K) for both clouds (4 ordered sums; K converted exactly).
  moments      dx = x - cx, dy = y - cy per point; the ordered sums of d = sqrt(dx dx + dy dy), dx dx, dx dy and dy dy, for both clouds (8).
  refusal      a cloud is on one line (or one point) where the smaller eigenvalue of its centred second moments [[a, b], [b, c]] is at most
               1e-18 max(larger, 1) -- `host._collinear`'s test on squared singular values -- in closed form and without a division:
               half = (a + c) 0.5, diff = (a - c) 0.5, big = half + sqrt(diff diff + b b), det = a c - b b; COLLINEAR unless
               det > (1e-18 max(big, 1)) big.  A NaN fails the comparison, so non-finite input ends here.  Early cloud or late cloud.
  similarity   `host._normalisation`: s = sqrt(2) / (sum d / K) with sqrt(2) = 1.4142135623730951, t = -(s c); a point becomes (x s + tx, y s + ty).
  normal sums  per point, in normalised coordinates (x, y) early and (u, v) late, with xx = x x, xy = x y, yy = y y, w = u u + v v: the 23
               ordered sums of q = (xx, xy, yy, x, y), u q, u, v q, v, w q, w -- a product of three factors is the late factor times the
               early product, e.g. u (x y).  The 24th, the sum of 1, is K.
  N            the 9 x 9 normal matrix A^T A of the DLT rows (p, 0, -u p), (0, p, -v p), p = (x, y, 1), without ever forming A:
               N[0:3, 0:3] = N[3:6, 3:6] = S(p p^T), N[0:3, 6:9] = -S(u p p^T), N[3:6, 6:9] = -S(v p p^T), N[6:9, 6:9] = S(w p p^T),
               N[0:3, 3:6] = 0, symmetric.
  eigenvector  cyclic Jacobi on N with V = 1: sweeps over (p, q), p < q, row-major.  A rotation is skipped where
               |a_pq| <= 2^-53 sqrt(|a_pp a_qq|).  Otherwise theta = (a_qq - a_pp) / (2 a_pq), t = sign / (|theta| + sqrt(theta theta + 1))
               with sign = 1 for theta >= 0 and -1 below, c = 1 / sqrt(t t + 1), s = t c; for k != p, q: a_kp' = c a_kp - s a_kq, a_kq' =
               s a_kp + c a_kq (mirrored into rows p and q); a_pp' = a_pp - t a_pq, a_qq' = a_qq + t a_pq, a_pq' = 0; for every k:
               v_kp' = c v_kp - s v_kq, v_kq' = s v_kp + c v_kq.  The loop ends after the first sweep without a rotation (that sweep counts)
               or after 30 sweeps: NOT_CONVERGED, never expected.  h = the column of V at the first index of the smallest diagonal entry.
  back         G = h T_early: g_i0 = h_i0 s_e, g_i1 = h_i1 s_e, g_i2 = (h_i0 tx_e + h_i1 ty_e) + h_i2; H = inv(T_late) G: H_0j = g_0j / s_l +
               cx_l g_2j, H_1j = g_1j / s_l + cy_l g_2j, H_2j = g_2j.
  refusal      m = the largest |H_ij| (a NaN never counts); AT_INFINITY unless |H_22| > 1e-12 m.  Otherwise every entry is divided by H_22.
  result       H (3, 3); info (status, K, sweeps run, index of the chosen eigenvalue); diag (s_early, s_late, cx_e, cy_e, cx_l, cy_l, smallest
               eigenvalue, second smallest): a mismatch names its stage.  A pair that is not OK gets the identity and zeros in diag where the
               value is undefined (TOO_FEW: all of it; COLLINEAR: all but the centroids).

Where this deviates from `host.lsq_homography` -- beyond what host.py already lists against cv2.findHomography (no Levenberg-Marquardt
refinement) -- :
  * the null vector comes from Jacobi rotations on the 9 x 9 normal matrix instead of LAPACK's SVD of the 2K x 9 matrix.  Both minimise the
    same algebraic error in the same normalised coordinates, and forming N squares the condition number, which float64 carries after the
    normalisation: the two agree to rounding (profiles/homography_fit.md has the measured distance, tests/test_homography_model.py asserts it);
  * the sums have the order above, NumPy's have pairwise order;
  * the collinearity test works on second moments (noise floor 1e-16 of the larger eigenvalue) where the host has the singular values of the
    centred points (noise floor 1e-16 of the larger singular VALUE): a cloud that is on a line only up to rounding can pass here and is
    refused there.  Clouds whose centred coordinates are exact -- integer coordinates with an integer centroid -- are refused by both;
  * a refused pair yields the identity and a status instead of a ValueError."""
import math

import numpy as np

OK, TOO_FEW, COLLINEAR, AT_INFINITY, NOT_CONVERGED = 0, 1, 2, 3, 4
LANES, WAVE, MAX_SWEEPS = 256, 64, 30
SQRT2 = 1.4142135623730951
EPS = 2.0 ** -53
F = np.float64


def ordered_sum(terms):
    """terms (K, Q) float64 -> the Q sums in the specification's order, as Python floats."""
    terms = np.asarray(terms, F)
    K, Q = terms.shape
    trips = -(-K // LANES)
    padded = np.zeros((trips * LANES, Q), F)                      # (a partial is never -0.0, so adding +0.0 changes nothing)
    padded[:K] = terms
    acc = np.zeros((LANES, Q), F)
    for m in range(trips):
        acc = acc + padded[m * LANES:(m + 1) * LANES]
    w = acc.reshape(LANES // WAVE, WAVE, Q).copy()
    step = WAVE // 2
    while step:
        w[:, :step] = w[:, :step] + w[:, step:2 * step]
        step //= 2
    return ((w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])).tolist()


def collinear(a, b, c):
    half, diff = (a + c) * 0.5, (a - c) * 0.5
    big = half + math.sqrt(diff * diff + b * b)
    det = a * c - b * b
    return not det > (1e-18 * (big if big > 1.0 else 1.0)) * big


def normal_matrix(sums, K):
    """The 9 x 9 N (list of rows) from the 23 ordered sums and K."""
    A = [sums[0], sums[1], sums[3], sums[1], sums[2], sums[4], sums[3], sums[4], float(K)]           # S(p p^T), row-major 3 x 3
    B, C, D = ([s[0], s[1], s[3], s[1], s[2], s[4], s[3], s[4], s[5]] for s in (sums[5:11], sums[11:17], sums[17:23]))
    N = [[0.0] * 9 for _ in range(9)]
    for i in range(3):
        for j in range(3):
            N[i][j] = N[3 + i][3 + j] = A[3 * i + j]
            N[i][6 + j] = N[6 + j][i] = -B[3 * i + j]
            N[3 + i][6 + j] = N[6 + j][3 + i] = -C[3 * i + j]
            N[6 + i][6 + j] = D[3 * i + j]
    return N


def jacobi(N):
    """Cyclic Jacobi on the 9 x 9 N (changed in place): (V, sweeps run, converged)."""
    V = [[1.0 if i == j else 0.0 for j in range(9)] for i in range(9)]
    for sweep in range(1, MAX_SWEEPS + 1):
        rotated = False
        for p in range(8):
            for q in range(p + 1, 9):
                app, aqq, apq = N[p][p], N[q][q], N[p][q]
                if abs(apq) <= EPS * math.sqrt(abs(app * aqq)):
                    continue
                rotated = True
                theta = (aqq - app) / (2.0 * apq)
                t = (1.0 if theta >= 0 else -1.0) / (abs(theta) + math.sqrt(theta * theta + 1.0))
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for k in range(9):
                    if k != p and k != q:
                        akp, akq = N[k][p], N[k][q]
                        N[k][p] = N[p][k] = c * akp - s * akq
                        N[k][q] = N[q][k] = s * akp + c * akq
                    vkp, vkq = V[k][p], V[k][q]
                    V[k][p] = c * vkp - s * vkq
                    V[k][q] = s * vkp + c * vkq
                N[p][p], N[q][q] = app - t * apq, aqq + t * apq
                N[p][q] = N[q][p] = 0.0
        if not rotated:
            return V, sweep, True
    return V, MAX_SWEEPS, False


def fit_pair(early, late):
    """early, late (K, 2) float64 -> (H (3, 3) float64, info (4,) int32, diag (8,) float64)."""
    early, late = np.asarray(early, F).reshape(-1, 2), np.asarray(late, F).reshape(-1, 2)
    K = len(early)
    H, info, diag = np.identity(3), np.array([OK, K, 0, 0], np.int32), np.zeros(8)
    if K < 4:
        info[0] = TOO_FEW
        return H, info, diag
    with np.errstate(all='ignore'):
        kf = float(K)
        cex, cey, clx, cly = (v / kf for v in ordered_sum(np.concatenate([early, late], axis=1)))
        diag[2:6] = cex, cey, clx, cly
        dex, dey, dlx, dly = early[:, 0] - F(cex), early[:, 1] - F(cey), late[:, 0] - F(clx), late[:, 1] - F(cly)
        de, ea, eb, ec, dl, la, lb, lc = ordered_sum(np.stack([np.sqrt(dex * dex + dey * dey), dex * dex, dex * dey, dey * dey,
                                                               np.sqrt(dlx * dlx + dly * dly), dlx * dlx, dlx * dly, dly * dly], axis=1))
        if collinear(ea, eb, ec) or collinear(la, lb, lc):
            info[0] = COLLINEAR
            return H, info, diag
        se, sl = SQRT2 / (de / kf), SQRT2 / (dl / kf)
        tex, tey, tlx, tly = -(se * cex), -(se * cey), -(sl * clx), -(sl * cly)
        diag[0:2] = se, sl
        x, y = early[:, 0] * F(se) + F(tex), early[:, 1] * F(se) + F(tey)
        u, v = late[:, 0] * F(sl) + F(tlx), late[:, 1] * F(sl) + F(tly)
        q = [x * x, x * y, y * y, x, y]
        w = u * u + v * v
        sums = ordered_sum(np.stack(q + [u * t for t in q] + [u] + [v * t for t in q] + [v] + [w * t for t in q] + [w], axis=1))
    N = normal_matrix(sums, K)
    V, sweeps, converged = jacobi(N)
    info[2] = sweeps
    eig = [N[i][i] for i in range(9)]
    index = 0
    for i in range(1, 9):
        if eig[i] < eig[index]:
            index = i
    second = None
    for i in range(9):
        if i != index and (second is None or eig[i] < second):
            second = eig[i]
    info[3] = index
    diag[6:8] = eig[index], second
    if not converged:
        info[0] = NOT_CONVERGED
        return H, info, diag
    h = [V[k][index] for k in range(9)]
    G = []
    for i in range(3):
        G += [h[3 * i] * se, h[3 * i + 1] * se, (h[3 * i] * tex + h[3 * i + 1] * tey) + h[3 * i + 2]]
    out = [G[j] / sl + clx * G[6 + j] for j in range(3)] + [G[3 + j] / sl + cly * G[6 + j] for j in range(3)] + G[6:9]
    m = 0.0
    for value in out:
        if abs(value) > m:
            m = abs(value)
    if not abs(out[8]) > 1e-12 * m:
        info[0] = AT_INFINITY
        return H, info, diag
    return np.array([value / out[8] for value in out], F).reshape(3, 3), info, diag


def pair_range(offsets, p, total):
    lo, hi = int(offsets[p]), int(offsets[p + 1])
    return (lo, hi) if 0 <= lo <= hi <= total else (0, 0)


def fit_homographies(early, late, offsets):
    """`ops.fit_homographies` on NumPy arrays: (H (P, 3, 3) float64, info (P, 4) int32, diag (P, 8) float64)."""
    early, late = np.asarray(early, F).reshape(-1, 2), np.asarray(late, F).reshape(-1, 2)
    offsets = np.asarray(offsets, np.int32)
    P = len(offsets) - 1
    H, info, diag = np.zeros((P, 3, 3)), np.zeros((P, 4), np.int32), np.zeros((P, 8))
    for p in range(P):
        lo, hi = pair_range(offsets, p, len(early))
        H[p], info[p], diag[p] = fit_pair(early[lo:hi], late[lo:hi])
    return H, info, diag


def first_refused(info):
    """`ops.fit_check` on a NumPy array."""
    bad = np.nonzero(np.asarray(info)[:, 0] != OK)[0]
    return int(bad[0]) if len(bad) else None
