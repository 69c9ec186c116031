"""Host-side (NumPy, float64) pieces of the hot path that stay on the CPU because they are O(F) or
O(F*omega) scalar work: adaptive weights, Jacobi band coefficients, vertex grid, stability score.

`mfs.py:N` = /root/reference/meshflowstabilizer.py line N."""
import math

import numpy as np

ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL = 0
ADAPTIVE_WEIGHTS_DEFINITION_FLIPPED = 1
ADAPTIVE_WEIGHTS_DEFINITION_CONSTANT_HIGH = 2
ADAPTIVE_WEIGHTS_DEFINITION_CONSTANT_LOW = 3
ADAPTIVE_WEIGHTS_DEFINITION_CONSTANT_HIGH_VALUE = 100
ADAPTIVE_WEIGHTS_DEFINITION_CONSTANT_LOW_VALUE = 1

VALID_DEFINITIONS = (0, 1, 2, 3)


def adaptive_weights(num_frames, frame_width, frame_height, definition, homographies):
    """lambda_t (mfs.py:786-841).  Same LAPACK eigenvalue routine as the reference, batched."""
    if definition in (ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, ADAPTIVE_WEIGHTS_DEFINITION_FLIPPED):
        affine = np.array(homographies, dtype=np.float64, copy=True)
        if affine.shape != (num_frames, 3, 3):
            raise ValueError(f'homographies must have shape ({num_frames}, 3, 3)')
        affine[:, 2, :] = [0, 0, 1]                                              # mfs.py:816
        mags = np.sort(np.abs(np.linalg.eigvals(affine)), axis=1)                # mfs.py:821
        tau = np.sqrt((affine[:, 0, 2] / frame_width) ** 2 + (affine[:, 1, 2] / frame_height) ** 2)
        a = mags[:, -2] / mags[:, -1]                                            # mfs.py:824
        c1 = -1.93 * tau + 0.95                                                  # mfs.py:826
        sign = 1.0 if definition == ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL else -1.0
        c2 = 5.83 * a + sign * 4.88                                              # mfs.py:829, 831
        return np.maximum(np.minimum(c1, c2), 0.0)                               # mfs.py:833-835
    if definition == ADAPTIVE_WEIGHTS_DEFINITION_CONSTANT_HIGH:
        return np.full((num_frames,), float(ADAPTIVE_WEIGHTS_DEFINITION_CONSTANT_HIGH_VALUE))
    if definition == ADAPTIVE_WEIGHTS_DEFINITION_CONSTANT_LOW:
        return np.full((num_frames,), float(ADAPTIVE_WEIGHTS_DEFINITION_CONSTANT_LOW_VALUE))
    raise ValueError('bad adaptive_weights_definition')


def jacobi_band_coefficients(num_frames, frame_width, frame_height, definition, homographies, omega):
    """(taps[2*omega+1], lam[F], inv_on[F]): the band of the reference's dense F x F system.

    mfs.py:713-783 builds off[t,r] = -2*lam_t*w(t-r) masked to |t-r| <= omega (the band INCLUDES the
    diagonal) and on[t] = 1 + 2*lam_t*sum_{r=0}^{F-1} w(t-r) over the WHOLE row (the sum is taken before
    the mask, mfs.py:775).  w(d) = exp(-((3/omega)*d)^2).  O(F) here instead of O(F^2)."""
    F = int(num_frames)
    omega = int(omega)
    if omega < 1:
        raise ValueError('temporal_smoothing_radius must be >= 1')
    d = np.arange(-omega, omega + 1)
    taps = np.exp(-np.square((3 / omega) * d))
    lam = np.asarray(adaptive_weights(F, frame_width, frame_height, definition, homographies), dtype=np.float64)
    # row sums: sum_{r=0}^{F-1} w(t-r) = sum_{d=t-F+1}^{t} w(d)
    dd = np.arange(-(F - 1), F)
    wfull = np.exp(-np.square((3 / omega) * dd))
    csum = np.concatenate([[0.0], np.cumsum(wfull)])
    t = np.arange(F)
    row = csum[t + F] - csum[t]                     # dd index of d is d + F - 1; range [t-F+1, t]
    on = 1 + 2 * lam * row
    return taps, lam, np.reciprocal(on)             # mfs.py:873


def online_taps(omega):
    """The online smoother's taps (include/meshflow_hip.h, mf_online_smooth_f64): w(d) for d = 1 .. omega, the offline band's formula
    without its centre."""
    omega = int(omega)
    if omega < 1:
        raise ValueError('omega must be >= 1')
    return np.exp(-np.square((3 / omega) * np.arange(1, omega + 1)))


def vertex_x_y(frame_width, frame_height, mesh_rows, mesh_cols):
    """mfs.py:881-906: (V, 1, 2) float32 vertex pixel coordinates."""
    xs = [math.ceil((frame_width - 1) * (col / mesh_cols)) for col in range(mesh_cols + 1)]
    ys = [math.ceil((frame_height - 1) * (row / mesh_rows)) for row in range(mesh_rows + 1)]
    out = np.empty((mesh_rows + 1, mesh_cols + 1, 2), dtype=np.float32)
    out[..., 0] = np.asarray(xs, dtype=np.float32)[None, :]
    out[..., 1] = np.asarray(ys, dtype=np.float32)[:, None]
    return out.reshape(-1, 1, 2)


def stability_score(vertex_stabilized_displacements_by_frame_index):
    """mfs.py:1216-1259 (pure NumPy in the reference as well)."""
    xs, ys = np.swapaxes(vertex_stabilized_displacements_by_frame_index, 0, 3)
    parts = []
    for profiles in (np.diff(xs), np.diff(ys)):
        energy = np.square(np.abs(np.fft.fft(profiles)))
        total = np.sum(energy, axis=2)
        low = np.sum(energy[:, :, 1:6], axis=2)
        parts.append(np.mean(low / total))
    return (parts[0] + parts[1]) / 2.0


def shard_range(num_frames, world_size, rank):
    """Contiguous frame range [lo, hi) of `rank`: ceil(F/G) frames per rank, the tail ranks shorter."""
    per = -(-num_frames // world_size)
    lo = min(rank * per, num_frames)
    hi = min(lo + per, num_frames)
    return lo, hi


def mesh_cropping_ratio_and_distortion(frame_width, frame_height, mesh_rows, mesh_cols, unstab_disp, stab_disp,
                                       crop_boundaries):
    """(cropping_ratio, distortion_score) from the mesh itself -- a DEVIATION from mfs.py:1160-1212, not parity-pinned.

    The reference estimates, for every frame, a homography between the unstabilized and the cropped frame from
    FAST/LK feature matches (mfs.py:1195) and takes 1/(H00*H11) (mean over frames, mfs.py:1203, 1212) and the ratio
    of the two largest eigenvalue magnitudes of its affine part (MIN over frames, mfs.py:1206-1212).  The feature
    tracker is outside this build; here the same two formulas are applied to the least-squares homography through
    the (R+1)(C+1) exactly known vertex correspondences: unstabilized grid vertex -> its stabilized position ->
    crop + resize (pixel centres: x_c = (x_s - left + 0.5) * W/cw - 0.5)."""
    left, top, right, bottom = (float(v) for v in crop_boundaries)
    cw, ch = right - left + 1.0, bottom - top + 1.0
    grid = vertex_x_y(frame_width, frame_height, mesh_rows, mesh_cols).reshape(-1, 2).astype(np.float64)
    motion = (np.asarray(stab_disp, dtype=np.float64) - np.asarray(unstab_disp, dtype=np.float64)).reshape(len(stab_disp), -1, 2)
    ratios = np.empty(len(motion), dtype=np.float32)
    distortions = np.empty(len(motion), dtype=np.float32)
    X, Y = grid[:, 0], grid[:, 1]
    for f in range(len(motion)):
        ps = grid + motion[f]
        x = (ps[:, 0] - left + 0.5) * (frame_width / cw) - 0.5
        y = (ps[:, 1] - top + 0.5) * (frame_height / ch) - 0.5
        zeros, ones = np.zeros_like(X), np.ones_like(X)
        A = np.concatenate([np.stack([X, Y, ones, zeros, zeros, zeros, -x * X, -x * Y], axis=1),
                            np.stack([zeros, zeros, zeros, X, Y, ones, -y * X, -y * Y], axis=1)])
        h, *_ = np.linalg.lstsq(A, np.concatenate([x, y]), rcond=None)
        Hm = np.append(h, 1.0).reshape(3, 3)
        ratios[f] = 1 / (Hm[0][0] * Hm[1][1])                                             # mfs.py:1203
        affine = Hm.copy()
        affine[2] = [0, 0, 1]                                                            # mfs.py:1207
        mags = np.sort(np.abs(np.linalg.eigvals(affine)))
        distortions[f] = mags[-2] / mags[-1]                                              # mfs.py:1209
    return np.mean(ratios), np.min(distortions)                                           # mfs.py:1212


def pack_features(features_by_pair):
    """[(early, late), ...] as `_get_matched_features_and_homography` returns them (mfs.py:528: (K, 1, 2) arrays, or
    None when too few features were found) -> (early (K_total, 2) float64, late, offsets (P+1,) int32, max per pair).
    float32 inputs are widened exactly; the reference's own flow already carries float64 (mfs.py:578)."""
    early, late = [], []
    for pair in features_by_pair:
        e, l = pair[0], pair[1]
        e = np.zeros((0, 2)) if e is None else np.asarray(e, dtype=np.float64).reshape(-1, 2)
        l = np.zeros((0, 2)) if l is None else np.asarray(l, dtype=np.float64).reshape(-1, 2)
        if e.shape != l.shape:
            raise ValueError('early and late features of a pair must have the same shape')
        early.append(e)
        late.append(l)
    counts = [len(e) for e in early]
    offsets = np.cumsum([0] + counts).astype(np.int32)
    cat = lambda parts: np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 2))
    return cat(early), cat(late), offsets, max(counts, default=0)


# ---- the host finisher of the device tracker (tracker.py): outlier rejection and the homography, mfs.py:524-526 and 569-574 ----
# cv2.findHomography cannot be restated here: its RANSAC draws samples from OpenCV's own random generator, and both of its modes end with a
# Levenberg-Marquardt refinement.  This is a documented deviation, like the mesh-based cropping ratio above: samples of 4 come from
# `synthetic.hash32` counters (the same on every platform), degenerate samples are skipped, the number of iterations follows cv2's adaptive
# formula (RANSACUpdateNumIters), the mask is the best sample's consensus set, and every fit is a normalised DLT in float64.  There is NO
# Levenberg-Marquardt refinement.  `lsq_homography` is the specification of the tracker's fit='host' mode; fit='device' (`ops.fit_homographies`)
# has its own, tests/homography_model.py -- the same similarity and the same algebraic error through the 9 x 9 normal matrix instead of an
# SVD -- and nothing here changes for it.

def _points(a, name):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim == 3 and a.shape[1:] == (1, 2):
        a = a[:, 0, :]
    if a.ndim != 2 or a.shape[1] != 2:
        raise ValueError(f'{name} must be (K, 2) or (K, 1, 2) points, got shape {a.shape}')
    return a


def _collinear(p):
    """All points of p (K, 2) on one line (or fewer than 3 distinct): the second singular value of the centred points vanishes."""
    c = p - p.mean(axis=0)
    sv = np.linalg.svd(c, compute_uv=False)
    return len(sv) < 2 or sv[1] <= 1e-9 * max(sv[0], 1.0)


def _matched_points(early, late, caller):
    early, late = _points(early, 'early'), _points(late, 'late')
    if early.shape != late.shape:
        raise ValueError(f'{caller}: early and late must hold the same number of points')
    if len(early) < 4:
        raise ValueError(f'{caller}: a homography needs at least 4 point pairs, got {len(early)}')
    if _collinear(early) or _collinear(late):
        raise ValueError(f'{caller}: all points lie on one line: no homography is determined')
    return early, late


def _normalisation(p):
    """Hartley's similarity: centroid to the origin, mean distance sqrt(2)."""
    c = p.mean(axis=0)
    d = np.sqrt(((p - c) ** 2).sum(axis=1)).mean()
    s = math.sqrt(2.0) / d if d > 0 else 1.0
    return np.array([[s, 0.0, -s * c[0]], [0.0, s, -s * c[1]], [0.0, 0.0, 1.0]])


def _dlt(early, late):
    """Normalised DLT: the 3 x 3 matrix (h22 = 1) that minimises the algebraic error, or None where it has h22 = 0."""
    te, tl = _normalisation(early), _normalisation(late)
    e = early * te[0, 0] + te[:2, 2]
    l = late * tl[0, 0] + tl[:2, 2]
    k = len(e)
    a = np.zeros((2 * k, 9))
    a[0::2, 0:2], a[0::2, 2] = e, 1.0
    a[0::2, 6:8], a[0::2, 8] = -l[:, :1] * e, -l[:, 0]
    a[1::2, 3:5], a[1::2, 5] = e, 1.0
    a[1::2, 6:8], a[1::2, 8] = -l[:, 1:] * e, -l[:, 1]
    h = np.linalg.svd(a)[2][-1].reshape(3, 3)
    h = np.linalg.inv(tl) @ h @ te
    if abs(h[2, 2]) <= 1e-12 * np.abs(h).max():
        return None
    return h / h[2, 2]


def _reprojection_sq(h, early, late):
    w = early @ h[2, :2] + h[2, 2]
    with np.errstate(divide='ignore', invalid='ignore'):
        x = (early @ h[0, :2] + h[0, 2]) / w
        y = (early @ h[1, :2] + h[1, 2]) / w
    err = (x - late[:, 0]) ** 2 + (y - late[:, 1]) ** 2
    return np.where(np.isfinite(err), err, np.inf)


def _degenerate_sample(p):
    """cv2's checkSubset for 4 points: three of them on one line."""
    for i, j, k in ((0, 1, 2), (0, 1, 3), (0, 2, 3), (1, 2, 3)):
        d1, d2 = p[j] - p[i], p[k] - p[i]
        if abs(d1[0] * d2[1] - d1[1] * d2[0]) <= 1.1920929e-07 * (abs(d1).sum() + abs(d2).sum()):
            return True
    return False


def _ransac_iterations(confidence, outlier_ratio, max_iters):
    """cv::RANSACUpdateNumIters for 4-point models."""
    p = min(max(confidence, 0.0), 1.0)
    ep = min(max(outlier_ratio, 0.0), 1.0)
    tiny = 2.2250738585072014e-308
    num = max(1.0 - p, tiny)
    denom = 1.0 - (1.0 - ep) ** 4
    if denom < tiny:
        return 0
    num, denom = math.log(num), math.log(denom)
    return max_iters if denom >= 0 or -num >= max_iters * (-denom) else int(round(num / denom))


def ransac_inliers(early, late, threshold=3.0, confidence=0.995, max_iters=2000, seed=0):
    """The boolean inlier mask that stands in for cv2.findHomography(early, late, method=cv2.RANSAC)[1] (mfs.py:569-572): see the note above.
    ValueError for fewer than 4 pairs or points that all lie on one line.  The same inputs give the same mask on every platform's float64."""
    from . import synthetic
    early, late = _matched_points(early, late, 'ransac_inliers')
    k = len(early)
    best, best_count = np.zeros(k, dtype=bool), 0
    iterations, counter, it = int(max_iters), 0, 0
    draws = np.zeros(0, dtype=np.int64)
    while it < iterations:
        it += 1
        sample = []
        while len(sample) < 4:                                   # four DISTINCT indices from consecutive hash counters
            if counter == len(draws):
                draws = np.concatenate([draws, synthetic.hash32(np.arange(counter, counter + 1024), seed) % k])
            i = int(draws[counter])
            counter += 1
            if i not in sample:
                sample.append(i)
        if _degenerate_sample(early[sample]) or _degenerate_sample(late[sample]):
            continue
        h = _dlt(early[sample], late[sample])
        if h is None:
            continue
        mask = _reprojection_sq(h, early, late) <= threshold * threshold
        count = int(mask.sum())
        if count > max(best_count, 3):
            best, best_count = mask, count
            iterations = min(iterations, _ransac_iterations(confidence, (k - count) / k, int(max_iters)))
    if best_count < 4:
        raise ValueError('ransac_inliers: no sample of 4 pairs had 4 inliers within %g pixels' % threshold)
    return best


def lsq_homography(early, late):
    """The least-squares homography that stands in for cv2.findHomography(early, late)[0] (mfs.py:524-526): a normalised DLT over all pairs
    in float64, h22 = 1, no Levenberg-Marquardt refinement (cv2 refines its own linear estimate; the two agree where the pairs fit a
    homography).  ValueError for fewer than 4 pairs or points that all lie on one line."""
    early, late = _matched_points(early, late, 'lsq_homography')
    h = _dlt(early, late)
    if h is None:
        raise ValueError('lsq_homography: the fitted matrix sends the origin to infinity')
    return h
