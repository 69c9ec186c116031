"""NumPy model of the device tracker: FAST corners, the LK pyramid, Scharr derivatives and pyramidal Lucas-Kanade on one-channel uint8
images, per sub-frame as mfs.py:492-516 and 581-629 call them.  This file is the specification of csrc/track_*.hip: the device equals it bit
for bit (tests/test_gpu_track.py).  It restates OpenCV 4.5-4.10 (fast.cpp, fast_score.cpp, pyramids.cpp, lkpyramid.cpp) for CV_8UC1.

No machine this project is built or tested on has OpenCV, so NOTHING here was checked against cv2; all of it is from recall of the sources:

  * FAST (FAST_t<16>, cornerScore<16>): circle offsets, "9 contiguous of 16 strictly brighter than p + t or strictly darker than p - t", no
    corner within 3 pixels of an edge, score = the largest threshold at which the pixel is still a corner = max(t, A, B) - 1 with A / B the
    best 9-arc minimum of (p - x) / (x - p), non-corners score 0, a corner is kept if its score is strictly greater than all 8 neighbours'.
    (cornerScore's early `continue`s and FAST_t's quick rejections are shortcuts that do not change these results.)
  * pyrDown: [1 4 6 4 1] x [1 4 6 4 1] in integers, (sum + 128) >> 8, BORDER_REFLECT_101, size ((w+1)//2, (h+1)//2);
    buildOpticalFlowPyramid stops BEFORE a level whose width or height is not larger than the window (21).
  * calcOpticalFlowPyrLK with images (no ready-made pyramid): every level gets a 21-pixel BORDER_REFLECT_101 border for the patch taps;
    calcSharrDeriv runs on the level alone with reflect-101 at ITS edges, and the derivative image is padded with ZEROS.
  * LKTrackerInvoker: the float32 sequence of prevPt / nextPt, cvFloor, the 14-bit weights with the fourth as the remainder, CV_DESCALE by 9
    bits (patch, stored as int16 scaled by 32) and 14 bits (derivatives), "lost" flagged at level 0 only, minEig and D tests, the update,
    epsilon^2 against the float64 dot product, the "moved back by less than 0.01 twice" half-step exit, and -- because the Python binding
    always asks for `err` -- the second bounds test on the final position at level 0, which can clear the flag after the iterations.
    THREE recalled details matter most and are the first to check when cv2 is at hand: that second bounds test, cvRound(float) rounding
    half to even, and the zero (not reflected) border of the derivative image.

One deliberate difference from cv2: it accumulates A11, A12, A22, b1, b2 in float32 in an order that depends on its SIMD width; here the
exact integer products are summed in int64 (order-independent), converted ONCE to float32 and multiplied by FLT_SCALE.  Everything after
that is the fixed sequence of float32 operations written out below.  The model therefore equals cv2 up to the float32 rounding of five sums.

A second limit is the device's, not cv2's: a sub-frame keeps at most `max_per_subframe` corners, the first ones in row-major order
(`track_pair_features(max_per_subframe=...)`; None = all, as cv2)."""
import math

import numpy as np

F32 = np.float32
WIN = 21
HALF = F32(10.0)                        # (winSize - 1) * 0.5f
W_BITS = 14
FLT_SCALE = F32(1.0 / (1 << 20))
FLT_EPSILON = F32(1.1920929e-07)
MIN_EIG_THRESHOLD = 1e-4                # (double, as cv2's default argument)
MAX_COUNT = 30
EPSILON_SQ = 0.01 * 0.01                # criteria.epsilon *= criteria.epsilon (double)
CIRCLE = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1),
          (-2, 2), (-1, 3))             # (dx, dy), fast.cpp makeOffsets, patternSize 16


def reflect101(p, n):
    """cv::borderInterpolate(p, n, BORDER_REFLECT_101) for any p (it loops; this is its closed form)."""
    p = np.asarray(p, dtype=np.int64)
    if n == 1:
        return np.zeros_like(p)
    period = 2 * (n - 1)
    p = np.abs(p) % period
    return np.where(p >= n, period - p, p)


def fast_scores(img, threshold=10):
    """int32 (h, w): cornerScore<16> where the pixel is a corner at `threshold`, 0 elsewhere."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    h, w = img.shape
    score = np.zeros((h, w), dtype=np.int32)
    if h < 7 or w < 7:
        return score
    p = img.astype(np.int32)
    d = np.stack([p[3:h - 3, 3:w - 3] - p[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx] for dx, dy in CIRCLE])
    d = np.concatenate([d, d[:8]])
    darker = np.stack([d[k:k + 9].min(axis=0) for k in range(16)]).max(axis=0)          # A: the best arc of p - x
    brighter = np.stack([(-d[k:k + 9]).min(axis=0) for k in range(16)]).max(axis=0)     # B: the best arc of x - p
    best = np.maximum(darker, brighter)
    score[3:h - 3, 3:w - 3] = np.where(best > threshold, best - 1, 0)
    return score


def fast_corners(img, threshold=10):
    """FastFeatureDetector_create().detect(img) as float32 (N, 2) of (x, y), row-major (y outer, x inner)."""
    s = fast_scores(img, threshold)
    h, w = s.shape
    pad = np.zeros((h + 2, w + 2), dtype=np.int32)
    pad[1:-1, 1:-1] = s
    keep = s > 0
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            if (dy, dx) != (1, 1):
                keep &= s > pad[dy:dy + h, dx:dx + w]
    ys, xs = np.nonzero(keep)
    return np.stack([xs, ys], axis=1).astype(np.float32).reshape(-1, 2)


def pyr_down(img):
    img = np.asarray(img)
    h, w = img.shape
    ow, oh = (w + 1) // 2, (h + 1) // 2
    k = np.array([1, 4, 6, 4, 1], dtype=np.int32)
    xs = reflect101(2 * np.arange(ow)[:, None] + np.arange(-2, 3)[None, :], w)
    ys = reflect101(2 * np.arange(oh)[:, None] + np.arange(-2, 3)[None, :], h)
    rows = (img.astype(np.int32)[:, xs] * k).sum(axis=2)                                 # (h, ow)
    out = (rows[ys] * k[None, :, None]).sum(axis=1)                                      # (oh, ow)
    return ((out + 128) >> 8).astype(np.uint8)


def num_levels(w, h, max_level=3, win=WIN):
    """The level count minus one that buildOpticalFlowPyramid returns for a w x h image."""
    level = 0
    while level < max_level:
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= win or h <= win:
            break
        level += 1
    return level


def build_pyramid(img, max_level=3, win=WIN):
    levels = [np.asarray(img)]
    for _ in range(num_levels(img.shape[1], img.shape[0], max_level, win)):
        levels.append(pyr_down(levels[-1]))
    return levels


def scharr(img):
    """(Ix, Iy) int16: (3, 10, 3) x (-1, 0, 1), reflect-101 at the image's own edges (calcSharrDeriv)."""
    img = np.asarray(img)
    h, w = img.shape
    p = img.astype(np.int32)[reflect101(np.arange(-1, h + 1), h)][:, reflect101(np.arange(-1, w + 1), w)]
    t0 = (p[:-2] + p[2:]) * 3 + p[1:-1] * 10                                             # (h, w + 2)
    t1 = p[2:] - p[:-2]
    ix = t0[:, 2:] - t0[:, :-2]
    iy = (t1[:, 2:] + t1[:, :-2]) * 3 + t1[:, 1:-1] * 10
    return ix.astype(np.int16), iy.astype(np.int16)


_PAD = WIN + 1          # taps reach from -21 to size + 20


def _weights(frac_x, frac_y):
    one = F32(1.0)
    scale = F32(1 << W_BITS)
    w00 = np.rint((one - frac_x) * (one - frac_y) * scale).astype(np.int64)              # cvRound: half to even
    w01 = np.rint(frac_x * (one - frac_y) * scale).astype(np.int64)
    w10 = np.rint((one - frac_x) * frac_y * scale).astype(np.int64)
    return w00, w01, w10, (1 << W_BITS) - w00 - w01 - w10


def _bilinear(padded, ix, iy, w4, shift):
    """CV_DESCALE of the four-tap sum over the 21 x 21 window whose top-left tap is (ix, iy): int64 (n, 21, 21)."""
    yy = (iy[:, None, None] + np.arange(WIN)[None, :, None] + _PAD)
    xx = (ix[:, None, None] + np.arange(WIN)[None, None, :] + _PAD)
    w00, w01, w10, w11 = (v[:, None, None] for v in w4)
    s = padded[yy, xx] * w00 + padded[yy, xx + 1] * w01 + padded[yy + 1, xx] * w10 + padded[yy + 1, xx + 1] * w11
    return (s + (1 << (shift - 1))) >> shift


def _f32sum(v):
    """The exact integer sum, rounded once to float32, times FLT_SCALE."""
    return v.reshape(v.shape[0], -1).sum(axis=1).astype(np.float64).astype(np.float32) * FLT_SCALE


def _outside(ip, w, h):
    return (ip[:, 0] < -WIN) | (ip[:, 0] >= w) | (ip[:, 1] < -WIN) | (ip[:, 1] >= h)


def lk_track(early, late, points, max_level=3):
    """calcOpticalFlowPyrLK(early, late, points, None) with its defaults -> (moved float32 (N, 2), found uint8 (N,))."""
    early, late = np.asarray(early), np.asarray(late)
    assert early.dtype == np.uint8 and late.dtype == np.uint8 and early.shape == late.shape and early.ndim == 2
    pts = np.asarray(points, dtype=np.float32).reshape(-1, 2)
    n = len(pts)
    moved = np.zeros((n, 2), dtype=np.float32)
    found = np.ones(n, dtype=bool)
    if n == 0:
        return moved, found.astype(np.uint8)
    pyr_e, pyr_l = build_pyramid(early, max_level), build_pyramid(late, max_level)
    top = len(pyr_e) - 1
    for level in range(top, -1, -1):
        img, nxt_img = pyr_e[level], pyr_l[level]
        h, w = img.shape
        ry, rx = reflect101(np.arange(-_PAD, h + _PAD), h), reflect101(np.arange(-_PAD, w + _PAD), w)
        pad_i = img.astype(np.int64)[ry][:, rx]
        pad_j = nxt_img.astype(np.int64)[ry][:, rx]
        dx, dy = scharr(img)
        pad_dx = np.pad(dx.astype(np.int64), _PAD)
        pad_dy = np.pad(dy.astype(np.int64), _PAD)
        prev = pts * F32(1.0 / (1 << level))
        moved = prev.copy() if level == top else moved * F32(2.0)
        prev = prev - HALF
        ip = np.floor(prev).astype(np.int64)
        lost = _outside(ip, w, h)
        if level == 0:
            found &= ~lost
        idx = np.nonzero(~lost)[0]
        if len(idx) == 0:
            continue
        ip, prev = ip[idx], prev[idx]
        w4 = _weights(prev[:, 0] - ip[:, 0].astype(np.float32), prev[:, 1] - ip[:, 1].astype(np.float32))
        patch = _bilinear(pad_i, ip[:, 0], ip[:, 1], w4, W_BITS - 5)
        gx = _bilinear(pad_dx, ip[:, 0], ip[:, 1], w4, W_BITS)
        gy = _bilinear(pad_dy, ip[:, 0], ip[:, 1], w4, W_BITS)
        a11, a12, a22 = _f32sum(gx * gx), _f32sum(gx * gy), _f32sum(gy * gy)
        det = a11 * a22 - a12 * a12
        min_eig = (a22 + a11 - np.sqrt((a11 - a22) * (a11 - a22) + F32(4.0) * a12 * a12)) / F32(2 * WIN * WIN)
        weak = (min_eig.astype(np.float64) < MIN_EIG_THRESHOLD) | (det < FLT_EPSILON)
        if level == 0:
            found[idx[weak]] = False
        ok = ~weak
        idx, patch, gx, gy, a11, a12, a22, det = idx[ok], patch[ok], gx[ok], gy[ok], a11[ok], a12[ok], a22[ok], det[ok]
        inv = F32(1.0) / det
        pos = moved[idx] - HALF                               # nextPt -= halfWin
        prev_delta = np.zeros((len(idx), 2), dtype=np.float32)
        run = np.arange(len(idx))
        for j in range(MAX_COUNT):
            if len(run) == 0:
                break
            ipos = np.floor(pos[run]).astype(np.int64)
            lost = _outside(ipos, w, h)
            if level == 0:
                found[idx[run[lost]]] = False
            run, ipos = run[~lost], ipos[~lost]
            if len(run) == 0:
                break
            w4 = _weights(pos[run, 0] - ipos[:, 0].astype(np.float32), pos[run, 1] - ipos[:, 1].astype(np.float32))
            diff = _bilinear(pad_j, ipos[:, 0], ipos[:, 1], w4, W_BITS - 5) - patch[run]
            b1, b2 = _f32sum(diff * gx[run]), _f32sum(diff * gy[run])
            delta = np.stack([(a12[run] * b2 - a22[run] * b1) * inv[run], (a12[run] * b1 - a11[run] * b2) * inv[run]], axis=1)
            pos[run] = pos[run] + delta
            moved[idx[run]] = pos[run] + HALF
            d64 = delta.astype(np.float64)
            done = d64[:, 0] * d64[:, 0] + d64[:, 1] * d64[:, 1] <= EPSILON_SQ
            if j > 0:
                back = delta + prev_delta[run]
                half = ~done & (np.abs(back[:, 0]).astype(np.float64) < 0.01) & (np.abs(back[:, 1]).astype(np.float64) < 0.01)
                moved[idx[run[half]]] = moved[idx[run[half]]] - delta[half] * F32(0.5)
                done |= half
            prev_delta[run] = delta
            run = run[~done]
    # the bounds test in front of the error measure (level 0; the Python binding always passes `err`)
    last = np.floor(moved - HALF).astype(np.int64)
    found &= ~_outside(last, early.shape[1], early.shape[0])
    return moved, found.astype(np.uint8)


def subframes(width, height, sub_rows, sub_cols):
    """[(left, top, w, h)] in the reference's order (mfs.py:503-504: left outer, top inner)."""
    sub_w, sub_h = math.ceil(width / sub_cols), math.ceil(height / sub_rows)
    return [(left, top, min(sub_w, width - left), min(sub_h, height - top))
            for left in range(0, width, sub_w) for top in range(0, height, sub_h)]


def track_subframes(early, late, sub_rows, sub_cols, max_per_subframe=None, threshold=10):
    """Per sub-frame, each an image of its own: (corners (k, 2) float32 relative to the sub-frame -- at most max_per_subframe, the first in
    row-major order --, the true corner count, moved (k, 2), found (k,))."""
    out = []
    for left, top, w, h in subframes(early.shape[1], early.shape[0], sub_rows, sub_cols):
        e = np.ascontiguousarray(early[top:top + h, left:left + w])
        l = np.ascontiguousarray(late[top:top + h, left:left + w])
        corners = fast_corners(e, threshold)
        total = len(corners)
        if max_per_subframe is not None:
            corners = corners[:max_per_subframe]
        moved, found = lk_track(e, l, corners)
        out.append((corners, total, moved, found))
    return out


def track_pair_features(early, late, sub_rows, sub_cols, min_features, max_per_subframe=None):
    """mfs.py:492-516 and 581-629 up to the RANSAC call: [(offset (left, top), early (k, 2) float32, late (k, 2) float32)] of the sub-frames
    that pass both `min_features` gates, coordinates still relative to the sub-frame (the caller adds the offset after its outlier step,
    which promotes them to float64, mfs.py:578)."""
    out = []
    parts = track_subframes(early, late, sub_rows, sub_cols, max_per_subframe)
    for (left, top, _, _), (corners, _, moved, found) in zip(subframes(early.shape[1], early.shape[0], sub_rows, sub_cols), parts):
        if len(corners) < min_features:
            continue
        keep = found.astype(bool)
        if keep.sum() < min_features:
            continue
        out.append(((left, top), corners[keep], moved[keep]))
    return out
