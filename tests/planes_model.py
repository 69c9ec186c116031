"""NumPy restatement of what OpenCV 4.5-4.10 computes for the side planes of a video -- float32 planes through INTER_LINEAR, elements of
1, 2, 4 or 8 bytes through INTER_NEAREST -- in cv2.remap (mfs.py:1063-1069) and cv2.resize (mfs.py:1150-1155).  MODELLED, NOT PINNED, like
tests/cv16_model.py, from whose pieces (and oracle/meshflow_oracle.py's) the four models are put together.

cv2.remap(plane CV_32FC1, map_x, map_y, INTER_LINEAR, BORDER_CONSTANT, borderValue=fill) (imgwarp.cpp RemapInvoker +
remapBilinear<Cast<float, float>, RemapNoVec, float>): cv16_model.remap_bilinear_u16c3 on one channel without saturate_cast -- the 8-bit map
quantisation sx = cvRound(32 u), ix = sat_short(sx >> 5), fx = sx & 31, BilinearTab_f's exact float32 weights, t = ((S00 w0 + S01 w1) +
S10 w2) + S11 w3 with every product and sum rounded on its own, out = t; a 2x2 footprint wholly outside gives float32(fill), otherwise each
outside tap is fill inside the same sum.
  ASSUMED: 32F has a SIMD remap (RemapVec_32f?) in no baseline build -- remapBilinear's vector operation for float is RemapNoVec.

cv2.remap(..., INTER_NEAREST, BORDER_CONSTANT) (remapNearest after RemapInvoker's map conversion): ix = sat_short(cvRound(u)), iy =
sat_short(cvRound(v)), cvRound on the float32 coordinate (half to even); the element is copied where 0 <= ix < W and 0 <= iy < H, otherwise
the result is fill cast to the element type.

cv2.resize(crop CV_32FC1, (w, h)) INTER_LINEAR (resize.cpp HResizeLinear<float, float, float> + VResizeLinear<float, float, float,
Cast<float, float>>): cv16_model.resize_linear_u16 without saturate_cast.  EXACTLY 2x down in both axes cv::hal::resize hands INTER_LINEAR to
INTER_AREA's fast path, as tests/cv16_area.py describes for uint16; there the 16-bit form is the integer (S00 + S01 + S10 + S11 + 2) >> 2,
here -- ResizeAreaFastNoVec<float, float> under resizeAreaFast_<float, float, ...>, scale 2 -- it is the float32 sum in the scalar code's
order times 0.25f: (((S00 + S01) + S10) + S11) * 0.25f.
  ASSUMED / CHOSEN: that scalar order.  ResizeAreaFastVec_SIMD_32f adds the two rows first ((S00 + S10) + (S01 + S11)), which rounds
  differently; the model takes the scalar order.

cv2.resize(..., INTER_NEAREST) (resizeNN): sx = min(floor(x * ifx), src_w - 1) with ifx = 1. / inv_scale_x, inv_scale_x = (double)dst_w /
src_w, float64, the two divisions as written; the same for y; the element is copied.

NON-FINITE SAMPLES, SIGNED ZEROS, SUBNORMALS.  Every operation above is an IEEE-754 binary32 operation, rounded to nearest even on its own,
subnormals kept (nothing is flushed to zero), and nothing looks at a sample's value before using it:
  remap_linear_f32: all four products are always formed -- a weight of 0 does not exclude its tap, so a +-Inf or NaN tap with weight 0 gives
  NaN (0 * Inf), as remapBilinear's unconditional sum does; an outside tap is `fill` INSIDE that sum (a +Inf fill with weight 0: NaN); a
  2 x 2 footprint wholly outside, and an unowned pixel, give float32(fill)'s own bits (-0.0 stays -0.0; a NaN fill gives a NaN).
  resize_linear_f32, horizontal pass (HResizeLinear): the two-tap loop D[dx] = S[sx] a0 + S[sx + 1] a1 runs for dx < xmax, the one-tap tail
  D[dx] = S[xofs[dx]] * ONE (ONE = 1.0f) from xmax on, where xmax is the first dx whose sx + 1 >= src_w -- the columns whose sx was clamped
  to src_w - 1.  S * 1.0f is S: +-Inf stays +-Inf there (the two-tap form would give Inf * 1 + Inf * 0 = NaN), -0.0 stays -0.0.  The columns
  clamped on the LEFT (sx < 0 -> sx = 0, f = 0) stay in the two-tap loop: S[0] * 1 + S[1] * 0.  With src_w = 1 every column is in the tail.
  resize_linear_f32, vertical pass (VResizeLinear): always two taps, D = S0 b0 + S1 b1 with b = (1 - fy, fy) and the two row indices
  clipped into the crop; fy is never reset, so a clipped row pair is the same row twice with weights summing to 1.
  resize_linear_f32, exactly 2x down: (((S00 + S01) + S10) + S11) * 0.25f in that order -- the first partial sum may overflow to +-Inf
  where another pairing would not; four subnormals give their exact (subnormal) sum times 0.25f, rounded to even.
  resize_linear_f32, identity size: cv::resize begins with `if (dsize == ssize) { src.copyTo(dst); return; }` -- a crop of the output's own
  size is a bit copy (NaN payloads, -0.0 and all), not the f = 0 arithmetic.  The nearest resize at identity size copies anyway.
  A NaN result's sign and payload are not modelled: x86 and gfx950 generate different default NaNs; callers compare NaN-ness.
  ASSUMED: resize.cpp read as above (4.5-4.10: HResizeLinear's `for (; dx < dwidth; dx++) D[dx] = WT(S[xofs[dx]] * ONE)` after the xmax
  loop; the dsize == ssize copy at the head of cv::resize); no cv2 was run against it.  The float SIMD rows (HResizeLinearVec_X4,
  VResizeLinearVec_32f) compute the same unfused products and sums."""
import numpy as np

import cv16_model
from oracle import meshflow_oracle as mo

F32 = np.float32


def remap_linear_f32(src, map_x_f32, map_y_f32, fill=0.0):
    """cv2.remap(src float32 HxW, map_x, map_y float32, INTER_LINEAR, BORDER_CONSTANT, borderValue=fill), as modelled above."""
    src = np.asarray(src, dtype=F32)
    sh, sw = src.shape
    with np.errstate(over='ignore', invalid='ignore'):
        sx = mo._cv_round_f32(np.asarray(map_x_f32, dtype=F32) * F32(32))
        sy = mo._cv_round_f32(np.asarray(map_y_f32, dtype=F32) * F32(32))
    ix = np.clip(sx >> 5, -32768, 32767)
    iy = np.clip(sy >> 5, -32768, 32767)
    w = cv16_model.weights_f32(sx & 31, sy & 31)
    cval = F32(fill)
    outside = (ix >= sw) | (ix + 1 < 0) | (iy >= sh) | (iy + 1 < 0)
    t = None
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):     # ((S00 w0 + S01 w1) + S10 w2) + S11 w3
        tx, ty = ix + dx, iy + dy
        inside = (tx >= 0) & (tx < sw) & (ty >= 0) & (ty < sh)
        tap = np.where(inside, src[np.clip(ty, 0, sh - 1), np.clip(tx, 0, sw - 1)], cval).astype(F32)
        with np.errstate(over='ignore', invalid='ignore', under='ignore'):
            term = tap * w[k]                                               # always formed: 0 * Inf is NaN
            t = term if t is None else t + term
    return np.where(outside, cval, t).astype(F32)


def nearest_indices(map_x_f32, map_y_f32):
    """ix = sat_short(cvRound(u)), iy = sat_short(cvRound(v))."""
    with np.errstate(over='ignore', invalid='ignore'):
        ix = np.clip(mo._cv_round_f32(np.asarray(map_x_f32, dtype=F32)), -32768, 32767)
        iy = np.clip(mo._cv_round_f32(np.asarray(map_y_f32, dtype=F32)), -32768, 32767)
    return ix, iy


def remap_nearest(src, map_x_f32, map_y_f32, fill):
    """cv2.remap(src HxW of any element type, INTER_NEAREST, BORDER_CONSTANT): `fill` is an element of src's dtype."""
    src = np.asarray(src)
    sh, sw = src.shape
    ix, iy = nearest_indices(map_x_f32, map_y_f32)
    inside = (ix >= 0) & (ix < sw) & (iy >= 0) & (iy < sh)
    return np.where(inside, src[np.clip(iy, 0, sh - 1), np.clip(ix, 0, sw - 1)], np.asarray(fill, dtype=src.dtype)).astype(src.dtype)


def resize_linear_f32(src, dst_w, dst_h):
    """cv2.resize(src float32 HxW, (dst_w, dst_h)) with INTER_LINEAR: a copy at the source's own size, the area branch at exactly 2x down in
    both axes, the float path everywhere else (two taps below xmax, one from xmax on)."""
    src = np.asarray(src, dtype=F32)
    sh, sw = src.shape
    if sh == 0 or sw == 0:
        raise ValueError('cv2.resize: empty source (the crop rectangle is empty)')
    if sw == 2 * dst_w and sh == 2 * dst_h:
        with np.errstate(over='ignore', invalid='ignore', under='ignore'):
            return (((src[0::2, 0::2] + src[0::2, 1::2]) + src[1::2, 0::2]) + src[1::2, 1::2]) * F32(0.25)
    if sw == dst_w and sh == dst_h:                   # cv::resize: dsize == ssize is src.copyTo(dst)
        return src.copy()
    sx, fx = mo.resize_linear_tables(sw, dst_w)
    low = sx < 0
    sx = np.where(low, 0, sx); fx = np.where(low, F32(0), fx).astype(F32)
    tail = sx >= sw - 1                               # dx >= xmax: HResizeLinear's one-tap tail, S[sw - 1] * 1.0f
    sx = np.where(tail, sw - 1, sx); fx = np.where(tail, F32(0), fx).astype(F32)
    a0, a1 = F32(1) - fx, fx
    sy, fy = mo.resize_linear_tables(sh, dst_h)
    b0, b1 = F32(1) - fy, fy.astype(F32)
    sy0 = np.clip(sy, 0, sh - 1)
    sy1 = np.clip(sy + 1, 0, sh - 1)
    sx1 = np.minimum(sx + 1, sw - 1)
    with np.errstate(over='ignore', invalid='ignore', under='ignore'):
        def row(r):
            return np.where(tail[None, :], r[:, sx], r[:, sx] * a0[None, :] + r[:, sx1] * a1[None, :]).astype(F32)
        return (row(src[sy0]) * b0[:, None] + row(src[sy1]) * b1[:, None]).astype(F32)


def resize_nearest(src, dst_w, dst_h):
    """cv2.resize(src HxW of any element type, (dst_w, dst_h)) with INTER_NEAREST."""
    src = np.asarray(src)
    sh, sw = src.shape
    if sh == 0 or sw == 0:
        raise ValueError('cv2.resize: empty source (the crop rectangle is empty)')
    ifx = 1.0 / (float(dst_w) / float(sw))
    ify = 1.0 / (float(dst_h) / float(sh))
    sx = np.minimum(np.floor(np.arange(dst_w, dtype=np.float64) * ifx).astype(np.int64), sw - 1)
    sy = np.minimum(np.floor(np.arange(dst_h, dtype=np.float64) * ify).astype(np.int64), sh - 1)
    return src[sy][:, sx]


def crop_planes(planes, bounds, interpolation, size=None):
    """mfs.py:1111-1157 on planes (n, H, W): crop to the inclusive bounds and resize to size = (width, height), by default back to (W, H)."""
    H, W = planes.shape[1:3]
    ow, oh = (W, H) if size is None else size
    left, top, right, bottom = (int(v) for v in bounds)
    fn = resize_linear_f32 if interpolation == 'linear' else resize_nearest
    return np.stack([fn(p[top:bottom + 1, left:right + 1], ow, oh) for p in planes])
