"""NumPy restatement of what the reference computes for uint16 (CV_16UC3) frames: cv2.remap at mfs.py:1063-1069 and cv2.resize at
mfs.py:1150-1155, OpenCV 4.5-4.10 -- the range oracle/meshflow_oracle.py models for 8-bit.  MODELLED, NOT PINNED: no OpenCV was at hand
to check it against.

cv2.remap, INTER_LINEAR, BORDER_CONSTANT, float32 maps (imgwarp.cpp RemapInvoker + remapBilinear<Cast<float, ushort>, RemapNoVec, float>):
  * the map quantisation of the 8-bit path: sx = cvRound(map_x * 32) (float32 product, rounded half to even), ix = sat_short(sx >> 5),
    fx = sx & 31, the same for y;
  * weights BilinearTab_f[fy][fx] = {(1-fy/32)(1-fx/32), (1-fy/32)(fx/32), (fy/32)(1-fx/32), (fy/32)(fx/32)}: float32, exact (dyadic),
    no fix-up like the fixed-point table's;
  * t = ((S00 w0 + S01 w1) + S10 w2) + S11 w3 in float32, each product and sum rounded on its own (the scalar RemapNoVec code: 16U has
    no SIMD remap);
  * out = saturate_cast<ushort>(t) = clamp(rint_half_even(t), 0, 65535);
  * borders as in the 8-bit path: a 2x2 footprint wholly outside gives cval, otherwise each outside tap is cval inside the same sum
    (pixels with ix == W-1 or iy == H-1 go through that branch too: the same value);
  * cval[k] = saturate_cast<ushort>(borderValue[k]): the default (0, 0, 255) stays (0, 0, 255), it is not scaled to 16 bits.
  ASSUMED: the IPP remap is compiled out in these versions, so the generic code above runs.

cv2.resize, INTER_LINEAR (resize.cpp resizeGeneric_ with HResizeLinear<ushort, float, float, 1, ...> + VResizeLinear<ushort, float, float,
Cast<float, ushort>, ...>):
  * the 8-bit index and fraction tables (oracle.meshflow_oracle.resize_linear_tables: float32 f, floor s; x clamped to [0, src-1] with
    f = 0 there; the y rows clipped), but float32 coefficients (1 - f, f): no x2048, no rounding;
  * horizontal t = float(S[sx]) a0 + float(S[sx+1]) a1, float32, unfused (the one-tap right-edge branch gives the same value);
  * vertical out = saturate_cast<ushort>(t0 b0 + t1 b1), float32, unfused, rounded half to even.
  ASSUMED: the SIMD versions (HResizeLinearVec_16u32f, VResizeLinearVec_32f16u) compute the same products and sums in baseline x86-64
  builds, which have no FMA; and no IPP resize runs for this depth and interpolation.

NumPy float32 arithmetic rounds every operation on its own, so the expressions below are the float32 chains above, term for term."""
import numpy as np

from oracle import meshflow_oracle as mo

F32 = np.float32


def border_u16(border_bgr):
    """cval = saturate_cast<ushort>(borderValue): clamp(round(v), 0, 65535), per channel."""
    return np.clip(np.rint(np.asarray(border_bgr, dtype=np.float64)[:3]), 0, 65535).astype(np.int64)


def weights_f32(fx, fy):
    """BilinearTab_f[fy][fx] as four float32 arrays (exact)."""
    ax = fx.astype(F32) * F32(1.0 / 32)
    ay = fy.astype(F32) * F32(1.0 / 32)
    ax0 = F32(1) - ax
    ay0 = F32(1) - ay
    return ay0 * ax0, ay0 * ax, ay * ax0, ay * ax


def saturate_u16(t):
    return np.clip(np.rint(t.astype(np.float64)), 0, 65535).astype(np.uint16)


def remap_bilinear_u16c3(src, map_x_f32, map_y_f32, border_bgr=(0, 0, 255)):
    """cv2.remap(src uint16 HxWx3, map_x, map_y float32, INTER_LINEAR, BORDER_CONSTANT, borderValue), as modelled above."""
    src = np.asarray(src, dtype=np.uint16)
    sh, sw = src.shape[:2]
    mx = np.asarray(map_x_f32, dtype=F32)
    my = np.asarray(map_y_f32, dtype=F32)
    with np.errstate(over='ignore', invalid='ignore'):
        sx = mo._cv_round_f32(mx * F32(32))
        sy = mo._cv_round_f32(my * F32(32))
    ix = np.clip(sx >> 5, -32768, 32767)
    iy = np.clip(sy >> 5, -32768, 32767)
    w = weights_f32(sx & 31, sy & 31)
    cval = border_u16(border_bgr)
    outside = (ix >= sw) | (ix + 1 < 0) | (iy >= sh) | (iy + 1 < 0)
    t = None
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):     # ((S00 w0 + S01 w1) + S10 w2) + S11 w3
        tx = ix + dx
        ty = iy + dy
        inside = (tx >= 0) & (tx < sw) & (ty >= 0) & (ty < sh)
        tap = src[np.clip(ty, 0, sh - 1), np.clip(tx, 0, sw - 1)].astype(np.int64)
        tap = np.where(inside[..., None], tap, cval).astype(F32)
        term = tap * w[k][..., None]
        t = term if t is None else t + term
    out = saturate_u16(t)
    return np.where(outside[..., None], cval.astype(np.uint16), out).astype(np.uint16)


def warp_maps(W, H, R, C, unstab_f, stab_f):
    """The reference's coordinate maps and per-frame crop values of one frame (C oracle: pixel-type independent), and its bad-cell count."""
    from oracle import clib
    table, bad = clib.cell_table(W, H, R, C, unstab_f, stab_f)
    _, crop, mx, my = clib.warp_frame(np.zeros((H, W, 3), np.uint8), R, C, table, use_bbox=True, want_maps=True)
    return mx, my, crop, bad


def warp_clip_u16(frames, R, C, unstab, stab, border_bgr=(0, 0, 255)):
    """_get_stabilized_frames_and_crop_boundaries' frames and per-frame crop values for a uint16 clip (n, H, W, 3)."""
    frames = np.asarray(frames, dtype=np.uint16)
    n, H, W = frames.shape[:3]
    out = np.empty_like(frames)
    crop = np.zeros((n, 4), np.int32)
    for f in range(n):
        mx, my, crop[f], bad = warp_maps(W, H, R, C, unstab[f], stab[f])
        assert bad == 0
        out[f] = remap_bilinear_u16c3(frames[f], mx, my, border_bgr)
    return out, crop


def resize_linear_u16(src, dst_w, dst_h):
    """cv2.resize(src uint16 HxWxC, (dst_w, dst_h)) with INTER_LINEAR, as modelled above."""
    src = np.asarray(src, dtype=np.uint16)
    sh, sw = src.shape[:2]
    if sh == 0 or sw == 0:
        raise ValueError('cv2.resize: empty source (the crop rectangle is empty)')
    sx, fx = mo.resize_linear_tables(sw, dst_w)
    low = sx < 0
    sx = np.where(low, 0, sx); fx = np.where(low, F32(0), fx).astype(F32)
    high = sx >= sw - 1
    sx = np.where(high, sw - 1, sx); fx = np.where(high, F32(0), fx).astype(F32)
    a0, a1 = F32(1) - fx, fx
    sy, fy = mo.resize_linear_tables(sh, dst_h)
    b0, b1 = F32(1) - fy, fy.astype(F32)
    sy0 = np.clip(sy, 0, sh - 1)
    sy1 = np.clip(sy + 1, 0, sh - 1)
    sx1 = np.minimum(sx + 1, sw - 1)                 # where sx = sw-1 the second weight is 0
    S = src.astype(F32)
    t0 = S[sy0][:, sx] * a0[None, :, None] + S[sy0][:, sx1] * a1[None, :, None]
    t1 = S[sy1][:, sx] * a0[None, :, None] + S[sy1][:, sx1] * a1[None, :, None]
    return saturate_u16(t0 * b0[:, None, None] + t1 * b1[:, None, None])


def crop_frames_u16(frames, bounds):
    """mfs.py:1111-1157 for uint16 frames (n, H, W, 3): crop to the inclusive bounds and resize back to (W, H)."""
    H, W = frames.shape[1:3]
    left, top, right, bottom = (int(v) for v in bounds)
    return np.stack([resize_linear_u16(f[top:bottom + 1, left:right + 1], W, H) for f in frames])
