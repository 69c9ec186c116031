"""NumPy model of the NV12 warp (`ops.warp_nv12`, mf_warp_nv12), put together from oracle/meshflow_oracle.py's 8-bit remap.  MODELLED on OpenCV
4.5-4.10 like every other format, NOT PINNED: no cv2 was run against it.

An NV12 frame is a luma plane y (H, W) uint8 and an interleaved chroma plane uv (H/2, W/2, 2) uint8, U first; W and H are even.  Given the
warp's float32 maps (mx, my) of the luma frame (frame_stabilized_x_y, mfs.py:1054-1061 -- what cv2.remap gets at mfs.py:1063-1069; a pixel no
cell owns holds (W + 1, H + 1)):

  luma    cv2.remap(y, mx, my, INTER_LINEAR, BORDER_CONSTANT, borderValue = border_yuv[0]) on CV_8UC1: the 8-bit fixed-point path works per
          channel, so it is channel 0 of `mo.remap_bilinear_u8c3` on the plane repeated three times.
  chroma  sited at the EVEN luma sample, by definition: output chroma sample (cx, cy) takes the map of luma pixel (2 cx, 2 cy), halved in
          float32 (u * 0.5f is exact), and the (H/2, W/2) two-channel plane goes through the same 8-bit remap: sx = cvRound(32 uc), ix =
          sat_short(sx >> 5), fx = sx & 31, weights from the 2^15 table, (sum + 2^14) >> 15 per channel; a 2 x 2 footprint wholly outside gives
          (border_yuv[1], border_yuv[2]), otherwise each outside tap is that border sample inside the sum.  CV_8UC2 is the per-channel path of
          CV_8UC3 on two channels: `mo.remap_bilinear_u8c3` of stack(U, V, U), channels 0 and 1.  An unowned pixel halves to
          ((W + 1) / 2, (H + 1) / 2), outside the chroma plane: the border, without a special case.
          No quarter-pixel correction for left- or centre-sited chroma."""
import numpy as np

from oracle import meshflow_oracle as mo

F32 = np.float32
BORDER_RED = (81, 90, 240)          # BT.601 limited-range red: the reference's default BGR (0, 0, 255)


def chroma_maps(mx, my):
    """The chroma plane's float32 maps (H/2, W/2) from the luma frame's (H, W): the even luma pixels' values times 0.5f."""
    mx, my = np.asarray(mx, dtype=F32), np.asarray(my, dtype=F32)
    return (mx[::2, ::2] * F32(0.5)).astype(F32), (my[::2, ::2] * F32(0.5)).astype(F32)


def remap_luma(y, mx, my, border):
    y = np.asarray(y, dtype=np.uint8)
    return mo.remap_bilinear_u8c3(np.stack([y, y, y], axis=-1), mx, my, (border, border, border))[..., 0]


def remap_chroma(uv, cmx, cmy, border_uv):
    """The 8-bit remap of the two-channel plane uv (Hc, Wc, 2) at its own maps (cmx, cmy); border_uv = (U, V)."""
    uv = np.asarray(uv, dtype=np.uint8)
    three = np.stack([uv[..., 0], uv[..., 1], uv[..., 0]], axis=-1)
    return np.ascontiguousarray(mo.remap_bilinear_u8c3(three, cmx, cmy, (border_uv[0], border_uv[1], border_uv[0]))[..., :2])


def warp_frame(y, uv, mx, my, border_yuv=BORDER_RED):
    """(out_y, out_uv) of one NV12 frame under the luma frame's maps."""
    H, W = np.asarray(y).shape
    assert W % 2 == 0 and H % 2 == 0 and np.asarray(uv).shape == (H // 2, W // 2, 2)
    cmx, cmy = chroma_maps(mx, my)
    return remap_luma(y, mx, my, border_yuv[0]), remap_chroma(uv, cmx, cmy, border_yuv[1:3])


def tap_classes(cmx, cmy, Wc, Hc):
    """Which chroma samples (border, partly, deep) the maps produce: the 2 x 2 tap footprint wholly outside the (Hc, Wc) plane (unowned pixels
    among them), straddling its edge, and at least two pixels inside on every side (what the kernel's fast path requires)."""
    with np.errstate(over='ignore', invalid='ignore'):
        ix = mo._cv_round_f32(np.asarray(cmx, dtype=F32) * F32(32)) >> 5
        iy = mo._cv_round_f32(np.asarray(cmy, dtype=F32) * F32(32)) >> 5
    border = (ix >= Wc) | (ix + 1 < 0) | (iy >= Hc) | (iy + 1 < 0)
    partly = ~border & ((ix < 0) | (ix + 1 >= Wc) | (iy < 0) | (iy + 1 >= Hc))
    deep = (ix >= 2) & (ix <= Wc - 3) & (iy >= 2) & (iy <= Hc - 3)
    return border, partly, deep
