"""NumPy model of the P010 crop-resize (`ops.crop_resize_p010`, mf_crop_resize_p010 / mf_crop_resize_dev_p010), put together from
tests/cv16_model.py / tests/cv16_area.py (cv2.resize of 16-bit data) and tests/nv12_crop_model.py (where 4:2:0 chroma sits).  DEFINED by the
project, MODELLED on cv2.resize (OpenCV 4.5-4.10), NOT PINNED: no cv2 was run against it.

A P010 frame is a luma plane y (H, W) uint16 and an interleaved chroma plane uv (H/2, W/2, 2) uint16, U first; W and H are even; samples are
plain 16-bit numbers.  The rectangle (left, top, right, bottom) is inclusive, in luma pixels, of any parity; the output size (oW, oH) is even.

  luma    `cv16_area.resize_u16` of the cropped plane: the float path, and INTER_AREA's (S00 + S01 + S10 + S11 + 2) >> 2 where the crop is
          exactly twice the output in both axes.
  chroma  sited at the EVEN luma sample: `nv12_crop_model.axis_positions` / `axis_range` give (s, f) and the clamp range of each axis -- x:
          s < c0 -> (c0, 0), s >= c1 -> (c1, 0); y: rows s and s + 1 clipped into [r0, r1], f kept --, then the float32 two-pass per channel
          with the weights (1 - f, f) as they are: t = S[s] a0 + S[s+1] a1, out = min(rint(t0 b0 + t1 b1), 65535), every product and sum
          rounded to float32 on its own.  No 2048 quantisation, no INTER_AREA special case; U and V never mix."""
import numpy as np

import cv16_area
import nv12_crop_model as sites

F32 = np.float32


def x_table(left, right, oW):
    """(s0, s1, a0, a1): the two absolute chroma columns of every output chroma column and their float32 weights."""
    s, f = sites.axis_positions(left, right, oW)
    c0, c1 = sites.axis_range(left, right)
    low = s < c0
    s = np.where(low, c0, s); f = np.where(low, F32(0), f).astype(F32)
    high = s >= c1
    s = np.where(high, c1, s); f = np.where(high, F32(0), f).astype(F32)
    return s, np.minimum(s + 1, c1), F32(1) - f, f          # (where s == c1 the second weight is 0)


def y_table(top, bottom, oH):
    """(s0, s1, b0, b1): the two absolute chroma rows of every output chroma row, clipped into [r0, r1], and their weights (kept)."""
    s, f = sites.axis_positions(top, bottom, oH)
    r0, r1 = sites.axis_range(top, bottom)
    f = f.astype(F32)
    return np.clip(s, r0, r1), np.clip(s + 1, r0, r1), F32(1) - f, f


def blend(S, sx0, sx1, a0, a1, sy0, sy1, b0, b1):
    """The float32 two-pass on S (rows, columns, channels) float32: each product and sum rounded on its own (NumPy float32 arithmetic)."""
    assert S.dtype == F32 and a0.dtype == F32 and a1.dtype == F32 and b0.dtype == F32 and b1.dtype == F32
    t0 = S[sy0][:, sx0] * a0[None, :, None] + S[sy0][:, sx1] * a1[None, :, None]
    t1 = S[sy1][:, sx0] * a0[None, :, None] + S[sy1][:, sx1] * a1[None, :, None]
    t = t0 * b0[:, None, None] + t1 * b1[:, None, None]
    assert t.dtype == F32
    return np.clip(np.rint(t), 0, 65535).astype(np.uint16)


def crop_resize_chroma(uv, rect, size):
    """uv (Hc, Wc, 2) uint16 of a W x H luma frame -> (oH/2, oW/2, 2) uint16."""
    left, top, right, bottom = (int(v) for v in rect)
    oW, oH = size
    return blend(np.asarray(uv, dtype=np.uint16).astype(F32), *x_table(left, right, oW), *y_table(top, bottom, oH))


def crop_resize_luma(y, rect, size):
    left, top, right, bottom = (int(v) for v in rect)
    y = np.asarray(y, dtype=np.uint16)
    return cv16_area.resize_u16(y[top:bottom + 1, left:right + 1, None], size[0], size[1])[..., 0]


def crop_resize_frame(y, uv, rect, size=None):
    """(out_y, out_uv) of one P010 frame; size = (oW, oH), by default the frame's own."""
    H, W = np.asarray(y).shape
    assert W % 2 == 0 and H % 2 == 0 and np.asarray(uv).shape == (H // 2, W // 2, 2)
    left, top, right, bottom = (int(v) for v in rect)
    assert 0 <= left <= right < W and 0 <= top <= bottom < H
    size = (W, H) if size is None else (int(size[0]), int(size[1]))
    assert size[0] % 2 == 0 and size[1] % 2 == 0 and size[0] >= 2 and size[1] >= 2
    return crop_resize_luma(y, rect, size), crop_resize_chroma(uv, rect, size)


def crop_resize_clip(y, uv, rect, size=None):
    outs = [crop_resize_frame(y[f], uv[f], rect, size) for f in range(len(y))]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
