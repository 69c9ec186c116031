"""NumPy model of the NV12 crop-resize (`ops.crop_resize_nv12`, mf_crop_resize_nv12 / mf_crop_resize_dev_nv12), put together from
oracle/meshflow_oracle.py's 8-bit resize.  DEFINED by the project, MODELLED on cv2.resize like the NV12 warp's chroma, NOT PINNED: no cv2 was
run against it.

An NV12 frame is a luma plane y (H, W) uint8 and an interleaved chroma plane uv (H/2, W/2, 2) uint8, U first; W and H are even.  The rectangle
(left, top, right, bottom) is inclusive, in luma pixels, of any parity; the output size (oW, oH) is even.

  luma    `mo.resize_linear_u8` of the cropped plane: _crop_frames (mfs.py:1111-1157) on a single-channel frame.
  chroma  sited at the EVEN luma sample: output chroma sample cx sits on output luma pixel 2 cx; its source is that pixel's luma source position
          (`mo.resize_linear_tables`' expression), made absolute in the frame and halved:
              scale = 1 / (float(oW) / cw)
              fc = float32((left + ((2 cx + 0.5) scale - 0.5)) 0.5);  s = floor(fc);  f = fc - s       (float32)
              c1 = right >> 1,  c0 = min((left + 1) >> 1, c1)     the chroma samples whose siting luma pixel lies inside the crop
              x axis: s < c0 -> (c0, 0);  s >= c1 -> (c1, 0)      y axis: rows s and s + 1 clipped into [r0, r1], the weights kept
          weights `mo._coef`, then resize_linear_u8's two passes per channel.  No INTER_AREA special case; U and V never mix."""
import numpy as np

from oracle import meshflow_oracle as mo

F32 = np.float32


def axis_range(lo, hi):
    """(c0, c1): the chroma samples whose siting (even) luma pixel lies in lo .. hi; the single sample lo >> 1 for a one-pixel crop on an odd
    column."""
    c1 = hi >> 1
    return min((lo + 1) >> 1, c1), c1


def axis_positions(lo, hi, out_len):
    """(s, f) before any clamp for the out_len / 2 chroma samples of an axis: s int64, f float32."""
    cw = hi - lo + 1
    scale = 1.0 / (float(out_len) / float(cw))
    c = np.arange(out_len // 2, dtype=np.float64)
    fc = ((float(lo) + ((2.0 * c + 0.5) * scale - 0.5)) * 0.5).astype(F32)
    s = np.floor(fc).astype(np.int64)
    return s, (fc - s.astype(F32)).astype(F32)


def x_table(left, right, oW):
    """(s0, s1, a0, a1): the two absolute chroma columns of every output chroma column and their weights."""
    s, f = axis_positions(left, right, oW)
    c0, c1 = axis_range(left, right)
    low = s < c0
    s = np.where(low, c0, s); f = np.where(low, F32(0), f)
    high = s >= c1
    s = np.where(high, c1, s); f = np.where(high, F32(0), f)
    a0, a1 = mo._coef(f.astype(F32))
    return s, np.minimum(s + 1, c1), a0, a1            # (where s == c1 the second weight is 0)


def y_table(top, bottom, oH):
    """(s0, s1, b0, b1): the two absolute chroma rows of every output chroma row, clipped into [r0, r1], and their weights (kept)."""
    s, f = axis_positions(top, bottom, oH)
    r0, r1 = axis_range(top, bottom)
    b0, b1 = mo._coef(f)
    return np.clip(s, r0, r1), np.clip(s + 1, r0, r1), b0, b1


def axis_classes(lo, hi, out_len):
    """How many samples of the axis are (low-clamped, high-clamped, interior): s < c0, s >= c1 (no second tap inside), anything else."""
    s, _ = axis_positions(lo, hi, out_len)
    c0, c1 = axis_range(lo, hi)
    low = s < c0
    high = ~low & (s >= c1)
    return int(low.sum()), int(high.sum()), int((~low & ~high).sum())


def crop_resize_chroma(uv, rect, size):
    """uv (Hc, Wc, 2) uint8 of a W x H luma frame -> (oH/2, oW/2, 2) uint8."""
    left, top, right, bottom = (int(v) for v in rect)
    oW, oH = size
    sx0, sx1, a0, a1 = x_table(left, right, oW)
    sy0, sy1, b0, b1 = y_table(top, bottom, oH)
    S = np.asarray(uv, dtype=np.uint8).astype(np.int64)
    t0 = S[sy0][:, sx0] * a0[None, :, None] + S[sy0][:, sx1] * a1[None, :, None]
    t1 = S[sy1][:, sx0] * a0[None, :, None] + S[sy1][:, sx1] * a1[None, :, None]
    out = (((b0[:, None, None] * (t0 >> 4)) >> 16) + ((b1[:, None, None] * (t1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255                      # (each weight pair sums to 2048 +- 1: no saturation, resize_u8.h)
    return out.astype(np.uint8)


def crop_resize_luma(y, rect, size):
    left, top, right, bottom = (int(v) for v in rect)
    y = np.asarray(y, dtype=np.uint8)
    return mo.resize_linear_u8(y[top:bottom + 1, left:right + 1, None], size[0], size[1])[..., 0]


def crop_resize_frame(y, uv, rect, size=None):
    """(out_y, out_uv) of one NV12 frame; size = (oW, oH), by default the frame's own."""
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
