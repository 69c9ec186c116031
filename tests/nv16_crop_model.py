"""NumPy model of the NV16 crop-resize (`ops.crop_resize_nv16`, mf_crop_resize_nv16 / mf_crop_resize_dev_nv16), put together from
oracle/meshflow_oracle.py's 8-bit resize and tests/nv12_crop_model.py's x axis.  DEFINED by the project, MODELLED on cv2.resize like the NV12
crop's chroma, NOT PINNED: no cv2 was run against it.

An NV16 frame is a luma plane y (H, W) uint8 and an interleaved chroma plane uv (H, W/2, 2) uint8, U first; W is even, H of either parity.
The rectangle (left, top, right, bottom) is inclusive, in luma pixels, of any parity; of the output size (oW, oH) only oW is even.

  luma    `mo.resize_linear_u8` of the cropped plane: _crop_frames (mfs.py:1111-1157) on a single-channel frame.
  chroma  x axis: `nv12_crop_model.x_table` -- the NV12 definition, imported, not copied: sited at the even luma sample, absolute chroma
          columns clamped into c0 .. c1 with fraction 0 where clamped.
          y axis: chroma has luma's rows, so output chroma row y takes the LUMA table's entry for row y (`mo.resize_linear_tables(ch, oH)`):
          rows top + clip(sy, 0, ch - 1) and top + clip(sy + 1, 0, ch - 1), weights `mo._coef(fy)`, kept where a row was clipped.  No second
          y table, nothing halved.
          then resize_linear_u8's two passes per channel.  No INTER_AREA special case; U and V never mix.

The keyword arguments of `crop_resize_chroma` switch on the MUTANTS tests/test_nv16_crop_model.py must reject; the model is the call without any."""
import numpy as np

import nv12_crop_model as nv12
from oracle import meshflow_oracle as mo

axis_range = nv12.axis_range
x_table = nv12.x_table


def y_table(top, bottom, oH):
    """(s0, s1, b0, b1): the two absolute plane rows of every output row and their weights -- the luma table's own, offset by `top`."""
    ch = bottom - top + 1
    sy, fy = mo.resize_linear_tables(ch, oH)
    b0, b1 = mo._coef(fy)
    return top + np.clip(sy, 0, ch - 1), top + np.clip(sy + 1, 0, ch - 1), b0, b1


def x_classes(left, right, oW):
    """(low-clamped, high-clamped, interior) chroma columns of a case: nv12_crop_model.axis_classes, the x axis being the NV12 one."""
    return nv12.axis_classes(left, right, oW)


def y_classes(top, bottom, oH):
    """(low-clamped, high-clamped, interior) output rows: sy < 0; sy + 1 > ch - 1 (no second row inside the crop); anything else."""
    ch = bottom - top + 1
    sy, _ = mo.resize_linear_tables(ch, oH)
    low = sy < 0
    high = ~low & (sy + 1 > ch - 1)
    return int(low.sum()), int(high.sum()), int((~low & ~high).sum())


def crop_resize_chroma(uv, rect, size, halve_rows=False, forget_top=False, plane_range=False, swap_uv=False):
    """uv (H, Wc, 2) uint8 of a W x H luma frame -> (oH, oW/2, 2) uint8.  The keywords are the mutants: row indices halved as for a 4:2:0
    plane, rows not offset by `top`, c0 / c1 taken from the plane instead of the crop, U and V
    swapped."""
    left, top, right, bottom = (int(v) for v in rect)
    oW, oH = size
    S = np.asarray(uv, dtype=np.uint8).astype(np.int64)
    if plane_range:
        s, f = nv12.axis_positions(left, right, oW)
        c0, c1 = 0, S.shape[1] - 1
        low = s < c0
        s = np.where(low, c0, s); f = np.where(low, np.float32(0), f)
        high = s >= c1
        s = np.where(high, c1, s); f = np.where(high, np.float32(0), f)
        a0, a1 = mo._coef(f.astype(np.float32))
        sx0, sx1 = s, np.minimum(s + 1, c1)
    else:
        sx0, sx1, a0, a1 = x_table(left, right, oW)
    sy0, sy1, b0, b1 = y_table(top, bottom, oH)
    if halve_rows:
        sy0, sy1 = sy0 >> 1, sy1 >> 1
    if forget_top:
        sy0, sy1 = sy0 - top, sy1 - top
    if swap_uv:
        S = S[..., ::-1]
    t0 = S[sy0][:, sx0] * a0[None, :, None] + S[sy0][:, sx1] * a1[None, :, None]
    t1 = S[sy1][:, sx0] * a0[None, :, None] + S[sy1][:, sx1] * a1[None, :, None]
    out = (((b0[:, None, None] * (t0 >> 4)) >> 16) + ((b1[:, None, None] * (t1 >> 4)) >> 16) + 2) >> 2
    assert out.min() >= 0 and out.max() <= 255                      # (each weight pair sums to 2048 +- 1: no saturation, resize_u8.h)
    return out.astype(np.uint8)


crop_resize_luma = nv12.crop_resize_luma


def crop_resize_frame(y, uv, rect, size=None):
    """(out_y, out_uv) of one NV16 frame; size = (oW, oH), by default the frame's own."""
    H, W = np.asarray(y).shape
    assert W % 2 == 0 and np.asarray(uv).shape == (H, W // 2, 2)
    left, top, right, bottom = (int(v) for v in rect)
    assert 0 <= left <= right < W and 0 <= top <= bottom < H
    size = (W, H) if size is None else (int(size[0]), int(size[1]))
    assert size[0] % 2 == 0 and size[0] >= 2 and size[1] >= 2
    return crop_resize_luma(y, rect, size), crop_resize_chroma(uv, rect, size)


def crop_resize_clip(y, uv, rect, size=None):
    outs = [crop_resize_frame(y[f], uv[f], rect, size) for f in range(len(y))]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
