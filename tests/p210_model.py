"""NumPy models of the P210 calls (`ops.warp_p210`, `ops.crop_resize_p210`, `ops.unpack_y210` / `ops.pack_y210`), COMPOSED from the pinned
models of the two formats whose product P210 is -- nothing is restated here.  MODELLED on OpenCV 4.5-4.10 like every other format, NOT PINNED.

A P210 frame is a luma plane y (H, W) uint16 and an interleaved chroma plane uv (H, W/2, 2) uint16, U first; W is even, H of either parity;
samples are plain 16-bit numbers.

  warp    luma    `p010_model.remap_luma`
          chroma  `p010_model.remap_chroma(uv, *nv16_model.chroma_maps(mx, my), border_uv)` on the (H, W/2) plane: 4:2:2 siting, CV_16U blend
  crop    luma    `p010_crop_model.crop_resize_luma` (the float path, INTER_AREA's box at exactly 2x)
          chroma  x: `p010_crop_model.x_table`;  y: the 16-bit luma resize's own rows and fractions (`mo.resize_linear_tables(ch, oH)`, rows
                  clipped into the crop and offset by `top`, float32 weights (1 - f, f) kept, as `cv16_model.resize_linear_u16` has them);
                  blend: `p010_crop_model.blend`.  No area branch, also at exactly 2x.
  Y210    a packed frame (H, W, 2) uint16 holds Y in [..., 0] and U, V alternating in [..., 1]: slicing.

The keyword arguments of `crop_resize_chroma` switch on the MUTANTS tests/test_p210_model.py must reject; the model is the call without any."""
import numpy as np

import cv16_area
import nv12_crop_model as sites
import nv16_model
import p010_crop_model
import p010_model
from oracle import meshflow_oracle as mo

F32 = np.float32
chroma_maps = nv16_model.chroma_maps
tap_classes = nv16_model.tap_classes
remap_luma = p010_model.remap_luma
remap_chroma = p010_model.remap_chroma
x_table = p010_crop_model.x_table
crop_resize_luma = p010_crop_model.crop_resize_luma


def warp_frame(y, uv, mx, my, border_yuv):
    """(out_y, out_uv) of one P210 frame under the luma frame's maps."""
    H, W = np.asarray(y).shape
    assert W % 2 == 0 and np.asarray(uv).shape == (H, W // 2, 2)
    cmx, cmy = chroma_maps(mx, my)
    return remap_luma(y, mx, my, border_yuv[0]), remap_chroma(uv, cmx, cmy, border_yuv[1:3])


def y_table(top, bottom, oH):
    """(s0, s1, b0, b1): the two absolute plane rows of every output row and their float32 weights -- the 16-bit luma table's own."""
    ch = bottom - top + 1
    sy, fy = mo.resize_linear_tables(ch, oH)
    fy = fy.astype(F32)
    return top + np.clip(sy, 0, ch - 1), top + np.clip(sy + 1, 0, ch - 1), F32(1) - fy, fy


def x_classes(left, right, oW):
    """(low-clamped, high-clamped, interior) chroma columns of a case."""
    return sites.axis_classes(left, right, oW)


def y_classes(top, bottom, oH):
    """(low-clamped, high-clamped, interior) output rows: sy < 0; sy + 1 > ch - 1; anything else."""
    ch = bottom - top + 1
    sy, _ = mo.resize_linear_tables(ch, oH)
    low = sy < 0
    high = ~low & (sy + 1 > ch - 1)
    return int(low.sum()), int(high.sum()), int((~low & ~high).sum())


def crop_resize_chroma(uv, rect, size, halve_rows=False, forget_top=False, swap_uv=False, quantise_x=False, area_box=False, plane_range=False):
    """uv (H, Wc, 2) uint16 of a W x H luma frame -> (oH, oW/2, 2) uint16.  The keywords are the mutants."""
    left, top, right, bottom = (int(v) for v in rect)
    oW, oH = size
    S = np.asarray(uv, dtype=np.uint16)
    if area_box and cv16_area.is_area_fast(right - left + 1, bottom - top + 1, oW, oH) and left % 2 == 0 and (right - left + 1) % 4 == 0:
        return cv16_area.area_fast_u16(S[top:bottom + 1, left // 2:right // 2 + 1])       # (a box over the crop's chroma samples)
    if plane_range:
        s, f = sites.axis_positions(left, right, oW)
        c0, c1 = 0, S.shape[1] - 1
        low = s < c0
        s = np.where(low, c0, s); f = np.where(low, F32(0), f).astype(F32)
        high = s >= c1
        s = np.where(high, c1, s); f = np.where(high, F32(0), f).astype(F32)
        sx0, sx1, a0, a1 = s, np.minimum(s + 1, c1), F32(1) - f, f
    else:
        sx0, sx1, a0, a1 = x_table(left, right, oW)
    if quantise_x:
        q0, q1 = mo._coef(a1.astype(F32))
        a0, a1 = (q0 / F32(2048)).astype(F32), (q1 / F32(2048)).astype(F32)
    sy0, sy1, b0, b1 = y_table(top, bottom, oH)
    if halve_rows:
        sy0, sy1 = sy0 >> 1, sy1 >> 1
    if forget_top:
        sy0, sy1 = sy0 - top, sy1 - top
    if swap_uv:
        S = S[..., ::-1]
    return p010_crop_model.blend(S.astype(F32), sx0, sx1, a0, a1, sy0, sy1, b0, b1)


def crop_resize_frame(y, uv, rect, size=None):
    """(out_y, out_uv) of one P210 frame; size = (oW, oH), by default the frame's own."""
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


def unpack_y210(packed):
    """packed (..., H, W, 2) uint16, words Y0 U Y1 V -> (y (..., H, W), uv (..., H, W/2, 2)): slicing."""
    packed = np.asarray(packed, dtype=np.uint16)
    assert packed.shape[-1] == 2 and packed.shape[-2] % 2 == 0
    y = np.ascontiguousarray(packed[..., 0])
    uv = np.ascontiguousarray(packed[..., 1].reshape(packed.shape[:-2] + (packed.shape[-2] // 2, 2)))
    return y, uv


def pack_y210(y, uv):
    y, uv = np.asarray(y, dtype=np.uint16), np.asarray(uv, dtype=np.uint16)
    assert uv.shape == y.shape[:-1] + (y.shape[-1] // 2, 2)
    return np.ascontiguousarray(np.stack([y, uv.reshape(y.shape)], axis=-1))
