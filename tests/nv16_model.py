"""NumPy model of the NV16 warp and of packed 4:2:2 (`ops.warp_nv16`, `ops.unpack_422`, `ops.pack_422`), put together from tests/nv12_model.py's
pieces.  MODELLED on OpenCV 4.5-4.10 like every other format, NOT PINNED: no cv2 was run against it.

An NV16 frame is a luma plane y (H, W) uint8 and an interleaved chroma plane uv (H, W/2, 2) uint8, U first; W is even, H of either parity.
Given the warp's float32 maps (mx, my) of the luma frame (a pixel no cell owns holds (W + 1, H + 1)):

  luma    `nv12_model.remap_luma`: the grey warp.
  chroma  sited at the EVEN luma sample OF THE SAME ROW, by definition: output chroma sample (cx, y) takes the map of luma pixel (2 cx, y), x
          halved in float32 (u * 0.5f is exact), y as it is, and the (H, W/2) two-channel plane goes through `nv12_model.remap_chroma`, which
          does not care about the plane's shape.  An unowned pixel lands at ((W + 1) / 2, H + 1), outside the plane: the border, without a
          special case.  No sub-pixel correction for other chroma sitings.

Packed 4:2:2: (H, W, 2) uint8 (any leading axes), a flat stream of 4-byte words -- 'yuyv': Y0 U Y1 V, 'uyvy': U Y0 V Y1."""
import numpy as np

from nv12_model import BORDER_RED, remap_chroma, remap_luma, tap_classes  # noqa: F401  (shared, unchanged)

F32 = np.float32
ORDERS = ('yuyv', 'uyvy')


def chroma_maps(mx, my):
    """The chroma plane's float32 maps (H, W/2) from the luma frame's (H, W): the even luma columns, x times 0.5f, y as it is."""
    mx, my = np.asarray(mx, dtype=F32), np.asarray(my, dtype=F32)
    return (mx[..., ::2] * F32(0.5)).astype(F32), np.ascontiguousarray(my[..., ::2])


def warp_frame(y, uv, mx, my, border_yuv=BORDER_RED):
    """(out_y, out_uv) of one NV16 frame under the luma frame's maps."""
    H, W = np.asarray(y).shape
    assert W % 2 == 0 and np.asarray(uv).shape == (H, W // 2, 2)
    cmx, cmy = chroma_maps(mx, my)
    return remap_luma(y, mx, my, border_yuv[0]), remap_chroma(uv, cmx, cmy, border_yuv[1:3])


def unpack(packed, order):
    """(y, uv) of a packed (..., H, W, 2) array."""
    packed = np.asarray(packed, dtype=np.uint8)
    assert packed.shape[-1] == 2 and packed.shape[-2] % 2 == 0 and order in ORDERS
    lum, chr_ = (0, 1) if order == 'yuyv' else (1, 0)
    y = np.ascontiguousarray(packed[..., lum])
    c = packed[..., chr_]                                                # U at the even pixels, V at the odd ones
    uv = np.stack([c[..., 0::2], c[..., 1::2]], axis=-1)
    return y, np.ascontiguousarray(uv)


def pack(y, uv, order):
    """The packed (..., H, W, 2) array of the pair."""
    y, uv = np.asarray(y, dtype=np.uint8), np.asarray(uv, dtype=np.uint8)
    assert uv.shape == y.shape[:-1] + (y.shape[-1] // 2, 2) and y.shape[-1] % 2 == 0 and order in ORDERS
    lum, chr_ = (0, 1) if order == 'yuyv' else (1, 0)
    out = np.empty(y.shape + (2,), np.uint8)
    out[..., lum] = y
    out[..., 0::2, chr_] = uv[..., 0]
    out[..., 1::2, chr_] = uv[..., 1]
    return out
