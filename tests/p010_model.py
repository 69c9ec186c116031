"""NumPy model of the P010 warp (`ops.warp_p010`, mf_warp_p010), put together from tests/cv16_model.py's CV_16U remap and tests/nv12_model.py's
chroma siting.  MODELLED on OpenCV 4.5-4.10 like every other format, NOT PINNED: no cv2 was run against it.

A P010 frame is a luma plane y (H, W) uint16 and an interleaved chroma plane uv (H/2, W/2, 2) uint16, U first; W and H are even.  Samples are
plain 16-bit numbers (P010, P012 and P016 differ only in how many low bits a producer leaves zero); nothing is masked on the way out.  Given
the warp's float32 maps (mx, my) of the luma frame:

  luma    cv2.remap(y, mx, my, INTER_LINEAR, BORDER_CONSTANT, borderValue = border_yuv[0]) on CV_16UC1: the float32 chain of
          `cv16_model.remap_bilinear_u16c3` works per channel, so it is channel 0 of that function on the plane repeated three times.
  chroma  sited at the EVEN luma sample, as for NV12: `nv12_model.chroma_maps` (the even luma pixels' maps times 0.5f), then the same CV_16U
          remap of the (H/2, W/2) two-channel plane: `remap_bilinear_u16c3` of stack(U, V, U), channels 0 and 1, border (U, V, U)."""
import numpy as np

import cv16_model
import nv12_model
from nv12_model import chroma_maps, tap_classes  # noqa: F401  (the same maps and the same classes as for NV12)

BORDER_RED = tuple(v << 8 for v in nv12_model.BORDER_RED)       # BT.601 limited-range red at 10 bits, in P010's high bits


def remap_luma(y, mx, my, border):
    y = np.asarray(y, dtype=np.uint16)
    return np.ascontiguousarray(cv16_model.remap_bilinear_u16c3(np.stack([y, y, y], axis=-1), mx, my, (border, border, border))[..., 0])


def remap_chroma(uv, cmx, cmy, border_uv):
    """The CV_16U remap of the two-channel plane uv (Hc, Wc, 2) at its own maps (cmx, cmy); border_uv = (U, V)."""
    uv = np.asarray(uv, dtype=np.uint16)
    three = np.stack([uv[..., 0], uv[..., 1], uv[..., 0]], axis=-1)
    return np.ascontiguousarray(cv16_model.remap_bilinear_u16c3(three, cmx, cmy, (border_uv[0], border_uv[1], border_uv[0]))[..., :2])


def warp_frame(y, uv, mx, my, border_yuv=BORDER_RED):
    """(out_y, out_uv) of one P010 frame under the luma frame's maps."""
    H, W = np.asarray(y).shape
    assert W % 2 == 0 and H % 2 == 0 and np.asarray(uv).shape == (H // 2, W // 2, 2)
    cmx, cmy = chroma_maps(mx, my)
    return remap_luma(y, mx, my, border_yuv[0]), remap_chroma(uv, cmx, cmy, border_yuv[1:3])
