"""The exact-2x branch of cv2.resize INTER_LINEAR on uint16 frames, beside tests/cv16_model.py's float path.  MODELLED, NOT PINNED: no
OpenCV was at hand to check it against.

cv::hal::resize (imgproc/resize.cpp, OpenCV 4.5-4.10) turns INTER_LINEAR into INTER_AREA when both inverse scales are integers and equal
to 2 (`is_area_fast && iscale_x == 2 && iscale_y == 2`): the source is exactly twice the output in both axes.  INTER_AREA's fast path
(resizeAreaFast_ with ResizeAreaFastVec, fast_mode for scale 2 and 1, 3 or 4 channels) then computes per channel
  out = (S[2y][2x] + S[2y][2x+1] + S[2y+1][2x] + S[2y+1][2x+1] + 2) >> 2
in integers: rounded half UP.  The float path (cv16_model.resize_linear_u16) computes the same quarter-sum at f = 0.5 and rounds it half to
EVEN, so the two differ by one where the sum is 2 modulo 4 and sum / 4 rounds down to even.  For 8-bit data the fixed-point bilinear result
at f = 0.5 equals the area form, so only uint16 needs this.
  ASSUMED: the SIMD form of the 16-bit fast path (ResizeAreaFastVec_SIMD_16u) adds the same four samples and 2 and shifts by 2, as its scalar
  tail does; no IPP resize runs for this depth and interpolation."""
import numpy as np

import cv16_model


def is_area_fast(src_w, src_h, dst_w, dst_h):
    """True where cv::resize takes INTER_AREA's fast path for INTER_LINEAR: the source exactly twice the output in both axes."""
    return src_w == 2 * dst_w and src_h == 2 * dst_h


def area_fast_u16(src):
    """(S00 + S01 + S10 + S11 + 2) >> 2 over the 2 x 2 blocks of src (uint16, 2h x 2w x C or 2h x 2w)."""
    s = np.asarray(src, dtype=np.int64)
    sh, sw = s.shape[:2]
    if sh % 2 or sw % 2:
        raise ValueError('area_fast_u16: the source must be twice the output in both axes')
    q = s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]
    return ((q + 2) >> 2).astype(np.uint16)


def resize_u16(src, dst_w, dst_h):
    """cv2.resize(src uint16 HxWxC, (dst_w, dst_h)) with INTER_LINEAR, as modelled here and in cv16_model: the area branch at exactly 2x
    down in both axes, the float path everywhere else."""
    sh, sw = np.asarray(src).shape[:2]
    if is_area_fast(sw, sh, dst_w, dst_h):
        return area_fast_u16(src)
    return cv16_model.resize_linear_u16(src, dst_w, dst_h)
