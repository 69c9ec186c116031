// Where a crop-resize kernel gets its rectangle from.  The kernel headers (resize_body.h, resize16_body.h, resize_c1_body.h, resize_c4_body.h)
// are written against these macros, and only their kernel entries: a __global__ loads the rectangle and hands plain left, top, cw to the
// format's tile function, which is the same text in both flavours.  Included from resize.hip, resize16.hip, resize_c1.hip and
// resize_c4.hip, their kernels take `left, top, cw` as launch arguments (MF_RECT_ARGS) -- the host knows the rectangle.  The translation
// unit of the device-rectangle calls (mf_crop_resize_dev_*: resize_dev.hip) defines MF_RESIZE_DEV, renames the kernels and includes the
// same headers: MF_RECT_ARGS is then a pointer to {left, top, right, bottom} in device memory and MF_RECT_LOAD, the first statement of
// every kernel entry, reads it (four uniform dwords: one scalar 16-byte load per wavefront) and RETURNS if the rectangle cannot be used,
// before the kernel has read a frame byte or written an output byte.  Without MF_RESIZE_DEV both macros expand to launch arguments and to
// nothing.
#pragma once
#include "mf_common.h"

#ifdef MF_RESIZE_DEV
namespace mf {
// the device twin of resize_rect_ok (resize_checks.h): an empty rectangle or one that leaves the W x H frame
__device__ __forceinline__ bool rect_usable(int left, int top, int right, int bottom, int W, int H)
{
    return left >= 0 && top >= 0 && right < W && bottom < H && right >= left && bottom >= top;
}
}  // namespace mf
#define MF_RECT_ARGS const int32_t* __restrict__ d_bounds
#define MF_RECT_LOAD(W, H)                                                                                              \
    const int left = d_bounds[0], top = d_bounds[1], rect_right = d_bounds[2], rect_bottom = d_bounds[3];               \
    if (!rect_usable(left, top, rect_right, rect_bottom, W, H)) return;                                                 \
    const int cw = rect_right - left + 1;                                                                               \
    [[maybe_unused]] const int ch = rect_bottom - top + 1;
// resize16_to_kernel: the exact-2x INTER_AREA branch is a wavefront-uniform branch on the loaded rectangle
#define MF_RECT16_TO_ARGS const int32_t* __restrict__ d_bounds, int oW, int oH
#define MF_RECT16_TO_LOAD(W, H) MF_RECT_LOAD(W, H) const bool area = 2 * oW == cw && 2 * oH == ch;
// the tables kernels (W x H: the OUTPUT size, frame_W x frame_H the frames'): the crop's size and the two scales in the float64 operations
// of launch_resize_tables_to (the build is -ffp-contract=off and float64 division is IEEE: the same bits); an unusable rectangle adds 1 to
// *d_status (one lane, a vector atomic) and leaves the tables alone
#define MF_TABLES_ARGS const int32_t* __restrict__ d_bounds, int frame_W, int frame_H, int W, int H, int32_t* __restrict__ d_status
#define MF_TABLES_LOAD(W, H)                                                                                            \
    const int left = d_bounds[0], top = d_bounds[1], rect_right = d_bounds[2], rect_bottom = d_bounds[3];               \
    if (!rect_usable(left, top, rect_right, rect_bottom, frame_W, frame_H)) {                                           \
        if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(d_status, 1);                                                \
        return;                                                                                                         \
    }                                                                                                                   \
    const int cw = rect_right - left + 1, ch = rect_bottom - top + 1;                                                   \
    const double scale_x = 1.0 / ((double)(W) / (double)cw), scale_y = 1.0 / ((double)(H) / (double)ch);
// the chroma tables kernels (resize_uv_body.h, resize_hdr_body.h) need all four edges (MF_RECT_ARGS carries left, top, cw only); they raise no
// status: the luma tables kernel in front of them has
#define MF_UV_TABLES_ARGS const int32_t* __restrict__ d_bounds, int frame_W, int frame_H
#define MF_UV_TABLES_LOAD MF_RECT_LOAD(frame_W, frame_H)
#else
#define MF_RECT_ARGS int left, int top, int cw
#define MF_RECT_LOAD(W, H)
#define MF_RECT16_TO_ARGS int left, int top, int cw, int oW, int oH, bool area
#define MF_RECT16_TO_LOAD(W, H)
#define MF_TABLES_ARGS int cw, int ch, int W, int H, double scale_x, double scale_y
#define MF_TABLES_LOAD(W, H)
#define MF_UV_TABLES_ARGS int left, int top, int rect_right, int rect_bottom
#define MF_UV_TABLES_LOAD const int cw = rect_right - left + 1, ch = rect_bottom - top + 1;
#endif
