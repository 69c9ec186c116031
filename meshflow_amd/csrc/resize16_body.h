// Crop + bilinear resize of uint16 frames: _crop_frames (meshflowstabilizer.py:1111-1157, cv2.resize at :1150-1155) for CV_16UC3.
//
// cv2.resize INTER_LINEAR of 16-bit data (imgproc/resize.cpp: resizeGeneric_ with HResizeLinear<ushort, float, float, 1, ...> and
// VResizeLinear<ushort, float, float, Cast<float, ushort>, ...>) is the float path: the index and fraction tables are the 8-bit ones
// (resize_body.h), but the coefficients stay float32 (1 - f, f) -- no x2048, no rounding --, and
//   horizontal  t  = float(S[sx]) a0 + float(S[sx+1]) a1                  (float32, unfused)
//   vertical    out = saturate_cast<ushort>(t0 b0 + t1 b1)                (float32, unfused, rounded half to even)
// The one-tap branch of the horizontal pass (columns whose sx is the crop's last) gives S[sx] * 1 = S[sx] + S[sx+1] * 0: the same value.
// resize16_tables_kernel builds the tables on the device in the float / double operations of resize_tables_kernel, in the workspace
// mf_crop_resize_workspace_bytes(W, H) already sizes (8 bytes per column and per row); resize16_pixel: one thread per output pixel, a
// workgroup per 256 pixels of an output row, taps straight from the frame (two 12-byte loads per pixel where sx + 1 is inside the crop).
// Its kernels: resize16_kernel (the same size) and resize16_to_kernel (a caller-chosen oW x oH: cv2.resize(crop, (oW, oH))).
#ifndef MF_RESIZE16_BODY_H
#define MF_RESIZE16_BODY_H
#include "mf_common.h"
#include "resize_rect.h"

namespace mf {

__global__ __launch_bounds__(256) void resize16_tables_kernel(MF_TABLES_ARGS,
                                                              Resize16Tab* __restrict__ xtab, Resize16Tab* __restrict__ ytab)
{
    MF_TABLES_LOAD(W, H)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < W) {
        float fx = (float)(((double)i + 0.5) * scale_x - 0.5);
        int sx = (int)floorf(fx);
        fx -= (float)sx;
        if (sx < 0) { fx = 0.0f; sx = 0; }
        if (sx >= cw - 1) { fx = 0.0f; sx = cw - 1; }
        xtab[i].ofs = sx;
        xtab[i].f = fx;
    }
    if (i < H) {
        float fy = (float)(((double)i + 0.5) * scale_y - 0.5);
        const int sy = (int)floorf(fy);
        fy -= (float)sy;
        const int sy0 = min(max(sy, 0), ch - 1), sy1 = min(max(sy + 1, 0), ch - 1);
        ytab[i].ofs = sy0 | (sy1 << 16);
        ytab[i].f = fy;
    }
}

// One output pixel: source pitch W and frame W H apart from the output oW x oH (the tables are for (oW, oH)); the workgroup's tile is 256 pixels
// of one output row.  `area`: the crop is exactly twice the output in both axes (2 oW == cw and 2 oH == ch), where cv::hal::resize hands
// INTER_LINEAR to INTER_AREA's fast path (is_area_fast && iscale_x == 2 && iscale_y == 2), whose 16-bit form is
// (S00 + S01 + S10 + S11 + 2) >> 2 -- rounded half UP, where the float path would round the same quarter-sums half to even.  The tables there
// give sx = 2 dx, sy0 = 2 dy, sy1 = 2 dy + 1, so the four taps are the ones the float path reads.
__device__ __forceinline__ void resize16_pixel(const uint16_t* __restrict__ frames, uint16_t* __restrict__ out, int W, int H,
                                               int left, int top, int cw, int oW, int oH, bool area,
                                               const Resize16Tab* __restrict__ xtab, const Resize16Tab* __restrict__ ytab, const TileOrder& order)
{
    int f, y, tx;
    if (!order.decode(blockIdx.x, f, y, tx)) return;
    const int x = tx * 256 + (int)threadIdx.x;
    if (x >= oW) return;
    const uint64_t frame_samples = 3ull * (uint64_t)((uint32_t)W * (uint32_t)H);
    const uint64_t out_samples = 3ull * (uint64_t)((uint32_t)oW * (uint32_t)oH);
    const uint16_t* __restrict__ src = frames + (uint64_t)f * frame_samples;
    const Resize16Tab xt = xtab[x], yt = ytab[y];
    const float a1 = xt.f, a0 = 1.0f - xt.f, b1 = yt.f, b0 = 1.0f - yt.f;
    const uint32_t sx = (uint32_t)(left + xt.ofs);
    const uint16_t* __restrict__ p0 = src + 3ull * (uint64_t)((uint32_t)(top + (yt.ofs & 0xFFFF)) * (uint32_t)W + sx);
    const uint16_t* __restrict__ p1 = src + 3ull * (uint64_t)((uint32_t)(top + (yt.ofs >> 16)) * (uint32_t)W + sx);
    uint32_t s0[6], s1[6];                                       // B G R of columns sx and sx + 1, rows sy0 and sy1
    if (xt.ofs + 1 < cw) {
        uint32_t a[3], b[3];
        __builtin_memcpy(a, p0, 12);
        __builtin_memcpy(b, p1, 12);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            s0[2 * k] = a[k] & 0xFFFFu; s0[2 * k + 1] = a[k] >> 16;
            s1[2 * k] = b[k] & 0xFFFFu; s1[2 * k + 1] = b[k] >> 16;
        }
    } else {                                                     // the crop's last column: a1 = 0, nothing to its right is read
#pragma unroll
        for (int c = 0; c < 3; ++c) { s0[c] = s0[3 + c] = p0[c]; s1[c] = s1[3 + c] = p1[c]; }
    }
    uint16_t* __restrict__ d = out + (uint64_t)f * out_samples + 3ull * (uint64_t)((uint32_t)y * (uint32_t)oW + (uint32_t)x);
    uint32_t o[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (area) {
            o[c] = (s0[c] + s0[3 + c] + s1[c] + s1[3 + c] + 2u) >> 2;
        } else {
            const float t0 = (float)s0[c] * a0 + (float)s0[3 + c] * a1, t1 = (float)s1[c] * a0 + (float)s1[3 + c] * a1;
            o[c] = min((uint32_t)rintf(t0 * b0 + t1 * b1), 65535u);
        }
    }
    d[0] = (uint16_t)o[0];
    d[1] = (uint16_t)o[1];
    d[2] = (uint16_t)o[2];
}

// The kernels: the rectangle (launch arguments, or loaded from device memory: resize_rect.h), then the pixel.
// resize16_kernel (mf_crop_resize_u16c3): the frame's own size, where a crop inside the frame is never the exact 2x reduction
__global__ __launch_bounds__(256) void resize16_kernel(const uint16_t* __restrict__ frames, uint16_t* __restrict__ out, int W, int H,
                                                       MF_RECT_ARGS, const Resize16Tab* __restrict__ xtab,
                                                       const Resize16Tab* __restrict__ ytab, TileOrder order)
{
    MF_RECT_LOAD(W, H)
    resize16_pixel(frames, out, W, H, left, top, cw, W, H, false, xtab, ytab, order);
}

// resize16_to_kernel (mf_crop_resize_to_u16c3)
__global__ __launch_bounds__(256) void resize16_to_kernel(const uint16_t* __restrict__ frames, uint16_t* __restrict__ out, int W, int H,
                                                          MF_RECT16_TO_ARGS,
                                                          const Resize16Tab* __restrict__ xtab, const Resize16Tab* __restrict__ ytab,
                                                          TileOrder order)
{
    MF_RECT16_TO_LOAD(W, H)
    resize16_pixel(frames, out, W, H, left, top, cw, oW, oH, area, xtab, ytab, order);
}

}  // namespace mf

#endif  // MF_RESIZE16_BODY_H
