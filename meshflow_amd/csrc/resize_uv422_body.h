// Crop + resize of the interleaved chroma plane of an NV16 (4:2:2) clip: uv [n][H][W/2][2] uint8, U first, to out_uv [n][oH][oW/2][2] -- the
// chroma half of mf_crop_resize_nv16 / mf_crop_resize_dev_nv16 (the luma half is the u8c1 crop-resize as it is).  W, H, oW, oH and the rectangle
// {left, top, right, bottom} (inclusive, any parity) are the LUMA frame's everywhere; W and oW are even, H and oH of either parity.
//
// x axis: resize_uv_body.h's, the NV12 definition (chroma_siting.h: column s clamped into c0 .. c1 and fraction f per output sample, weights
// a0 = cvRound((1 - f) 2048), a1 = cvRound(f 2048)).  y axis: chroma has luma's rows, so output chroma row y takes the LUMA table's own entry
// for row y -- rows top + sy0 and top + sy1 (resize_tables_kernel's, already clipped into the crop) and its weights b0, b1: no second y table,
// nothing halved.  Then per channel, U and V never mixing,
//   horizontal  t   = S[s] a0 + S[s+1] a1
//   vertical    out = (((b0 (t0 >> 4)) >> 16) + ((b1 (t1 >> 4)) >> 16) + 2) >> 2
// uv422_tables_kernel builds the oW/2 x entries on the device (absolute chroma columns), for the host rectangle too.  uv422_resize_kernel
// applies them with chroma_resize_kernel's mapping: a lane owns 4 consecutive chroma samples of a row (one 8-byte store, 2-byte stores at a row
// end), a wavefront 256 samples x kUvRows rows, tiles counted over oH rows; taps straight from the plane, no LDS.  Where s < c1 the two taps of
// a row are ONE 4-byte load at 2-byte alignment (U0 V0 U1 V1), split by v_perm_b32 and blended by v_dot2_u32_u16 / v_mul_hi_u32_u24; where
// s == c1 (a1 == 0) only the 2-byte sample is read, so nothing right of column c1 -- and never a byte behind the stack -- is touched.
// The text stands beside resize_uv_body.h's instead of sharing a body with it: the four NV12 kernels keep their listings that way.
// Device code only, written against resize_rect.h's macros: resize_uv422.hip compiles it with the rectangle as launch arguments,
// resize_uv422_dev.hip a second time under MF_RESIZE_DEV and other names, with the rectangle read from device memory.  An unusable device
// rectangle: both kernels return before they read or write anything, the luma y table included (the luma tables kernel has left it alone);
// *d_status is that kernel's to raise, once per call.
#ifndef MF_RESIZE_UV422_BODY_H
#define MF_RESIZE_UV422_BODY_H
#include "mf_common.h"
#include "chroma_siting.h"
#include "resize_u8.h"
#include "resize_rect.h"

namespace mf {

constexpr int kUv422Rows = 4;         // output chroma rows per wavefront (resize_uv_body.h's kUvRows)

// ofs = s (absolute chroma column, clamped into c0 .. c1), w = 16 a0 | 16 a1 << 16 -- resize_tables_kernel's x layout
__global__ __launch_bounds__(256) void uv422_tables_kernel(MF_UV_TABLES_ARGS, int oW, ResizeTab* __restrict__ xtab)
{
    MF_UV_TABLES_LOAD
    (void)top; (void)rect_bottom; (void)ch;                       // (the y axis is the luma table's)
    const double scale_x = 1.0 / ((double)oW / (double)cw);
    int c0, c1;
    chroma_site_range(left, rect_right, c0, c1);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (oW >> 1)) {
        float fx;
        int sx;
        chroma_site_x(i, left, scale_x, c0, c1, sx, fx);
        const int a0 = (int)rintf((1.0f - fx) * 2048.0f), a1 = (int)rintf(fx * 2048.0f);
        xtab[i].ofs = sx;
        xtab[i].w = ((uint32_t)a0 << 4) | ((uint32_t)a1 << 20);
    }
}

// U0 | V0 << 8 | U1 << 16 | V1 << 24 of samples s and s + 1 at p (two), or U0 | V0 << 8 of sample s alone
__device__ __forceinline__ uint32_t load_uv422_taps(const uint8_t* __restrict__ p, bool two)
{
    uint32_t v;
    if (two) __builtin_memcpy(&v, __builtin_assume_aligned(p, 2), 4);
    else v = *reinterpret_cast<const uint16_t*>(p);
    return v;
}

// xtab: uv422_tables_kernel's; ytab: the LUMA y table of the call (oH entries, rows relative to `top`)
__global__ __launch_bounds__(64 * kWaves) void uv422_resize_kernel(const uint8_t* __restrict__ uv, uint8_t* __restrict__ out, int W, int H,
                                                                   MF_RECT_ARGS, int oW, int oH, const ResizeTab* __restrict__ xtab,
                                                                   const ResizeTab* __restrict__ ytab, TileOrder order)
{
    MF_RECT_LOAD(W, H)
    int f, tile_y, tile_x;
    if (!order.decode(blockIdx.x, f, tile_y, tile_x)) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int CW = W >> 1, oCW = oW >> 1;
    const int ya = (tile_y * kWaves + wave) * kUv422Rows;
    const int x0 = tile_x * 256 + lane * 4;
    if (ya >= oH || x0 >= oCW) return;
    const int c1 = (left + cw - 1) >> 1;                           // the crop's last chroma column: nothing to its right is read
    const uint8_t* __restrict__ src = uv + (uint64_t)f * (2ull * (uint64_t)((uint32_t)CW * (uint32_t)H));
    uint8_t* __restrict__ dst = out + (uint64_t)f * (2ull * (uint64_t)((uint32_t)oCW * (uint32_t)oH));
    uint32_t at[4], w[4];
    bool two[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const ResizeTab xt = xtab[min(x0 + j, oCW - 1)];
        at[j] = 2u * (uint32_t)xt.ofs;
        w[j] = xt.w;
        two[j] = xt.ofs < c1;
    }
#pragma unroll
    for (int q = 0; q < kUv422Rows; ++q) {
        const int y = ya + q;
        if (y >= oH) break;
        const ResizeTab yt = ytab[y];
        const uint32_t b0s = (yt.w & 0xFFFFu) << 8, b1s = (yt.w >> 16) << 8;
        const uint8_t* __restrict__ p0 = src + (uint32_t)(top + (yt.ofs & 0xFFFF)) * (uint32_t)CW * 2u;   // (a plane is below 2^30 bytes)
        const uint8_t* __restrict__ p1 = src + (uint32_t)(top + (yt.ofs >> 16)) * (uint32_t)CW * 2u;
        uint32_t px[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t v0 = load_uv422_taps(p0 + at[j], two[j]), v1 = load_uv422_taps(p1 + at[j], two[j]);
            const uint32_t U0 = udot2(__builtin_amdgcn_perm(0u, v0, 0x0C020C00u), w[j], 0u) & ~255u;
            const uint32_t U1 = udot2(__builtin_amdgcn_perm(0u, v1, 0x0C020C00u), w[j], 0u) & ~255u;
            const uint32_t V0 = udot2(__builtin_amdgcn_perm(0u, v0, 0x0C030C01u), w[j], 0u) & ~255u;
            const uint32_t V1 = udot2(__builtin_amdgcn_perm(0u, v1, 0x0C030C01u), w[j], 0u) & ~255u;
            const uint32_t u = (mulhi_u24(b0s, U0) + mulhi_u24(b1s, U1) + 2u) >> 2;
            const uint32_t v = (mulhi_u24(b0s, V0) + mulhi_u24(b1s, V1) + 2u) >> 2;
            px[j] = u | (v << 8);
        }
        uint8_t* __restrict__ d = dst + ((uint32_t)y * (uint32_t)oCW + (uint32_t)x0) * 2u;
        if (x0 + 3 < oCW) {
            uint2 o;
            o.x = px[0] | (px[1] << 16);
            o.y = px[2] | (px[3] << 16);
            __builtin_memcpy(__builtin_assume_aligned(d, 2), &o, 8);
        } else {                                                  // a row end of oW/2 % 4 != 0 samples
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (x0 + j < oCW) reinterpret_cast<uint16_t*>(d)[j] = (uint16_t)px[j];
        }
    }
}

}  // namespace mf

#endif  // MF_RESIZE_UV422_BODY_H
