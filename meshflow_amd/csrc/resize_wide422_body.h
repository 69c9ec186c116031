// Crop + resize of the interleaved chroma plane of a P210 / P212 / P216 (10-bit 4:2:2) clip: uv [n][H][W/2][2] uint16, U first, to out_uv
// [n][oH][oW/2][2] -- the chroma half of mf_crop_resize_p210 / mf_crop_resize_dev_p210 (the luma half is hdr_luma_resize_kernel as it is,
// resize_hdr_body.h).  W, H, oW, oH and the rectangle {left, top, right, bottom} (inclusive, any parity) are the LUMA frame's everywhere; W and
// oW are even, H and oH of either parity.  Samples are plain 16-bit numbers; nothing is masked.
//
// x axis: hdr_uv_tables_kernel's x half, the P010 definition (chroma_siting.h: column s clamped into c0 .. c1 and fraction f per output sample,
// kept as float32, weights (1 - f, f) as they are).  y axis: chroma has luma's rows, so output chroma row y takes the LUMA call's own
// Resize16Tab entry for row y -- rows top + sy0 and top + sy1 and the fraction f, as hdr_luma_resize_kernel reads them: no second y table,
// nothing halved.  Then blend16 per channel, U and V never mixing:
//   t = float(S[s]) a0 + float(S[s+1]) a1,   out = min(rint(t0 b0 + t1 b1), 65535)        (every product and sum rounded on its own)
// There is NO area branch: at exactly 2x down, where luma takes INTER_AREA's box, chroma still takes the float path on the luma table's entries
// (launch_resize16_tables writes them in every case) -- the NV16 rule (resize_uv422_body.h) restated for 16 bits.
// wide422_tables_kernel builds the oW/2 x entries on the device (absolute chroma columns), for the host rectangle too.  wide422_resize_kernel
// applies them with hdr_uv_resize_kernel's mapping and tap loads: a tap is one 4-byte word U | V << 16; a lane owns 4 consecutive chroma
// samples of a row (one 16-byte store, 4-byte stores at a row end), a wavefront 256 samples x kHdrRows rows, tiles counted over oH rows; taps
// straight from the plane, no LDS.  Where s < c1 the two taps of a row are ONE 8-byte load at 2-byte alignment; where s == c1 (f == 0) only
// that 4-byte sample is read, so nothing right of column c1 -- and never a byte behind the stack -- is touched.
// Bounds: a tile row y < oH reads ytab[y] of the oH luma entries; rows top + sy <= bottom < H; columns c0 .. c1 <= (W - 1) / 2 < W / 2;
// x entries min(x0 + j, oW/2 - 1); stores to samples x0 + j < oW/2 of row y < oH of frame f < n (the tile order's).
// The text stands beside resize_hdr_body.h's kernels instead of widening them: the six P010 kernels keep their listings that way.
// Device code only, written against resize_rect.h's macros: resize_hdr.hip compiles it with the rectangle as launch arguments,
// resize_hdr_dev.hip a second time under MF_RESIZE_DEV and other names, with the rectangle read from device memory.  An unusable device
// rectangle: both kernels return before they read or write anything, the luma y table included (the luma tables kernel has left it alone);
// *d_status is that kernel's to raise, once per call.
#ifndef MF_RESIZE_WIDE422_BODY_H
#define MF_RESIZE_WIDE422_BODY_H
#include "resize_hdr_body.h"

namespace mf {

// ofs = s (absolute chroma column, clamped into c0 .. c1), f = the float32 fraction -- hdr_uv_tables_kernel's x layout
__global__ __launch_bounds__(256) void wide422_tables_kernel(MF_UV_TABLES_ARGS, int oW, Resize16Tab* __restrict__ xtab)
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
        xtab[i].ofs = sx;
        xtab[i].f = fx;
    }
}

// xtab: wide422_tables_kernel's; ytab: the LUMA y table of the call (oH entries, rows relative to `top`)
__global__ __launch_bounds__(64 * kWaves) void wide422_resize_kernel(const uint16_t* __restrict__ uv, uint16_t* __restrict__ out, int W, int H,
                                                                     MF_RECT_ARGS, int oW, int oH, const Resize16Tab* __restrict__ xtab,
                                                                     const Resize16Tab* __restrict__ ytab, TileOrder order)
{
    MF_RECT_LOAD(W, H)
    int f, tile_y, tile_x;
    if (!order.decode(blockIdx.x, f, tile_y, tile_x)) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int CW = W >> 1, oCW = oW >> 1;
    const int ya = (tile_y * kWaves + wave) * kHdrRows;
    const int x0 = tile_x * 256 + lane * 4;
    if (ya >= oH || x0 >= oCW) return;
    const int c1 = (left + cw - 1) >> 1;                           // the crop's last chroma column: nothing to its right is read
    const uint16_t* __restrict__ src = uv + (uint64_t)f * (2ull * (uint64_t)((uint32_t)CW * (uint32_t)H));
    uint16_t* __restrict__ dst = out + (uint64_t)f * (2ull * (uint64_t)((uint32_t)oCW * (uint32_t)oH));
    uint32_t at[4];
    float a0[4], a1[4];
    bool two[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const Resize16Tab xt = xtab[min(x0 + j, oCW - 1)];
        at[j] = 2u * (uint32_t)xt.ofs;
        a1[j] = xt.f;
        a0[j] = 1.0f - xt.f;
        two[j] = xt.ofs < c1;
    }
#pragma unroll
    for (int q = 0; q < kHdrRows; ++q) {
        const int yo = ya + q;
        if (yo >= oH) break;
        const Resize16Tab yt = ytab[yo];
        const float b1 = yt.f, b0 = 1.0f - yt.f;
        const uint16_t* __restrict__ p0 = src + (uint32_t)(top + (yt.ofs & 0xFFFF)) * (uint32_t)CW * 2u;   // (a plane is below 2^30 samples)
        const uint16_t* __restrict__ p1 = src + (uint32_t)(top + (yt.ofs >> 16)) * (uint32_t)CW * 2u;
        uint32_t px[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint2 v0 = load_uv16_taps(p0, at[j], two[j]), v1 = load_uv16_taps(p1, at[j], two[j]);
            const uint32_t u = blend16(v0.x & 0xFFFFu, v0.y & 0xFFFFu, v1.x & 0xFFFFu, v1.y & 0xFFFFu, a0[j], a1[j], b0, b1);
            const uint32_t v = blend16(v0.x >> 16, v0.y >> 16, v1.x >> 16, v1.y >> 16, a0[j], a1[j], b0, b1);
            px[j] = u | (v << 16);
        }
        uint16_t* __restrict__ d = dst + ((uint32_t)yo * (uint32_t)oCW + (uint32_t)x0) * 2u;
        if (x0 + 3 < oCW) {
            const uint4 o = make_uint4(px[0], px[1], px[2], px[3]);
            __builtin_memcpy(__builtin_assume_aligned(d, 2), &o, 16);
        } else {                                                  // a row end of oW/2 % 4 != 0 samples
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (x0 + j < oCW) __builtin_memcpy(__builtin_assume_aligned(d + 2 * j, 2), &px[j], 4);
        }
    }
}

}  // namespace mf

#endif  // MF_RESIZE_WIDE422_BODY_H
