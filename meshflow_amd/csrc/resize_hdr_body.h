// Crop + resize of a P010 clip (mf_crop_resize_p010 / mf_crop_resize_dev_p010): y [n][H][W] uint16 to out_y [n][oH][oW] and the interleaved chroma
// plane uv [n][H/2][W/2][2] uint16, U first, to out_uv [n][oH/2][oW/2][2].  W, H, oW, oH and the rectangle {left, top, right, bottom}
// (inclusive, any parity) are the LUMA frame's everywhere.  Samples are plain 16-bit numbers; nothing is masked.
//
// Luma is channel 0 of resize16_to_kernel (resize16_body.h) on stack(Y, Y, Y), bit for bit: cv2.resize INTER_LINEAR of CV_16UC1 -- the tables
// are resize16_tables_kernel's for (oW, oH) (resize16_body.h; launched by the units that own that kernel), float32 weights (1 - f, f),
//   t = float(S[sx]) a0 + float(S[sx+1]) a1,   out = min(rint(t0 b0 + t1 b1), 65535)        (every product and sum rounded on its own)
// and, where the crop is exactly twice the output in both axes (`area`, uniform per launch), INTER_AREA's (S00 + S01 + S10 + S11 + 2) >> 2.
// hdr_luma_resize_kernel: a lane owns 4 consecutive output samples of a row (one 8-byte store), a wavefront 256 samples x kHdrRows rows;
// where sx + 1 < cw a sample's two taps of a row are ONE 4-byte load at 2-byte alignment, on the crop's last column only the 2-byte sample
// is read (a1 = 0 there).
//
// Chroma is sited at the even luma sample (chroma_siting.h has the positions and clamps: column s and fraction f per output sample) and takes
// the 16-bit float arithmetic above per channel with the weights (1 - f, f) as they are: no 2048 quantisation, and NO area branch (at
// exactly 2x down an even `left` gives f = 0.25, not a box).  U and V never mix.  hdr_uv_tables_kernel builds the oW/2 + oH/2 Resize16Tab
// entries on the device, for the host rectangle too (x: ofs = the ABSOLUTE clamped chroma column, f;  y: ofs = sy0 | sy1 << 16, absolute rows,
// f).  hdr_uv_resize_kernel: a tap is one 4-byte word U | V << 16; a lane owns 4 consecutive chroma samples of a row (one 16-byte store), a
// wavefront 256 samples x kHdrRows rows; taps straight from the plane, no LDS.  Where s + 1 <= c1 the two taps of a row are ONE 8-byte load at
// 2-byte alignment; where s == c1 (f == 0) only that 4-byte sample is read, so nothing right of column c1 -- and never a byte behind the
// stack -- is touched.
// Device code only, written against resize_rect.h's macros: resize_hdr.hip compiles it with the rectangle as launch arguments,
// resize_hdr_dev.hip a second time under MF_RESIZE_DEV and other names, with the rectangle read from device memory.  An unusable device
// rectangle: all three kernels return before they read or write anything; *d_status is the luma tables kernel's to raise, once per call.
#ifndef MF_RESIZE_HDR_BODY_H
#define MF_RESIZE_HDR_BODY_H
#include "mf_common.h"
#include "chroma_siting.h"
#include "resize_u8.h"
#include "resize_rect.h"

namespace mf {

constexpr int kHdrRows = 4;           // output rows per wavefront, luma and chroma

// the float path of one sample: taps s00 s01 of the first row, s10 s11 of the second
__device__ __forceinline__ uint32_t blend16(uint32_t s00, uint32_t s01, uint32_t s10, uint32_t s11, float a0, float a1, float b0, float b1)
{
    const float t0 = (float)s00 * a0 + (float)s01 * a1, t1 = (float)s10 * a0 + (float)s11 * a1;
    return min((uint32_t)rintf(t0 * b0 + t1 * b1), 65535u);
}

// S[sx] | S[sx+1] << 16 at p (two), or the sample at p in both halves
__device__ __forceinline__ uint32_t load_y16_taps(const uint16_t* __restrict__ p, bool two)
{
    uint32_t v;
    if (two) __builtin_memcpy(&v, __builtin_assume_aligned(p, 2), 4);
    else v = (uint32_t)*p * 0x10001u;
    return v;
}

__global__ __launch_bounds__(64 * kWaves) void hdr_luma_resize_kernel(const uint16_t* __restrict__ y, uint16_t* __restrict__ out, int W, int H,
                                                                      MF_RECT16_TO_ARGS, const Resize16Tab* __restrict__ xtab,
                                                                      const Resize16Tab* __restrict__ ytab, TileOrder order)
{
    MF_RECT16_TO_LOAD(W, H)
    int f, tile_y, tile_x;
    if (!order.decode(blockIdx.x, f, tile_y, tile_x)) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int ya = (tile_y * kWaves + wave) * kHdrRows;
    const int x0 = tile_x * 256 + lane * 4;
    if (ya >= oH || x0 >= oW) return;
    const uint16_t* __restrict__ src = y + (uint64_t)f * (uint64_t)((uint32_t)W * (uint32_t)H);
    uint16_t* __restrict__ dst = out + (uint64_t)f * (uint64_t)((uint32_t)oW * (uint32_t)oH);
    uint32_t at[4];
    float a0[4], a1[4];
    bool two[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const Resize16Tab xt = xtab[min(x0 + j, oW - 1)];
        at[j] = (uint32_t)(left + xt.ofs);
        a1[j] = xt.f;
        a0[j] = 1.0f - xt.f;
        two[j] = xt.ofs + 1 < cw;                                 // the crop's last column: a1 = 0, nothing to its right is read
    }
#pragma unroll
    for (int q = 0; q < kHdrRows; ++q) {
        const int yo = ya + q;
        if (yo >= oH) break;
        const Resize16Tab yt = ytab[yo];
        const float b1 = yt.f, b0 = 1.0f - yt.f;
        const uint16_t* __restrict__ p0 = src + (uint32_t)(top + (yt.ofs & 0xFFFF)) * (uint32_t)W;       // (a plane is below 2^30 samples)
        const uint16_t* __restrict__ p1 = src + (uint32_t)(top + (yt.ofs >> 16)) * (uint32_t)W;
        uint32_t px[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t v0 = load_y16_taps(p0 + at[j], two[j]), v1 = load_y16_taps(p1 + at[j], two[j]);
            if (area) px[j] = ((v0 & 0xFFFFu) + (v0 >> 16) + (v1 & 0xFFFFu) + (v1 >> 16) + 2u) >> 2;
            else px[j] = blend16(v0 & 0xFFFFu, v0 >> 16, v1 & 0xFFFFu, v1 >> 16, a0[j], a1[j], b0, b1);
        }
        uint16_t* __restrict__ d = dst + ((uint32_t)yo * (uint32_t)oW + (uint32_t)x0);
        if (x0 + 3 < oW) {
            uint2 o;
            o.x = px[0] | (px[1] << 16);
            o.y = px[2] | (px[3] << 16);
            __builtin_memcpy(__builtin_assume_aligned(d, 2), &o, 8);
        } else {                                                  // a row end of oW % 4 != 0 samples
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (x0 + j < oW) d[j] = (uint16_t)px[j];
        }
    }
}

// chroma_siting.h's positions with the fractions kept as float32
__global__ __launch_bounds__(256) void hdr_uv_tables_kernel(MF_UV_TABLES_ARGS, int oW, int oH, Resize16Tab* __restrict__ xtab,
                                                            Resize16Tab* __restrict__ ytab)
{
    MF_UV_TABLES_LOAD
    const double scale_x = 1.0 / ((double)oW / (double)cw), scale_y = 1.0 / ((double)oH / (double)ch);
    int c0, c1, r0, r1;
    chroma_site_range(left, rect_right, c0, c1);
    chroma_site_range(top, rect_bottom, r0, r1);
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (oW >> 1)) {
        float fx;
        int sx;
        chroma_site_x(i, left, scale_x, c0, c1, sx, fx);
        xtab[i].ofs = sx;
        xtab[i].f = fx;
    }
    if (i < (oH >> 1)) {
        float fy;
        int sy;
        chroma_site(i, top, scale_y, sy, fy);
        ytab[i].ofs = chroma_site_rows(sy, r0, r1);
        ytab[i].f = fy;
    }
}

// the words U | V << 16 of chroma samples s and s + 1 at row[at] (two), or the word of sample s in both
__device__ __forceinline__ uint2 load_uv16_taps(const uint16_t* __restrict__ row, uint32_t at, bool two)
{
    uint2 v;
    if (two) {
        asm("" : "+v"(at));                                      // (its own offset: the compiler would otherwise share the first word's load
                                                                  // with the other branch and fetch the second word on its own)
        __builtin_memcpy(&v, __builtin_assume_aligned(row + at, 2), 8);
    } else {
        __builtin_memcpy(&v.x, __builtin_assume_aligned(row + at, 2), 4);
        v.y = v.x;
    }
    return v;
}

__global__ __launch_bounds__(64 * kWaves) void hdr_uv_resize_kernel(const uint16_t* __restrict__ uv, uint16_t* __restrict__ out, int W, int H,
                                                                    MF_RECT_ARGS, int oW, int oH, const Resize16Tab* __restrict__ xtab,
                                                                    const Resize16Tab* __restrict__ ytab, TileOrder order)
{
    MF_RECT_LOAD(W, H)
    (void)top;                                                    // (the tables hold absolute rows)
    int f, tile_y, tile_x;
    if (!order.decode(blockIdx.x, f, tile_y, tile_x)) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int CW = W >> 1, CH = H >> 1, oCW = oW >> 1, oCH = oH >> 1;
    const int ya = (tile_y * kWaves + wave) * kHdrRows;
    const int x0 = tile_x * 256 + lane * 4;
    if (ya >= oCH || x0 >= oCW) return;
    const int c1 = (left + cw - 1) >> 1;                           // the crop's last chroma column: nothing to its right is read
    const uint16_t* __restrict__ src = uv + (uint64_t)f * (2ull * (uint64_t)((uint32_t)CW * (uint32_t)CH));
    uint16_t* __restrict__ dst = out + (uint64_t)f * (2ull * (uint64_t)((uint32_t)oCW * (uint32_t)oCH));
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
        if (yo >= oCH) break;
        const Resize16Tab yt = ytab[yo];
        const float b1 = yt.f, b0 = 1.0f - yt.f;
        const uint16_t* __restrict__ p0 = src + (uint32_t)(yt.ofs & 0xFFFF) * (uint32_t)CW * 2u;         // (a plane is below 2^30 samples)
        const uint16_t* __restrict__ p1 = src + (uint32_t)(yt.ofs >> 16) * (uint32_t)CW * 2u;
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

#endif  // MF_RESIZE_HDR_BODY_H
