// _crop_frames to a caller-chosen output size: cv2.resize(crop, (oW, oH)) with INTER_LINEAR (mfs.py:1150-1155 with any dsize), the kernels of
// mf_crop_resize_to_u8c3 / _u16c3 / _u8c1.  launch_crop_resize_to (resize.hip) checks the call, sends oW x oH == W x H to the same-size kernels
// and builds the tables for (oW, oH) -- resize_tables_kernel's (resize_body.h) or resize16_tables_kernel's (resize16_body.h) -- before it
// launches these.
#ifndef MF_RESIZE_TO_BODY_H
#define MF_RESIZE_TO_BODY_H
#include "mf_common.h"
#include "resize_u8.h"
#include "resize_rect.h"

namespace mf {

// ---- u8c3 (mf_crop_resize_to_u8c3) -----------------------------------------------------------------------------------------------------
// Source geometry (pitch W, frame W H 3 bytes) and output geometry (oW x oH) apart; the tables are resize_tables_kernel's for (oW, oH).
// Three instantiations of one kernel, all with resize_kernel's lanes (4 output pixels, one 12-byte store) and arithmetic:
//   up   (oW >= cw and oH >= ch): resize_kernel's staged design -- 8 output rows per wavefront read at most 9 consecutive source rows, 256
//        output pixels span at most 258 source pixels; the rows r_first .. r_last go to LDS slots 0 .. nsrc-1.
//   down (anything else): consecutive output rows share few or no source rows, and 256 output pixels span ~256 scale_x source pixels.
//        A wavefront owns kDownRows output rows and stages exactly the two source rows of each (slots 2q, 2q + 1: no unused row is
//        copied) over a span of up to kDownPitch bytes.
//   direct (PITCH 0: no LDS at all): where 256 output pixels span more than kDownPitch bytes (scale_x above ~2.6), taps from the frame.
//        Its own instantiation because the down kernel's 33 KB of LDS per workgroup cost occupancy even in wavefronts that do not stage
//        (4-5 % just above the cut-over).
// up and down fall back to the direct path per wavefront wherever staging would not fit or would read outside the stack.
// Exactly 2x down in both axes: cv::resize runs INTER_AREA's fast path there ((S00 + S01 + S10 + S11 + 2) >> 2); for 8-bit data that is
// this fixed-point bilinear result (f = 0.5: a0 = a1 = b0 = b1 = 1024, t >> 4 = 64 (S0 + S1), each high half = S0 + S1), so nothing extra.
#ifndef MF_RESIZE_TO_STAGE_BYTES
#define MF_RESIZE_TO_STAGE_BYTES 2048     // kDownPitch (a build-time knob for the staged / direct measurement)
#endif
constexpr int kDownRows = 2;                                   // output rows per wavefront of the down instantiation
constexpr int kDownPitch = MF_RESIZE_TO_STAGE_BYTES;           // bytes of one staged source row (a multiple of 16)
static_assert(kDownPitch % 16 == 0 && kDownPitch >= 16, "whole 16-byte chunks");

template <int ROWS, int SLOTS, int PITCH, bool PAIRS>
__global__ __launch_bounds__(64 * kWaves) void resize_to_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, int n,
                                                                int W, int H, MF_RECT_ARGS, int oW, int oH,
                                                                const ResizeTab* __restrict__ xtab,
                                                                const ResizeTab* __restrict__ ytab, TileOrder order)
{
    MF_RECT_LOAD(W, H)
    __shared__ __attribute__((aligned(16))) uint8_t s_rows[kWaves][SLOTS][PITCH + 16];
    int f, tile_y, tile_x;
    if (!order.decode(blockIdx.x, f, tile_y, tile_x)) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int ya = (tile_y * kWaves + wave) * ROWS;
    const int xw = tile_x * 256, x0 = xw + lane * 4;
    if (ya >= oH) return;
    const int rows = min(ROWS, oH - ya);
    const size_t frame_bytes = (size_t)W * H * 3, out_frame_bytes = (size_t)oW * oH * 3;
    const uint8_t* __restrict__ src = frames + (size_t)f * frame_bytes;
    uint8_t* __restrict__ dst = out + (size_t)f * out_frame_bytes;
    const size_t limit = (size_t)(n - f) * frame_bytes;
    const size_t base = (size_t)(uintptr_t)src;

    const uint32_t sx_first = (uint32_t)xtab[xw].ofs, sx_last = (uint32_t)xtab[min(xw + 255, oW - 1)].ofs;
    const uint32_t span = 3u * (sx_last + 2u - sx_first);
    // slot i holds source row src_row(i): r_first + i (up), or row h of output row ya + q for i = 2q + h (PAIRS)
    const int r_first = ytab[ya].ofs & 0xFFFF, r_last = ytab[ya + rows - 1].ofs >> 16;
    const int nsrc = PAIRS ? 2 * rows : r_last - r_first + 1;
    const auto src_row = [&](int i) {
        if (!PAIRS) return r_first + i;
        const int32_t o = ytab[ya + (i >> 1)].ofs;
        return (i & 1) ? (o >> 16) : (o & 0xFFFF);
    };
    const auto g_of = [&](int r) { return ((size_t)(top + r) * (size_t)W + (size_t)left + sx_first) * 3u; };
    // (the rows are monotone: the first and the last staged row bound every copy)
    const bool staged = PITCH > 0 && nsrc <= SLOTS && span + 3u + 12u <= (uint32_t)PITCH && g_of(r_first) >= 3u &&
                        g_of(r_last) + (size_t)PITCH <= limit;
    if (staged) {
#pragma unroll 1
        for (int i = 0; i < nsrc; ++i) {
            const size_t g = g_of(src_row(i));
            const uint8_t* const a = src + (g - ((base + g) & 3u));
#pragma unroll
            for (int c = 0; c < PITCH / 16; c += 64) {
                if (lane + c < PITCH / 16) {
                    uint32_t o = (uint32_t)(lane + c) << 4;
                    asm("" : "+v"(o));
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a + o),
                                                     (__attribute__((address_space(3))) void*)&s_rows[wave][i][c * 16], 16, 0, 0);
                }
            }
        }
    }
    ResizeTab xt[4];
    if (x0 < oW) {
#pragma unroll
        for (int j = 0; j < 4; ++j) xt[j] = xtab[min(x0 + j, oW - 1)];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // staged rows (and the column table) have landed
    if (x0 >= oW) return;

    if (staged) {
        uint32_t rel[4], wq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { rel[j] = 3u * ((uint32_t)xt[j].ofs - sx_first) + (uint32_t)(uintptr_t)&s_rows[wave][0][0]; wq[j] = xt[j].w; }
        const auto row_at = [&](int i, uint32_t (&at)[4]) {
            const uint32_t add = (uint32_t)i * (uint32_t)(PITCH + 16) + (uint32_t)((base + g_of(src_row(i))) & 3u);
#pragma unroll
            for (int j = 0; j < 4; ++j) at[j] = rel[j] + add;
        };
        // resize_kernel's two register sets: an output row whose first source row is the previous one's second reuses its horizontal pass
        // (up); with PAIRS every slot is a row of its own and each set is refilled
        uint32_t Ta[4][3], Tb[4][3], at[4];
        int have_a = -1, have_b = -1;
#pragma unroll 1
        for (int q = 0; q < rows; q += 2) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int y = ya + q + h;
                if (y >= ya + rows) break;
                const ResizeTab yt = ytab[y];
                const int i0 = PAIRS ? 2 * (q + h) : (yt.ofs & 0xFFFF) - r_first, i1 = PAIRS ? 2 * (q + h) + 1 : (yt.ofs >> 16) - r_first;
                const uint32_t b0s = (yt.w & 0xFFFFu) << 8, b1s = (yt.w >> 16) << 8;
                const uint32_t o = ((uint32_t)y * (uint32_t)oW + (uint32_t)x0) * 3u;
                if (h == 0) {
                    if (have_a != i0) { row_at(i0, at); hpass_row(at, wq, Ta); have_a = i0; }
                    if (have_b != i1) { row_at(i1, at); hpass_row(at, wq, Tb); have_b = i1; }
                    vpass_store(Ta, Tb, b0s, b1s, dst, o, x0, oW);
                } else {
                    if (have_b != i0) { row_at(i0, at); hpass_row(at, wq, Tb); have_b = i0; }
                    if (have_a != i1) { row_at(i1, at); hpass_row(at, wq, Ta); have_a = i1; }
                    vpass_store(Tb, Ta, b0s, b1s, dst, o, x0, oW);
                }
            }
        }
        return;
    }

    // direct path: taps straight from the frame, row by row (resize_kernel's)
#pragma unroll 1
    for (int q = 0; q < rows; ++q) {
        const int y = ya + q;
        const ResizeTab yt = ytab[y];
        const uint32_t b0s = (yt.w & 0xFFFFu) << 8, b1s = (yt.w >> 16) << 8;
        const uint32_t row0 = (uint32_t)(top + (yt.ofs & 0xFFFF)) * (uint32_t)W + (uint32_t)left;
        const uint32_t row1 = (uint32_t)(top + (yt.ofs >> 16)) * (uint32_t)W + (uint32_t)left;
        const uint32_t o = ((uint32_t)y * (uint32_t)oW + (uint32_t)x0) * 3u;
        const bool whole = x0 + 3 < oW && ((size_t)(max(row0, row1) + (uint32_t)cw) * 3u + 8u <= limit);
        if (whole) {
            uint32_t T0[4][3], T1[4][3];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint2 a, b;                                              // bytes: B0 G0 R0 B1 | G1 R1 . .
                __builtin_memcpy(&a, src + (row0 + (uint32_t)xt[j].ofs) * 3u, 8);
                __builtin_memcpy(&b, src + (row1 + (uint32_t)xt[j].ofs) * 3u, 8);
                const uint32_t w = xt[j].w;
                T0[j][0] = udot2(__builtin_amdgcn_perm(a.y, a.x, 0x0C030C00u), w, 0u) & ~255u; T1[j][0] = udot2(__builtin_amdgcn_perm(b.y, b.x, 0x0C030C00u), w, 0u) & ~255u;
                T0[j][1] = udot2(__builtin_amdgcn_perm(a.y, a.x, 0x0C040C01u), w, 0u) & ~255u; T1[j][1] = udot2(__builtin_amdgcn_perm(b.y, b.x, 0x0C040C01u), w, 0u) & ~255u;
                T0[j][2] = udot2(__builtin_amdgcn_perm(a.y, a.x, 0x0C050C02u), w, 0u) & ~255u; T1[j][2] = udot2(__builtin_amdgcn_perm(b.y, b.x, 0x0C050C02u), w, 0u) & ~255u;
            }
            vpass_store(T0, T1, b0s, b1s, dst, o, x0, oW);
            continue;
        }
        const uint32_t b0 = b0s >> 8, b1 = b1s >> 8;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x0 + j >= oW) continue;
            const uint32_t a0 = (xt[j].w & 0xFFFFu) >> 4, a1 = xt[j].w >> 20;
            const uint32_t sx = (uint32_t)xt[j].ofs, sx1 = min(sx + 1u, (uint32_t)(cw - 1));     // a1 == 0 where sx == cw-1
            const uint32_t p00 = load_bgr(src, (row0 + sx) * 3u, limit), p01 = load_bgr(src, (row0 + sx1) * 3u, limit);
            const uint32_t p10 = load_bgr(src, (row1 + sx) * 3u, limit), p11 = load_bgr(src, (row1 + sx1) * 3u, limit);
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const uint32_t t0 = ((p00 >> (8 * c)) & 255u) * a0 + ((p01 >> (8 * c)) & 255u) * a1;
                const uint32_t t1 = ((p10 >> (8 * c)) & 255u) * a0 + ((p11 >> (8 * c)) & 255u) * a1;
                const uint32_t v = (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2u) >> 2;
                dst[o + 3 * j + c] = (uint8_t)min(v, 255u);
            }
        }
    }
}

// ---- u8c1 (mf_crop_resize_to_u8c1): resize_to_kernel's split on one byte per pixel ------------------------------------------------------
// Source pitch W and frame W H apart from the output oW x oH; resize_body.h's tables for (oW, oH).  up (oW >= cw and oH >= ch): resize8c1_kernel's
// staging (8 output rows, at most 9 consecutive source rows, 258 bytes of span); down: kDown1Rows output rows per wavefront, exactly the two
// source rows of each staged (slots 2q, 2q + 1) over up to kDown1Pitch bytes (scale_x up to ~4), beyond it the direct instantiation (PITCH
// 0, no LDS), as for u8c3.  Exactly 2x down
// in both axes is INTER_AREA's fast path in cv::resize, which for 8-bit data equals this arithmetic at f = 0.5 (resize_body.h).
constexpr int kDown1Rows = 4;
constexpr int kDown1Pitch = 1024;     // one 16-byte chunk per lane and row

template <int ROWS, int SLOTS, int PITCH, bool PAIRS>
__global__ __launch_bounds__(64 * kWaves) void resize8c1_to_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, int n,
                                                                   int W, int H, MF_RECT_ARGS, int oW, int oH,
                                                                   const ResizeTab* __restrict__ xtab,
                                                                   const ResizeTab* __restrict__ ytab, TileOrder order)
{
    MF_RECT_LOAD(W, H)
    __shared__ __attribute__((aligned(16))) uint8_t s_rows[kWaves][SLOTS][PITCH > 0 ? PITCH : 16];
    int f, tile_y, tile_x;
    if (!order.decode(blockIdx.x, f, tile_y, tile_x)) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int ya = (tile_y * kWaves + wave) * ROWS;
    const int xw = tile_x * 256, x0 = xw + lane * 4;
    if (ya >= oH) return;
    const int rows = min(ROWS, oH - ya);
    const size_t frame_bytes = (size_t)W * H, out_frame_bytes = (size_t)oW * oH;
    const uint8_t* __restrict__ src = frames + (size_t)f * frame_bytes;
    uint8_t* __restrict__ dst = out + (size_t)f * out_frame_bytes;
    const size_t limit = (size_t)(n - f) * frame_bytes;           // bytes from src to the end of the stack
    const size_t base = (size_t)(uintptr_t)src;

    const uint32_t sx_first = (uint32_t)xtab[xw].ofs, sx_last = (uint32_t)xtab[min(xw + 255, oW - 1)].ofs;
    const uint32_t span = sx_last + 2u - sx_first;
    const int r_first = ytab[ya].ofs & 0xFFFF, r_last = ytab[ya + rows - 1].ofs >> 16;
    const int nsrc = PAIRS ? 2 * rows : r_last - r_first + 1;
    const auto src_row = [&](int i) {
        if (!PAIRS) return r_first + i;
        const int32_t o = ytab[ya + (i >> 1)].ofs;
        return (i & 1) ? (o >> 16) : (o & 0xFFFF);
    };
    const auto g_of = [&](int r) { return (size_t)(top + r) * (size_t)W + (size_t)left + sx_first; };
    const bool staged = PITCH > 0 && nsrc <= SLOTS && span + 3u <= (uint32_t)PITCH && g_of(r_first) >= 3u && g_of(r_last) + (size_t)PITCH <= limit;
    if (staged) {
#pragma unroll 1
        for (int i = 0; i < nsrc; ++i) {
            const size_t g = g_of(src_row(i));
            const uint8_t* const a = src + (g - ((base + g) & 3u));
#pragma unroll
            for (int c = 0; c < PITCH / 16; c += 64) {
                if (lane + c < PITCH / 16) {
                    uint32_t o = (uint32_t)(lane + c) << 4;
                    asm("" : "+v"(o));
                    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(a + o),
                                                     (__attribute__((address_space(3))) void*)&s_rows[wave][i][c * 16], 16, 0, 0);
                }
            }
        }
    }
    ResizeTab xt[4];
    if (x0 < oW) {
#pragma unroll
        for (int j = 0; j < 4; ++j) xt[j] = xtab[min(x0 + j, oW - 1)];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // staged rows (and the column table) have landed
    if (x0 >= oW) return;

    if (staged) {
        const uint8_t* const s0 = &s_rows[wave][0][0];
        uint32_t rel[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) rel[j] = (uint32_t)xt[j].ofs - sx_first;
#pragma unroll 1
        for (int q = 0; q < rows; ++q) {
            const int y = ya + q;
            const ResizeTab yt = ytab[y];
            const int i0 = PAIRS ? 2 * q : (yt.ofs & 0xFFFF) - r_first, i1 = PAIRS ? 2 * q + 1 : (yt.ofs >> 16) - r_first;
            const uint8_t* const p0 = s0 + i0 * PITCH + ((base + g_of(src_row(i0))) & 3u);
            const uint8_t* const p1 = s0 + i1 * PITCH + ((base + g_of(src_row(i1))) & 3u);
            const uint32_t b0s = (yt.w & 0xFFFFu) << 8, b1s = (yt.w >> 16) << 8;
            uint32_t px = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t T0 = udot2((uint32_t)p0[rel[j]] | ((uint32_t)p0[rel[j] + 1] << 16), xt[j].w, 0u) & ~255u;
                const uint32_t T1 = udot2((uint32_t)p1[rel[j]] | ((uint32_t)p1[rel[j] + 1] << 16), xt[j].w, 0u) & ~255u;
                px |= ((mulhi_u24(b0s, T0) + mulhi_u24(b1s, T1) + 2u) >> 2) << (8 * j);
            }
            const uint32_t o = (uint32_t)y * (uint32_t)oW + (uint32_t)x0;
            if (x0 + 3 < oW) {
                __builtin_memcpy(dst + o, &px, 4);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x0 + j < oW) dst[o + j] = (uint8_t)(px >> (8 * j));
            }
        }
        return;
    }

    // direct path: taps straight from the frame, row by row
#pragma unroll 1
    for (int q = 0; q < rows; ++q) {
        const int y = ya + q;
        const ResizeTab yt = ytab[y];
        const uint32_t b0 = yt.w & 0xFFFFu, b1 = yt.w >> 16;
        const uint32_t row0 = (uint32_t)(top + (yt.ofs & 0xFFFF)) * (uint32_t)W + (uint32_t)left;
        const uint32_t row1 = (uint32_t)(top + (yt.ofs >> 16)) * (uint32_t)W + (uint32_t)left;
        const uint32_t o = (uint32_t)y * (uint32_t)oW + (uint32_t)x0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x0 + j >= oW) continue;
            const uint32_t a0 = (xt[j].w & 0xFFFFu) >> 4, a1 = xt[j].w >> 20;
            const uint32_t sx = (uint32_t)xt[j].ofs, sx1 = min(sx + 1u, (uint32_t)(cw - 1));     // a1 == 0 where sx == cw-1
            const uint32_t t0 = (uint32_t)src[row0 + sx] * a0 + (uint32_t)src[row0 + sx1] * a1;
            const uint32_t t1 = (uint32_t)src[row1 + sx] * a0 + (uint32_t)src[row1 + sx1] * a1;
            const uint32_t v = (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2u) >> 2;
            dst[o + j] = (uint8_t)min(v, 255u);
        }
    }
}

// ---- u16c3 (mf_crop_resize_to_u16c3) ---------------------------------------------------------------------------------------------------
// resize16_kernel with the source pitch W and frame W H apart from the output oW x oH (resize16_tables_kernel's tables for (oW, oH)): one
// thread per output pixel, taps straight from the frame.  `area`: the crop is exactly twice the output in both axes (2 oW == cw and
// 2 oH == ch), where cv::hal::resize hands INTER_LINEAR to INTER_AREA's fast path (is_area_fast && iscale_x == 2 && iscale_y == 2), whose
// 16-bit form is (S00 + S01 + S10 + S11 + 2) >> 2 -- rounded half UP, where the float path would round the same quarter-sums half to even.
// The tables there give sx = 2 dx, sy0 = 2 dy, sy1 = 2 dy + 1, so the four taps are the ones the float path reads.
__global__ __launch_bounds__(256) void resize16_to_kernel(const uint16_t* __restrict__ frames, uint16_t* __restrict__ out, int W, int H,
                                                          MF_RECT16_TO_ARGS,
                                                          const Resize16Tab* __restrict__ xtab, const Resize16Tab* __restrict__ ytab,
                                                          TileOrder order)
{
    MF_RECT16_TO_LOAD(W, H)
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

}  // namespace mf

#endif  // MF_RESIZE_TO_BODY_H
