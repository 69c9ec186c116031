// _crop_frames (mfs.py:1111-1157) for 4-channel uint8 frames: crop to the inclusive rectangle, resize to (W, H) or to a caller-chosen
// (oW, oH) with cv2.resize INTER_LINEAR -- mf_crop_resize_u8c4 and mf_crop_resize_to_u8c4.  cv2.resize runs the same fixed-point
// HResizeLinear / VResizeLinear per channel, so channels 0-2 of the result are the u8c3 result on channels 0-2 and channel 3 the u8c1 result on
// the alpha plane.  The tables are resize_body.h's (resize_tables_kernel, built by launch_crop_resize / launch_crop_resize_to for the output size).
#ifndef MF_RESIZE_C4_BODY_H
#define MF_RESIZE_C4_BODY_H
#include "mf_common.h"
#include "resize_u8.h"
#include "resize_rect.h"

namespace mf {

// up (oW >= cw and oH >= ch, the same-size call included): resize_kernel's staging -- 8 output rows read at most 9 consecutive source rows,
// 256 output pixels span at most 258 source pixels = 1,032 bytes (65 chunks)
constexpr int kUpRows = 8, kUpSlots = 9, kUpPitch = 1040;
// down: kDown4Rows output rows per wavefront, exactly the two source rows of each staged (slots 2q, 2q + 1) over up to kDown4Pitch bytes (scale_x
// up to ~2.37: a 4K crop to 1080p fits); beyond it the direct instantiation (PITCH 0, no LDS)
constexpr int kDown4Rows = 2, kDown4Pitch = 2432;
static_assert(kUpPitch % 16 == 0 && kDown4Pitch % 16 == 0, "whole 16-byte chunks");

// The horizontal pass of one source row for one output pixel from its two taps (8 contiguous bytes, pixel sx then sx + 1): per channel
// t = S[sx] a0 + S[sx+1] a1 by v_dot2_u32_u16 with the weights pre-scaled by 16 (xtab's w), kept as 256 (t >> 4) -- resize_kernel's T.
__device__ __forceinline__ void hpass_c4(uint32_t p0, uint32_t p1, uint32_t w, uint32_t (&T)[4])
{
#pragma unroll
    for (int c = 0; c < 4; ++c) T[c] = udot2(__builtin_amdgcn_perm(p1, p0, 0x0C040C00u + 0x00010001u * (uint32_t)c), w, 0u) & ~255u;
}

// The vertical pass of one output pixel: (((b0 (t0 >> 4)) >> 16) + ((b1 (t1 >> 4)) >> 16) + 2) >> 2 per channel (<= 255 without saturation:
// resize_u8.h), packed B | G << 8 | R << 16 | A << 24.
__device__ __forceinline__ uint32_t vpass_c4(const uint32_t (&T0)[4], const uint32_t (&T1)[4], uint32_t b0s, uint32_t b1s)
{
    uint32_t px = 0;
#pragma unroll
    for (int c = 0; c < 4; ++c) px |= ((mulhi_u24(b0s, T0[c]) + mulhi_u24(b1s, T1[c]) + 2u) >> 2) << (8 * c);
    return px;
}

// The lane's four output pixels of one row: one 16-byte store, or pixel by pixel at the end of a row of oW % 4 != 0
__device__ __forceinline__ void store_c4(uint8_t* __restrict__ dst, uint32_t o, int x0, int oW, const uint32_t (&px)[4])
{
    if (x0 + 3 < oW) {
        const uint4 q = make_uint4(px[0], px[1], px[2], px[3]);
        __builtin_memcpy(dst + o, &q, 16);
    } else {                                                            // (a loop: its stores do not merge with the 16-byte one)
        const int m = oW - x0;
#pragma unroll 1
        for (int j = 0; j < m; ++j) __builtin_memcpy(dst + o + 4 * j, &px[j], 4);
    }
}

// Workgroup = kWaves wavefronts; wavefront = ROWS consecutive output rows x 256 pixels; lane = 4 consecutive pixels per row.  Source pitch W
// and frame 4 W H bytes, output oW x oH (the same-size call: oW = W, oH = H).  Staged (PITCH > 0, a 4-byte aligned stack, the span and rows
// fit, the copy stays inside the stack): the source rows go to LDS slots with one 16-byte global->LDS load per lane and chunk, a pixel's taps
// are two dwords there; slot i holds source row r_first + i (up) or row h of output row ya + q for i = 2q + h (PAIRS).  Everything else takes
// the direct form: four 4-byte loads per pixel at the clamped tap positions, nothing outside the frame stack read.
template <int ROWS, int SLOTS, int PITCH, bool PAIRS>
__global__ __launch_bounds__(64 * kWaves) void resize8c4_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, int n,
                                                                int W, int H, MF_RECT_ARGS, int oW, int oH,
                                                                const ResizeTab* __restrict__ xtab,
                                                                const ResizeTab* __restrict__ ytab, TileOrder order)
{
    MF_RECT_LOAD(W, H)
    constexpr int STRIDE = PITCH > 0 ? PITCH : 4;
    __shared__ __attribute__((aligned(16))) uint32_t s_rows[kWaves][SLOTS][STRIDE / 4];
    Tile8<4, ROWS, PAIRS> t;
    if (!t.decode(frames, out, n, W, H, left, top, oW, oH, xtab, ytab, order)) return;
    // (Tile8::fits, ALIGNED: a pixel is a dword, so on a 4-byte aligned stack every copy starts at its first tap -- no misalignment, no slack)
    const bool staged = t.template fits<SLOTS, PITCH, 0, true>(frames);
    ResizeTab xt[4];
    t.template stage_rows<PITCH, STRIDE, true>(staged, (uint8_t*)&s_rows[t.wave][0][0], xtab, oW, xt);
    const int ya = t.ya, rows = t.rows, x0 = t.x0;
    const uint8_t* __restrict__ src = t.src;
    uint8_t* __restrict__ dst = t.dst;
    if (x0 >= oW) return;

    if (staged) {
        uint32_t rel[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) rel[j] = (uint32_t)xt[j].ofs - t.sx_first;        // in dwords
        const auto hpass_slot = [&](int i, uint32_t (&T)[4][4]) {
            const uint32_t* const s = &s_rows[t.wave][i][0];
#pragma unroll
            for (int j = 0; j < 4; ++j) hpass_c4(s[rel[j]], s[rel[j] + 1], xt[j].w, T[j]);
        };
        // resize_kernel's two register sets: an output row whose first source row is the previous one's second reuses its horizontal pass
        // (up); with PAIRS every slot is a row of its own and each set is refilled
        uint32_t Ta[4][4], Tb[4][4], px[4];
        int have_a = -1, have_b = -1;
#pragma unroll 1
        for (int q = 0; q < rows; q += 2) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int y = ya + q + h;
                if (y >= ya + rows) break;
                const ResizeTab yt = ytab[y];
                const int i0 = PAIRS ? 2 * (q + h) : (yt.ofs & 0xFFFF) - t.r_first, i1 = PAIRS ? 2 * (q + h) + 1 : (yt.ofs >> 16) - t.r_first;
                const uint32_t b0s = (yt.w & 0xFFFFu) << 8, b1s = (yt.w >> 16) << 8;
                const uint32_t o = ((uint32_t)y * (uint32_t)oW + (uint32_t)x0) * 4u;
                if (h == 0) {
                    if (have_a != i0) { hpass_slot(i0, Ta); have_a = i0; }
                    if (have_b != i1) { hpass_slot(i1, Tb); have_b = i1; }
#pragma unroll
                    for (int j = 0; j < 4; ++j) px[j] = vpass_c4(Ta[j], Tb[j], b0s, b1s);
                } else {
                    if (have_b != i0) { hpass_slot(i0, Tb); have_b = i0; }
                    if (have_a != i1) { hpass_slot(i1, Ta); have_a = i1; }
#pragma unroll
                    for (int j = 0; j < 4; ++j) px[j] = vpass_c4(Tb[j], Ta[j], b0s, b1s);
                }
                store_c4(dst, o, x0, oW, px);
            }
        }
        return;
    }

    // direct form: taps straight from the frame, row by row, at positions inside the crop (a1 == 0 where sx == cw - 1)
#pragma unroll 1
    for (int q = 0; q < rows; ++q) {
        const int y = ya + q;
        const ResizeTab yt = ytab[y];
        const uint32_t b0s = (yt.w & 0xFFFFu) << 8, b1s = (yt.w >> 16) << 8;
        const uint32_t row0 = (uint32_t)(top + (yt.ofs & 0xFFFF)) * (uint32_t)W + (uint32_t)left;
        const uint32_t row1 = (uint32_t)(top + (yt.ofs >> 16)) * (uint32_t)W + (uint32_t)left;
        uint32_t px[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t sx = (uint32_t)xt[j].ofs, sx1 = min(sx + 1u, (uint32_t)(cw - 1));
            uint32_t p00, p01, p10, p11;
            __builtin_memcpy(&p00, src + 4ull * (row0 + sx), 4);
            __builtin_memcpy(&p01, src + 4ull * (row0 + sx1), 4);
            __builtin_memcpy(&p10, src + 4ull * (row1 + sx), 4);
            __builtin_memcpy(&p11, src + 4ull * (row1 + sx1), 4);
            uint32_t T0[4], T1[4];
            hpass_c4(p00, p01, xt[j].w, T0);
            hpass_c4(p10, p11, xt[j].w, T1);
            px[j] = vpass_c4(T0, T1, b0s, b1s);
        }
        store_c4(dst, ((uint32_t)y * (uint32_t)oW + (uint32_t)x0) * 4u, x0, oW, px);
    }
}

}  // namespace mf

#endif  // MF_RESIZE_C4_BODY_H
