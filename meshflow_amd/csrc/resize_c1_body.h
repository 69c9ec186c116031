// _crop_frames (mfs.py:1111-1157) for single-channel uint8 frames: crop to the inclusive rectangle, resize back to (W, H) or to a caller-chosen
// (oW, oH) with cv2.resize INTER_LINEAR -- the u8c1 tile and its kernels: resize8c1_kernel (mf_crop_resize_u8c1) and resize8c1_to_kernel
// (mf_crop_resize_to_u8c1; the luma of the NV12 calls).  The tables are resize_body.h's (the same resize_tables_kernel, the same workspace,
// built by launch_crop_resize / launch_crop_resize_to for the output size).
#ifndef MF_RESIZE_C1_BODY_H
#define MF_RESIZE_C1_BODY_H
#include "mf_common.h"
#include "resize_u8.h"
#include "resize_rect.h"

namespace mf {

// ---- the u8c1 tile: resize_bgr_tile's tiles, tables and arithmetic on one byte per pixel ----------------------------------------------
// cv2.resize runs the same fixed-point HResizeLinear / VResizeLinear per channel, so the grey output is channel 0 of the u8c3 output on a
// frame that repeats the grey one three times.  Source pitch W and frame W H apart from the output oW x oH.  The same three instantiations:
//   up   (oW >= cw and oH >= ch, the same-size call included): a wavefront stages the at most kSrcRows consecutive source rows its 8 x 256
//        output pixels need (256 pixels of an upscale span at most 258 bytes) with one 16-byte global->LDS chunk per lane < 17 and row, from
//        the dword below the first byte, and reads the taps there;
//   down: kDown1Rows output rows per wavefront, exactly the two source rows of each staged (slots 2q, 2q + 1) over up to kDown1Pitch bytes
//        (scale_x up to ~4);
//   direct (PITCH 0, no LDS): beyond that span, as for u8c3.
// Tiles whose rows or span do not fit, or whose copy would reach past the clip, take the direct form: byte loads at the clamped positions,
// nothing outside the frame stack read.  Tile8::fits (resize_u8.h) with the 3 bytes of misalignment as slack; a slot's misalignment is
// Tile8::mis_of (incremental for consecutive rows, as the same-size kernel had it; per row for PAIRS).
// Exactly 2x down in both axes is INTER_AREA's fast path in cv::resize, which for 8-bit data equals this arithmetic at f = 0.5 (resize_body.h).
constexpr int kDown1Rows = 4;
constexpr int kDown1Pitch = 1024;     // one 16-byte chunk per lane and row

template <int ROWS, int SLOTS, int PITCH, bool PAIRS>
__device__ __forceinline__ void resize_c1_tile(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, int n, int W, int H,
                                               int left, int top, int cw, int oW, int oH,
                                               const ResizeTab* __restrict__ xtab, const ResizeTab* __restrict__ ytab, const TileOrder& order)
{
    constexpr int STRIDE = PITCH > 0 ? PITCH : 16;
    __shared__ __attribute__((aligned(16))) uint8_t s_rows[kWaves][SLOTS][STRIDE];
    Tile8<1, ROWS, PAIRS> t;
    if (!t.decode(frames, out, n, W, H, left, top, oW, oH, xtab, ytab, order)) return;
    const bool staged = t.template fits<SLOTS, PITCH, 3, false>(frames);
    ResizeTab xt[4];
    t.template stage_rows<PITCH, STRIDE, false>(staged, &s_rows[t.wave][0][0], xtab, oW, xt);
    const int ya = t.ya, rows = t.rows, x0 = t.x0;
    const uint8_t* __restrict__ src = t.src;
    uint8_t* __restrict__ dst = t.dst;
    if (x0 >= oW) return;

    if (staged) {
        const uint8_t* const s0 = &s_rows[t.wave][0][0];
        uint32_t rel[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) rel[j] = (uint32_t)xt[j].ofs - t.sx_first;
#pragma unroll 1
        for (int q = 0; q < rows; ++q) {
            const int y = ya + q;
            const ResizeTab yt = ytab[y];
            const int i0 = PAIRS ? 2 * q : (yt.ofs & 0xFFFF) - t.r_first, i1 = PAIRS ? 2 * q + 1 : (yt.ofs >> 16) - t.r_first;
            const uint8_t* const p0 = s0 + i0 * STRIDE + t.mis_of(i0);
            const uint8_t* const p1 = s0 + i1 * STRIDE + t.mis_of(i1);
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

// The kernels: the rectangle (launch arguments, or loaded from device memory: resize_rect.h), then the tile.
// resize8c1_kernel: the same-size call, the up instantiation at the frame's own size
__global__ __launch_bounds__(64 * kWaves) void resize8c1_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, int n,
                                                        int W, int H, MF_RECT_ARGS,
                                                        const ResizeTab* __restrict__ xtab,
                                                        const ResizeTab* __restrict__ ytab, TileOrder order)
{
    MF_RECT_LOAD(W, H)
    resize_c1_tile<kRows, kSrcRows, kC1RowPitch, false>(frames, out, n, W, H, left, top, cw, W, H, xtab, ytab, order);
}

template <int ROWS, int SLOTS, int PITCH, bool PAIRS>
__global__ __launch_bounds__(64 * kWaves) void resize8c1_to_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, int n,
                                                                   int W, int H, MF_RECT_ARGS, int oW, int oH,
                                                                   const ResizeTab* __restrict__ xtab,
                                                                   const ResizeTab* __restrict__ ytab, TileOrder order)
{
    MF_RECT_LOAD(W, H)
    resize_c1_tile<ROWS, SLOTS, PITCH, PAIRS>(frames, out, n, W, H, left, top, cw, oW, oH, xtab, ytab, order);
}

}  // namespace mf

#endif  // MF_RESIZE_C1_BODY_H
