// _crop_frames (mfs.py:1111-1157) for single-channel uint8 frames: crop to the inclusive rectangle, resize back to (W, H) with
// cv2.resize INTER_LINEAR.  The tables are resize_body.h's (the same resize_tables_kernel, the same workspace, built by launch_crop_resize).
#ifndef MF_RESIZE_C1_BODY_H
#define MF_RESIZE_C1_BODY_H
#include "mf_common.h"
#include "resize_u8.h"
#include "resize_rect.h"

namespace mf {

// ---- single-channel uint8 frames (mf_crop_resize_u8c1): resize_kernel's tiles, tables and arithmetic on one byte per pixel ------------
// cv2.resize runs the same fixed-point HResizeLinear / VResizeLinear per channel, so the grey output is channel 0 of the u8c3 output on a
// frame that repeats the grey one three times.  A wavefront stages the at most kSrcRows source rows its 8 x 256 output pixels need (256
// pixels of an upscale span at most 258 bytes) with one 16-byte global->LDS chunk per lane < 17 and row, from the dword below the first
// byte, and reads the taps there; tiles whose rows or span do not fit, or whose copy would reach past the clip, take the direct form: byte
// loads at the clamped positions, nothing outside the frame stack read.
__global__ __launch_bounds__(64 * kWaves) void resize8c1_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, int n,
                                                        int W, int H, MF_RECT_ARGS,
                                                        const ResizeTab* __restrict__ xtab,
                                                        const ResizeTab* __restrict__ ytab, TileOrder order)
{
    MF_RECT_LOAD(W, H)
    __shared__ __attribute__((aligned(16))) uint8_t s_rows[kWaves][kSrcRows][kC1RowPitch];
    int f, tile_y, tile_x;
    if (!order.decode(blockIdx.x, f, tile_y, tile_x)) return;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int ya = (tile_y * kWaves + wave) * kRows;
    const int xw = tile_x * 256, x0 = xw + lane * 4;
    if (ya >= H) return;
    const int rows = min(kRows, H - ya);
    const size_t frame_bytes = (size_t)W * H;
    const uint8_t* __restrict__ src = frames + (size_t)f * frame_bytes;
    uint8_t* __restrict__ dst = out + (size_t)f * frame_bytes;
    const size_t limit = (size_t)(n - f) * frame_bytes;           // bytes from src to the end of the stack
    const size_t base = (size_t)(uintptr_t)src;

    const uint32_t sx_first = (uint32_t)xtab[xw].ofs, sx_last = (uint32_t)xtab[min(xw + 255, W - 1)].ofs;
    const uint32_t span = sx_last + 2u - sx_first;
    const int r_first = ytab[ya].ofs & 0xFFFF, r_last = ytab[ya + rows - 1].ofs >> 16;
    const int nsrc = r_last - r_first + 1;
    const size_t g_first = (size_t)(top + r_first) * (size_t)W + (size_t)left + sx_first;
    const size_t g_last = g_first + (size_t)(nsrc - 1) * (size_t)W;
    const bool staged = nsrc <= kSrcRows && span + 3u <= (uint32_t)kC1RowPitch && g_first >= 3u && g_last + (size_t)kC1RowPitch <= limit;
    if (staged && lane < kC1RowPitch / 16) {
        uint32_t o = (uint32_t)lane << 4;
        asm("" : "+v"(o));
#pragma unroll 1
        for (int i = 0; i < nsrc; ++i) {
            const size_t g = g_first + (size_t)i * (size_t)W;
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (g - ((base + g) & 3u)) + o),
                                             (__attribute__((address_space(3))) void*)&s_rows[wave][i][0], 16, 0, 0);
        }
    }
    ResizeTab xt[4];
    if (x0 < W) {
#pragma unroll
        for (int j = 0; j < 4; ++j) xt[j] = xtab[min(x0 + j, W - 1)];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // staged rows (and the column table) have landed
    if (x0 >= W) return;

    if (staged) {
        const uint8_t* const s0 = &s_rows[wave][0][0];
        uint32_t rel[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) rel[j] = (uint32_t)xt[j].ofs - sx_first;
        const uint32_t mis0 = (uint32_t)((base + g_first) & 3u), mis_step = (uint32_t)W & 3u;     // misalignment of row i: (mis0 + i mis_step) & 3
#pragma unroll 1
        for (int q = 0; q < rows; ++q) {
            const int y = ya + q;
            const ResizeTab yt = ytab[y];
            const int i0 = (yt.ofs & 0xFFFF) - r_first, i1 = (yt.ofs >> 16) - r_first;
            const uint8_t* const p0 = s0 + i0 * kC1RowPitch + ((mis0 + (uint32_t)i0 * mis_step) & 3u);
            const uint8_t* const p1 = s0 + i1 * kC1RowPitch + ((mis0 + (uint32_t)i1 * mis_step) & 3u);
            const uint32_t b0s = (yt.w & 0xFFFFu) << 8, b1s = (yt.w >> 16) << 8;
            uint32_t px = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t T0 = udot2((uint32_t)p0[rel[j]] | ((uint32_t)p0[rel[j] + 1] << 16), xt[j].w, 0u) & ~255u;
                const uint32_t T1 = udot2((uint32_t)p1[rel[j]] | ((uint32_t)p1[rel[j] + 1] << 16), xt[j].w, 0u) & ~255u;
                px |= ((mulhi_u24(b0s, T0) + mulhi_u24(b1s, T1) + 2u) >> 2) << (8 * j);
            }
            const uint32_t o = (uint32_t)y * (uint32_t)W + (uint32_t)x0;
            if (x0 + 3 < W) {
                __builtin_memcpy(dst + o, &px, 4);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (x0 + j < W) dst[o + j] = (uint8_t)(px >> (8 * j));
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
        const uint32_t o = (uint32_t)y * (uint32_t)W + (uint32_t)x0;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (x0 + j >= W) continue;
            const uint32_t a0 = (xt[j].w & 0xFFFFu) >> 4, a1 = xt[j].w >> 20;
            const uint32_t sx = (uint32_t)xt[j].ofs, sx1 = min(sx + 1u, (uint32_t)(cw - 1));     // a1 == 0 where sx == cw-1
            const uint32_t t0 = (uint32_t)src[row0 + sx] * a0 + (uint32_t)src[row0 + sx1] * a1;
            const uint32_t t1 = (uint32_t)src[row1 + sx] * a0 + (uint32_t)src[row1 + sx1] * a1;
            const uint32_t v = (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2u) >> 2;
            dst[o + j] = (uint8_t)min(v, 255u);
        }
    }
}

}  // namespace mf

#endif  // MF_RESIZE_C1_BODY_H
