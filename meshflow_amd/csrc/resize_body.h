// Crop + bilinear resize of u8c3 frames: the step right after the warp in the reference's stabilize()
// (meshflowstabilizer.py:159 -> _crop_frames, :1111-1157): every frame is cropped to the clip-level bounds
// (inclusive) and scaled back to (W, H) with cv2.resize's default INTER_LINEAR -- or to a caller-chosen (oW, oH),
// cv2.resize(crop, (oW, oH)) (mfs.py:1150-1155 with any dsize).  The 8-bit tables kernel, the u8c3 tile, and its
// kernels: resize_kernel (mf_crop_resize_u8c3) and resize_to_kernel (mf_crop_resize_to_u8c3).
//
// cv2.resize for 8-bit images (imgproc/resize.cpp, cv::hal::resize + resizeGeneric_) is a two-pass 11-bit
// fixed-point interpolation:
//   scale = 1 / ((double)dst / src);  f = float((d + 0.5) * scale - 0.5);  s = floor(f);  f -= s
//   x axis: s < 0 -> (0, 0);  s >= src-1 -> (src-1, 0)        y axis: the two row indices are clipped instead
//   weights  a0 = cvRound((1 - f) * 2048), a1 = cvRound(f * 2048)          (int16)
//   horizontal  t  = S[s] * a0 + S[s+1] * a1                                (int32)
//   vertical    out = (((b0 * (t0 >> 4)) >> 16) + ((b1 * (t1 >> 4)) >> 16) + 2) >> 2
// resize_tables_kernel builds the per-column / per-row tables (W + H entries) on the device in the same
// float / double operations; resize_bgr_tile applies them: a lane owns 4 consecutive output pixels (one
// 12-byte store), the two source rows of an output row staged in LDS, v_dot2_u32_u16 for the horizontal pass.
// Memory-bound in principle (2*H*W*3 bytes per frame).
// Device code only, written against resize_rect.h's macros: resize.hip compiles it with the rectangle as launch arguments, resize_dev.hip a
// second time with the rectangle read from device memory.
#ifndef MF_RESIZE_BODY_H
#define MF_RESIZE_BODY_H
#include "mf_common.h"
#include "resize_u8.h"
#include "resize_rect.h"

namespace mf {

__device__ __forceinline__ int cv_round_pos(float v) { return (int)rintf(v); }

__global__ __launch_bounds__(256) void resize_tables_kernel(MF_TABLES_ARGS,
                                                            ResizeTab* __restrict__ xtab, ResizeTab* __restrict__ ytab)
{
    MF_TABLES_LOAD(W, H)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < W) {
        float fx = (float)(((double)i + 0.5) * scale_x - 0.5);
        int sx = (int)floorf(fx);
        fx -= (float)sx;
        if (sx < 0) { fx = 0.0f; sx = 0; }
        if (sx >= cw - 1) { fx = 0.0f; sx = cw - 1; }
        const int a0 = cv_round_pos((1.0f - fx) * 2048.0f), a1 = cv_round_pos(fx * 2048.0f);
        xtab[i].ofs = sx;
        xtab[i].w = ((uint32_t)a0 << 4) | ((uint32_t)a1 << 20);
    }
    if (i < H) {
        float fy = (float)(((double)i + 0.5) * scale_y - 0.5);
        const int sy = (int)floorf(fy);
        fy -= (float)sy;
        const int b0 = cv_round_pos((1.0f - fy) * 2048.0f), b1 = cv_round_pos(fy * 2048.0f);
        const int sy0 = min(max(sy, 0), ch - 1), sy1 = min(max(sy + 1, 0), ch - 1);
        ytab[i].ofs = sy0 | (sy1 << 16);
        ytab[i].w = (uint32_t)b0 | ((uint32_t)b1 << 16);
    }
}

// ---- the u8c3 tile (mf_crop_resize_u8c3, mf_crop_resize_to_u8c3 and their device-rectangle twins) ---------------------------------------
// Workgroup = kWaves wavefronts; wavefront = ROWS consecutive output rows x 256 pixels; lane = 4 consecutive pixels per row (one 12-byte
// store each).  Source geometry (pitch W, frame W H 3 bytes) and output geometry (oW x oH) apart; the tables are resize_tables_kernel's for
// (oW, oH).  Three instantiations of one body:
//   up   (oW >= cw and oH >= ch; _crop_frames' own same-size call, oW x oH == W x H, is one: the crop lies inside the frame): the source
//        rows of an output row are shared by all its pixels and by the NEXT output row too -- the 8 output rows of a wavefront read at most
//        9 consecutive source rows, 256 output pixels span at most 258 source pixels.  The wavefront copies the span it needs of each
//        (<= 800 bytes, from the dword holding the first tap) into LDS slots 0 .. nsrc-1 with ONE global->LDS 16-byte load per lane and row,
//        runs the horizontal pass once per SOURCE row (the result of an output row's second source row is the next output row's first) and
//        the vertical pass per output row: (ROWS + 1) / ROWS horizontal passes per output row instead of 2, 9 window copies per 8 rows
//        instead of 16.
//   down (anything else): consecutive output rows share few or no source rows, and 256 output pixels span ~256 scale_x source pixels.
//        A wavefront owns kDownRows output rows and stages exactly the two source rows of each (slots 2q, 2q + 1: no unused row is
//        copied) over a span of up to kDownPitch bytes.
//   direct (PITCH 0: no LDS at all): where 256 output pixels span more than kDownPitch bytes (scale_x above ~2.6), taps from the frame.
//        Its own instantiation because the down kernel's 33 KB of LDS per workgroup cost occupancy even in wavefronts that do not stage
//        (4-5 % just above the cut-over).
// up and down fall back to the direct path per wavefront wherever staging would not fit or would read outside the stack (a frame narrower
// than a chunk, the last rows of the stack): Tile8::fits (resize_u8.h) with a slack of 3 bytes of misalignment + 12.  Where the
// same-size and the to-size kernel were two texts, the choices here are: the copy is bounded by PITCH bytes from the last row's first TAP
// (the to-size form, the more conservative one: the same-size kernel counted from the row's aligned start, up to 3 bytes less), and a slot's
// misalignment comes from Tile8::mis_of, incremental for consecutive rows (the same-size form) and per row for PAIRS.  Staged and direct
// paths compute the same bytes, so only the path a tile at the very end of the stack takes depends on the bound.
// Exactly 2x down in both axes: cv::resize runs INTER_AREA's fast path there ((S00 + S01 + S10 + S11 + 2) >> 2); for 8-bit data that is
// this fixed-point bilinear result (f = 0.5: a0 = a1 = b0 = b1 = 1024, t >> 4 = 64 (S0 + S1), each high half = S0 + S1), so nothing extra.
#ifndef MF_RESIZE_TO_STAGE_BYTES
#define MF_RESIZE_TO_STAGE_BYTES 2048     // kDownPitch (a build-time knob for the staged / direct measurement)
#endif
constexpr int kDownRows = 2;                                   // output rows per wavefront of the down instantiation
constexpr int kDownPitch = MF_RESIZE_TO_STAGE_BYTES;           // bytes of one staged source row (a multiple of 16)
static_assert(kDownPitch % 16 == 0 && kDownPitch >= 16, "whole 16-byte chunks");

template <int ROWS, int SLOTS, int PITCH, bool PAIRS>
__device__ __forceinline__ void resize_bgr_tile(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, int n, int W, int H,
                                                int left, int top, int cw, int oW, int oH,
                                                const ResizeTab* __restrict__ xtab, const ResizeTab* __restrict__ ytab, const TileOrder& order)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_rows[kWaves][SLOTS][PITCH + 16];
    Tile8<3, ROWS, PAIRS> t;
    if (!t.decode(frames, out, n, W, H, left, top, oW, oH, xtab, ytab, order)) return;
    const bool staged = t.template fits<SLOTS, PITCH, 3 + 12, false>(frames);
    ResizeTab xt[4];
    t.template stage_rows<PITCH, PITCH + 16, false>(staged, &s_rows[t.wave][0][0], xtab, oW, xt);
    const int ya = t.ya, rows = t.rows, x0 = t.x0;
    const uint8_t* __restrict__ src = t.src;
    uint8_t* __restrict__ dst = t.dst;
    if (x0 >= oW) return;

    if (staged) {
        uint32_t rel[4], wq[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) { rel[j] = 3u * ((uint32_t)xt[j].ofs - t.sx_first) + (uint32_t)(uintptr_t)&s_rows[t.wave][0][0]; wq[j] = xt[j].w; }
        const auto row_at = [&](int i, uint32_t (&at)[4]) {
            const uint32_t add = (uint32_t)i * (uint32_t)(PITCH + 16) + t.mis_of(i);
#pragma unroll
            for (int j = 0; j < 4; ++j) at[j] = rel[j] + add;
        };
        // Two register sets take turns as "first source row" and "second source row" of an output row (no copies): an output row
        // whose first source row is the previous one's second reuses its horizontal pass (up); with PAIRS every slot is a row of its own
        // and each set is refilled.
        uint32_t Ta[4][3], Tb[4][3], at[4];
        int have_a = -1, have_b = -1;                                  // slot each set holds
#pragma unroll 1
        for (int q = 0; q < rows; q += 2) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int y = ya + q + h;
                if (y >= ya + rows) break;
                const ResizeTab yt = ytab[y];
                const int i0 = PAIRS ? 2 * (q + h) : (yt.ofs & 0xFFFF) - t.r_first, i1 = PAIRS ? 2 * (q + h) + 1 : (yt.ofs >> 16) - t.r_first;
                const uint32_t b0s = (yt.w & 0xFFFFu) << 8, b1s = (yt.w >> 16) << 8;
                const uint32_t o = ((uint32_t)y * (uint32_t)oW + (uint32_t)x0) * 3u;
                if (h == 0) {                                          // first source row in set A, second in set B
                    if (have_a != i0) { row_at(i0, at); hpass_row(at, wq, Ta); have_a = i0; }
                    if (have_b != i1) { row_at(i1, at); hpass_row(at, wq, Tb); have_b = i1; }
                    vpass_store(Ta, Tb, b0s, b1s, dst, o, x0, oW);
                } else {                                               // ... and the other way round: this row's first is usually set B
                    if (have_b != i0) { row_at(i0, at); hpass_row(at, wq, Tb); have_b = i0; }
                    if (have_a != i1) { row_at(i1, at); hpass_row(at, wq, Ta); have_a = i1; }
                    vpass_store(Tb, Ta, b0s, b1s, dst, o, x0, oW);
                }
            }
        }
        return;
    }

    // direct path: taps straight from the frame, row by row
    const size_t limit = t.limit;
#pragma unroll 1
    for (int q = 0; q < rows; ++q) {
        const int y = ya + q;
        const ResizeTab yt = ytab[y];
        const uint32_t b0s = (yt.w & 0xFFFFu) << 8, b1s = (yt.w >> 16) << 8;
        const uint32_t row0 = (uint32_t)(top + (yt.ofs & 0xFFFF)) * (uint32_t)W + (uint32_t)left;
        const uint32_t row1 = (uint32_t)(top + (yt.ofs >> 16)) * (uint32_t)W + (uint32_t)left;
        const uint32_t o = ((uint32_t)y * (uint32_t)oW + (uint32_t)x0) * 3u;
        // Fast form: the lane's four pixels are inside the frame and every tap load stays inside the frame stack.
        // Where sx is the last column of the crop the second weight is 0, so whatever lies right of it may be read.
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

// The kernels: the rectangle (launch arguments, or loaded from device memory: resize_rect.h), then the tile.
// resize_kernel: the same-size call, the up instantiation at the frame's own size
__global__ __launch_bounds__(64 * kWaves) void resize_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, int n,
                                                     int W, int H, MF_RECT_ARGS,
                                                     const ResizeTab* __restrict__ xtab,
                                                     const ResizeTab* __restrict__ ytab, TileOrder order)
{
    MF_RECT_LOAD(W, H)
    resize_bgr_tile<kRows, kSrcRows, kRowPitch, false>(frames, out, n, W, H, left, top, cw, W, H, xtab, ytab, order);
}

template <int ROWS, int SLOTS, int PITCH, bool PAIRS>
__global__ __launch_bounds__(64 * kWaves) void resize_to_kernel(const uint8_t* __restrict__ frames, uint8_t* __restrict__ out, int n,
                                                                int W, int H, MF_RECT_ARGS, int oW, int oH,
                                                                const ResizeTab* __restrict__ xtab,
                                                                const ResizeTab* __restrict__ ytab, TileOrder order)
{
    MF_RECT_LOAD(W, H)
    resize_bgr_tile<ROWS, SLOTS, PITCH, PAIRS>(frames, out, n, W, H, left, top, cw, oW, oH, xtab, ytab, order);
}

}  // namespace mf

#endif  // MF_RESIZE_BODY_H
