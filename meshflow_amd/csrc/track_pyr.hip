// The LK pyramid of every sub-frame of both stacks (early and late) of a chunk of frame pairs: cv2.pyrDown's separable [1 4 6 4 1] in
// integers, (sum + 128) >> 8, BORDER_REFLECT_101 at the SUB-FRAME's edges (each sub-frame is an image of its own), one launch per level.
// Level 0 is the frames themselves and is never copied; levels 1-3 live in the workspace, one sub-image per (stack, pair, sub-frame) at the
// size of the largest sub-frame's level.  A sub-frame makes only the levels buildOpticalFlowPyramid would make for it (track_body.h,
// top_level): blocks of the others leave at once.
// pyr_down_kernel: a block of 256 lanes makes 32 x 8 output pixels: the horizontal pass of the 19 source rows under them goes to LDS (sums
// up to 16 x 255), the vertical pass reads five of those per pixel.
#include "track.h"

namespace mf {
using namespace track;

struct PyrLevel { size_t offset; int pitch, rows; };

static PyrLevel pyr_level(const Geom& g, int n_pairs, int level)
{
    PyrLevel p = {0, 0, 0};
    size_t at = 0;
    for (int l = 1; l <= level; ++l) {
        level_size(g.sub_w, g.sub_h, l, p.pitch, p.rows);
        p.offset = at;
        at += (size_t)2 * n_pairs * g.ncols * g.nrows * p.pitch * p.rows;
        at = align16(at);
    }
    return p;
}

size_t track_pyramid_bytes(const Geom& g, int n_pairs)
{
    const PyrLevel last = pyr_level(g, n_pairs, MAX_LEVEL);
    return align16(last.offset + (size_t)2 * n_pairs * g.ncols * g.nrows * last.pitch * last.rows);
}

size_t track_level_offset(const Geom& g, int n_pairs, int level) { return pyr_level(g, n_pairs, level).offset; }

// src_pitch == 0: the source level is the frames (level 0): sub-image j = (stack, pair, sub-frame) is a window of frame `pair` of its stack
__global__ void __launch_bounds__(256) pyr_down_kernel(const uint8_t* __restrict__ src0, const uint8_t* __restrict__ src1, int src_pitch,
                                                       int src_rows, Geom g, int n_pairs, int level, int tiles_x, uint8_t* __restrict__ dst,
                                                       int dst_pitch, int dst_rows)
{
    __shared__ uint16_t sums[PYR_ROWS][PYR_OUT_W];
    const int S = g.ncols * g.nrows, j = blockIdx.y, s = j % S, pair = (j / S) % n_pairs, stack = j / (S * n_pairs);
    const Sub sb = sub_of(g, s);
    if (level > top_level(sb.w, sb.h)) return;
    int sw, sh, dw, dh;
    level_size(sb.w, sb.h, level - 1, sw, sh);
    level_size(sb.w, sb.h, level, dw, dh);
    const int ox0 = (int)(blockIdx.x % (unsigned)tiles_x) * PYR_OUT_W, oy0 = (int)(blockIdx.x / (unsigned)tiles_x) * PYR_OUT_H;
    if (ox0 >= dw || oy0 >= dh) return;
    const uint8_t* src;
    int pitch;
    if (src_pitch == 0) {
        src = (stack ? src1 : src0) + ((size_t)pair * g.H + sb.top) * g.W + sb.left;
        pitch = g.W;
    } else {
        src = src0 + (size_t)j * src_pitch * src_rows;
        pitch = src_pitch;
    }
    for (int t = threadIdx.x; t < PYR_ROWS * PYR_OUT_W; t += 256) {
        const int r = t / PYR_OUT_W, c = t % PYR_OUT_W, ox = ox0 + c;
        if (ox >= dw) continue;
        const uint8_t* row = src + (size_t)reflect101(2 * oy0 - 2 + r, sh) * pitch;
        sums[r][c] = (uint16_t)pyr_taps(row[reflect101(2 * ox - 2, sw)], row[reflect101(2 * ox - 1, sw)], row[2 * ox],
                                        row[reflect101(2 * ox + 1, sw)], row[reflect101(2 * ox + 2, sw)]);
    }
    __syncthreads();
    const int c = threadIdx.x % PYR_OUT_W, r = threadIdx.x / PYR_OUT_W, ox = ox0 + c, oy = oy0 + r;
    if (ox >= dw || oy >= dh) return;
    const int v = pyr_taps(sums[2 * r][c], sums[2 * r + 1][c], sums[2 * r + 2][c], sums[2 * r + 3][c], sums[2 * r + 4][c]);
    dst[(size_t)j * dst_pitch * dst_rows + (size_t)oy * dst_pitch + ox] = (uint8_t)((v + 128) >> 8);
}

int launch_pyramid(const uint8_t* early, const uint8_t* late, int n_pairs, const Geom& g, void* work, hipStream_t st)
{
    const int S = g.ncols * g.nrows;
    for (int level = 1; level <= MAX_LEVEL; ++level) {
        if (level > top_level(g.sub_w, g.sub_h)) break;                     // (no sub-frame is larger than the first)
        const PyrLevel d = pyr_level(g, n_pairs, level), p = pyr_level(g, n_pairs, level - 1);
        const int tiles_x = (d.pitch + PYR_OUT_W - 1) / PYR_OUT_W, tiles_y = (d.rows + PYR_OUT_H - 1) / PYR_OUT_H;
        const uint8_t* s0 = level == 1 ? early : (const uint8_t*)work + p.offset;
        hipLaunchKernelGGL(pyr_down_kernel, dim3(tiles_x * tiles_y, 2 * n_pairs * S), dim3(256), 0, st, s0, late, level == 1 ? 0 : p.pitch,
                           p.rows, g, n_pairs, level, tiles_x, (uint8_t*)work + d.offset, d.pitch, d.rows);
        MF_HIP_TRY(hipGetLastError());
    }
    return MF_OK;
}

}  // namespace mf
