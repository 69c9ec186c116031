// FAST corners (TYPE_9_16, non-maximum suppression) of every sub-frame of every image of a grey stack, each sub-frame an image of its own
// (mfs.py:505-516, 613): fast_detect_kernel marks the surviving corners in a mask, fast_compact_kernel writes them in row-major order.
//
// fast_detect_kernel: a block of 256 lanes = 16 x 16, each lane 4 adjacent pixels, scores a 64 x 16 patch from an LDS tile with the circle's
// 3-pixel halo; the outer ring of lanes only supplies the scores the suppression of the inner 14 x 14 lanes (56 x 14 pixels) compares
// with, so nothing is read from HBM twice and no score is ever stored there.  Tiles are clipped to the sub-frame: what lies outside it is
// never loaded and scores 0, like cv2's rows and columns within 3 pixels of an edge.  Each inner lane stores its 4 flags as one byte.
// fast_compact_kernel: one wavefront per (image, sub-frame); a lane counts one mask row, an exclusive scan over the rows gives each row its
// first slot, and the lane writes its row's corners from there -- the order is row-major by construction, no atomic takes part.
#include "track.h"

namespace mf {
using namespace track;

__global__ void __launch_bounds__(256) fast_detect_kernel(const uint8_t* __restrict__ grey, Geom g, int threshold, int tiles_x,
                                                          uint8_t* __restrict__ mask)
{
    __shared__ uint32_t tile[FAST_LDS_H][FAST_LDS_W / 4];
    __shared__ uint32_t scores[16][16];
    const int S = g.ncols * g.nrows, s = blockIdx.y, image = blockIdx.z;
    const Sub sb = sub_of(g, s);
    const int X0 = (int)(blockIdx.x % (unsigned)tiles_x) * FAST_OUT_W, Y0 = (int)(blockIdx.x / (unsigned)tiles_x) * FAST_OUT_H;
    if (X0 >= sb.w || Y0 >= sb.h) return;                                   // (the grid is sized for the largest sub-frame)
    const uint8_t* src = grey + ((size_t)image * g.H + sb.top) * g.W + sb.left;
    for (int t = threadIdx.x; t < FAST_LDS_H * (FAST_LDS_W / 4); t += 256) {
        const int r = t / (FAST_LDS_W / 4), c = t % (FAST_LDS_W / 4), y = Y0 - 4 + r;
        uint32_t word = 0;
        if (y >= 0 && y < sb.h) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int x = X0 - 8 + 4 * c + k;
                if (x >= 0 && x < sb.w) word |= (uint32_t)src[(size_t)y * g.W + x] << (8 * k);
            }
        }
        tile[r][c] = word;
    }
    __syncthreads();
    const int lx = threadIdx.x & 15, ly = threadIdx.x >> 4;
    const int x0 = X0 - 4 + 4 * lx, y = Y0 - 1 + ly;                         // this lane's 4 pixels: (x0 .. x0 + 3, y)
    uint32_t rows[7][3];                                                    // LDS columns 4 lx .. 4 lx + 11 of rows ly .. ly + 6
#pragma unroll
    for (int j = 0; j < 7; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) rows[j][c] = tile[ly + j][lx + c];
    constexpr int DX[16] = {0, 1, 2, 3, 3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1};
    constexpr int DY[16] = {3, 3, 2, 1, 0, -1, -2, -3, -3, -3, -2, -1, 0, 1, 2, 3};
    uint32_t packed = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int centre = (int)((rows[3][(4 + k) >> 2] >> (8 * ((4 + k) & 3))) & 255u);
        int d[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int col = 4 + k + DX[i], row = 3 + DY[i];
            d[i] = centre - (int)((rows[row][col >> 2] >> (8 * (col & 3))) & 255u);
        }
        const int best = fast_best(d), x = x0 + k;
        const bool inner = x >= 3 && x < sb.w - 3 && y >= 3 && y < sb.h - 3;
        packed |= (uint32_t)(inner && best > threshold ? best - 1 : 0) << (8 * k);
    }
    scores[ly][lx] = packed;
    __syncthreads();
    if (lx < 1 || lx > 14 || ly < 1 || ly > 14 || x0 >= sb.w || y >= sb.h) return;
    uint32_t n[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int c = 0; c < 3; ++c) n[j][c] = scores[ly - 1 + j][lx - 1 + c];
    uint32_t flags = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t mine = (packed >> (8 * k)) & 255u;
        bool keep = mine > 0;
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int c = -1; c <= 1; ++c) {
                if (j == 1 && c == 0) continue;
                const int col = 4 + k + c;                                  // column among the 12 of words lx - 1 .. lx + 1
                keep = keep && mine > ((n[j][col >> 2] >> (8 * (col & 3))) & 255u);
            }
        flags |= (uint32_t)keep << k;
    }
    mask[(((size_t)image * S + s) * g.sub_h + y) * mask_pitch(g) + (x0 >> 2)] = (uint8_t)flags;
}

__global__ void __launch_bounds__(64) fast_compact_kernel(const uint8_t* __restrict__ mask, Geom g, int max_per, float* __restrict__ points,
                                                          int32_t* __restrict__ counts, int32_t* __restrict__ status)
{
    const int S = g.ncols * g.nrows, s = blockIdx.x, image = blockIdx.y, lane = threadIdx.x;
    const Sub sb = sub_of(g, s);
    const int pitch = mask_pitch(g), used = (sb.w + 3) / 4;
    const size_t slot = (size_t)image * S + s;
    const uint8_t* base = mask + slot * g.sub_h * pitch;
    float2* out = (float2*)points + slot * max_per;
    int running = 0;
    for (int y0 = 0; y0 < sb.h; y0 += 64) {
        const int y = y0 + lane;
        const uint8_t* row = base + (size_t)y * pitch;
        int mine = 0;
        if (y < sb.h)
            for (int b = 0; b < used; ++b) mine += __popc((unsigned)row[b]);
        int incl = mine;
#pragma unroll
        for (int step = 1; step < 64; step <<= 1) {
            const int up = __shfl_up(incl, step);
            if (lane >= step) incl += up;
        }
        int at = running + incl - mine;
        if (mine > 0)
            for (int b = 0; b < used && at < max_per; ++b) {
                const unsigned bits = row[b];
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (((bits >> k) & 1u) && at < max_per) out[at++] = make_float2((float)(4 * b + k), (float)y);
            }
        running += __shfl(incl, 63);
    }
    if (lane == 0) {
        counts[slot] = running;
        status[slot] = running > max_per ? MF_TRACK_OVERFLOW : 0;
    }
}

size_t track_mask_bytes(const Geom& g, int n)
{
    return (size_t)n * g.ncols * g.nrows * g.sub_h * mask_pitch(g);
}

int launch_fast_corners(const uint8_t* grey, int n, const Geom& g, int max_per, int threshold, float* points, int32_t* counts,
                        int32_t* status, void* work, hipStream_t st)
{
    const int S = g.ncols * g.nrows;
    const int tiles_x = (g.sub_w + FAST_OUT_W - 1) / FAST_OUT_W, tiles_y = (g.sub_h + FAST_OUT_H - 1) / FAST_OUT_H;
    hipLaunchKernelGGL(fast_detect_kernel, dim3(tiles_x * tiles_y, S, n), dim3(256), 0, st, grey, g, threshold, tiles_x, (uint8_t*)work);
    MF_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(fast_compact_kernel, dim3(S, n), dim3(64), 0, st, (const uint8_t*)work, g, max_per, points, counts, status);
    MF_HIP_TRY(hipGetLastError());
    return MF_OK;
}

}  // namespace mf
