// Pyramidal Lucas-Kanade (cv2.calcOpticalFlowPyrLK's defaults: 21 x 21 window, 4 levels, 30 iterations or eps 0.01, minEigThreshold 1e-4)
// for every corner of every sub-frame of a chunk of frame pairs, each sub-frame an image of its own: one launch per pyramid level, top
// first, one wavefront per feature.  The feature's position and its "found" flag travel from level to level in the outputs themselves.
//
// lk_level_kernel: the 441 window positions are spread over the 64 lanes, 7 each; the early patch I and its interpolated derivatives Ix, Iy
// stay in registers across the iterations.  The derivatives are NOT read from a stored int16 level: the wavefront stages the 24 x 24 early
// pixels under its window in LDS (reflect-101 at the sub-frame's edges, like cv2's bordered level), takes the Scharr derivative of the 22 x
// 22 positions the window interpolates from there (zero outside the image, like cv2's zero-padded derivative image) and keeps those as
// int16 pairs in LDS for the one interpolation that follows.  A stored derivative level would cost 4 bytes per pixel and level of workspace
// and an extra pass over HBM to be read exactly once per window; the tile costs 2.5 KB of LDS and ~8 Scharr taps per lane and level.
// Per-lane partial sums fit int32 (7 x 4080^2, 7 x 8160 x 4080 < 2^31); lanes are reduced in int64, so every lane holds the exact sums and
// computes the same float32 update: the iteration loop is wave-uniform.  The late level is gathered tap by tap (it is L2-resident), each
// tap placed by the same window test and reflect-101 rule the model uses -- no pointer is clamped.
#include "track.h"

namespace mf {
using namespace track;

__device__ __forceinline__ long long wave_sum(int v)
{
    long long s = v;
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) s += __shfl_xor(s, step);
    return s;
}

__device__ __forceinline__ float uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

__global__ void __launch_bounds__(64) lk_level_kernel(const uint8_t* __restrict__ early, const uint8_t* __restrict__ late, int pitch, int rows,
                                                      Geom g, int n_pairs, int level, int max_per, const float* __restrict__ points,
                                                      const int32_t* __restrict__ counts, float* __restrict__ moved, uint8_t* __restrict__ found)
{
    __shared__ uint8_t tile[TILE][TILE];
    __shared__ uint32_t deriv[GRID][GRID];                                   // Ix | Iy << 16, int16 each
    const int S = g.ncols * g.nrows, slot = blockIdx.y, s = slot % S, pair = slot / S, k = blockIdx.x, lane = threadIdx.x;
    if (k >= counts[slot]) return;                                          // (k < max_per: the grid's width)
    const Sub sb = sub_of(g, s);
    const int top = top_level(sb.w, sb.h);
    if (level > top) return;
    int lw, lh;
    level_size(sb.w, sb.h, level, lw, lh);
    const uint8_t *I, *J;
    int row_pitch;
    if (level == 0) {
        const size_t at = ((size_t)pair * g.H + sb.top) * g.W + sb.left;
        I = early + at; J = late + at; row_pitch = g.W;
    } else {                                                                 // `early`: this level's sub-images, early stack then late stack
        I = early + (size_t)slot * pitch * rows;
        J = early + ((size_t)n_pairs * S + slot) * pitch * rows;
        row_pitch = pitch;
    }
    const size_t feature = (size_t)slot * max_per + k;
    const float scale = 1.f / (float)(1 << level);
    const float px = points[2 * feature] * scale, py = points[2 * feature + 1] * scale;
    float nx = px, ny = py;
    int ok = 1;
    if (level != top) { nx = moved[2 * feature] * 2.f; ny = moved[2 * feature + 1] * 2.f; ok = found[feature]; }
    const float hx = px - 10.f, hy = py - 10.f;
    const int ix = floor_sat(hx), iy = floor_sat(hy);
    bool tracking = __builtin_amdgcn_readfirstlane((int)!outside(ix, iy, lw, lh)) != 0;      // (the same in every lane: the barriers below)
    Matrix m = {0.f, 0.f, 0.f, 0.f};
    int wx[PER_LANE] = {}, wy[PER_LANE] = {}, Iv[PER_LANE] = {}, Ixv[PER_LANE] = {}, Iyv[PER_LANE] = {};
    if (tracking) {
        for (int t = lane; t < TILE * TILE; t += 64) {
            const int r = t / TILE, c = t % TILE;
            tile[r][c] = I[(size_t)reflect101(iy - 1 + r, lh) * row_pitch + reflect101(ix - 1 + c, lw)];
        }
        __syncthreads();
        for (int t = lane; t < GRID * GRID; t += 64) {
            const int r = t / GRID, c = t % GRID;                           // position (ix + c, iy + r): tile[r + 1][c + 1]
            int dx = 0, dy = 0;
            if (ix + c >= 0 && ix + c < lw && iy + r >= 0 && iy + r < lh) {
                int t0[3], t1[3];
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const int a = tile[r][c + q], b = tile[r + 1][c + q], e = tile[r + 2][c + q];
                    t0[q] = (a + e) * 3 + b * 10;
                    t1[q] = e - a;
                }
                dx = t0[2] - t0[0];
                dy = (t1[0] + t1[2]) * 3 + t1[1] * 10;
            }
            deriv[r][c] = ((uint32_t)dx & 0xFFFFu) | ((uint32_t)dy << 16);
        }
        __syncthreads();
        const Weights w = lk_weights(hx - (float)ix, hy - (float)iy);
        int s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
        for (int i = 0; i < PER_LANE; ++i) {
            const int q = lane + 64 * i;
            const bool live = q < POSITIONS;
            wy[i] = live ? q / WIN : 0;
            wx[i] = live ? q % WIN : 0;
            const int r = wy[i], c = wx[i];
            Iv[i] = blend(w, tile[r + 1][c + 1], tile[r + 1][c + 2], tile[r + 2][c + 1], tile[r + 2][c + 2], W_BITS - 5);
            const uint32_t d00 = deriv[r][c], d01 = deriv[r][c + 1], d10 = deriv[r + 1][c], d11 = deriv[r + 1][c + 1];
            const int gx = blend(w, (int16_t)d00, (int16_t)d01, (int16_t)d10, (int16_t)d11, W_BITS);
            const int gy = blend(w, (int32_t)d00 >> 16, (int32_t)d01 >> 16, (int32_t)d10 >> 16, (int32_t)d11 >> 16, W_BITS);
            Ixv[i] = live ? gx : 0;
            Iyv[i] = live ? gy : 0;
            s11 += Ixv[i] * Ixv[i]; s12 += Ixv[i] * Iyv[i]; s22 += Iyv[i] * Iyv[i];
        }
        tracking = lk_matrix(wave_sum(s11), wave_sum(s12), wave_sum(s22), m);
    }
    tracking = __builtin_amdgcn_readfirstlane((int)tracking) != 0;
    if (!tracking) {
        if (level == 0) ok = 0;
    } else {
        float fx = uniform(nx - 10.f), fy = uniform(ny - 10.f), pdx = 0.f, pdy = 0.f;
        for (int it = 0; it < MAX_COUNT; ++it) {
            const int jx = floor_sat(fx), jy = floor_sat(fy);
            if (outside(jx, jy, lw, lh)) {
                if (level == 0) ok = 0;
                break;
            }
            const Weights w = lk_weights(fx - (float)jx, fy - (float)jy);
            int sb1 = 0, sb2 = 0;
#pragma unroll
            for (int i = 0; i < PER_LANE; ++i) {
                const uint8_t* r0 = J + (size_t)reflect101(jy + wy[i], lh) * row_pitch;
                const uint8_t* r1 = J + (size_t)reflect101(jy + wy[i] + 1, lh) * row_pitch;
                const int c0 = reflect101(jx + wx[i], lw), c1 = reflect101(jx + wx[i] + 1, lw);
                const int diff = blend(w, r0[c0], r0[c1], r1[c0], r1[c1], W_BITS - 5) - Iv[i];
                sb1 += diff * Ixv[i]; sb2 += diff * Iyv[i];                 // (Ixv = Iyv = 0 in the idle positions of the last lane group)
            }
            float dx, dy;
            lk_delta(m, wave_sum(sb1), wave_sum(sb2), dx, dy);
            dx = uniform(dx); dy = uniform(dy);
            fx = fx + dx; fy = fy + dy;
            nx = fx + 10.f; ny = fy + 10.f;
            const int leave = lk_exit(dx, dy, pdx, pdy, it);
            if (leave == 2) { nx = nx - dx * 0.5f; ny = ny - dy * 0.5f; }
            if (leave) break;
            pdx = dx; pdy = dy;
        }
    }
    // the bounds test in front of cv2's error measure, on the final position
    if (level == 0 && ok && outside(floor_sat(nx - 10.f), floor_sat(ny - 10.f), lw, lh)) ok = 0;
    if (lane == 0) {
        moved[2 * feature] = nx;
        moved[2 * feature + 1] = ny;
        found[feature] = (uint8_t)ok;
    }
}

int launch_lk_levels(const uint8_t* early, const uint8_t* late, int n_pairs, const Geom& g, int max_per, const float* points,
                     const int32_t* counts, float* moved, uint8_t* found, const void* work, hipStream_t st)
{
    const int S = g.ncols * g.nrows;
    for (int level = top_level(g.sub_w, g.sub_h); level >= 0; --level) {
        int pitch = 0, rows = 0;
        if (level > 0) level_size(g.sub_w, g.sub_h, level, pitch, rows);
        const uint8_t* e = level ? (const uint8_t*)work + track_level_offset(g, n_pairs, level) : early;
        hipLaunchKernelGGL(lk_level_kernel, dim3(max_per, n_pairs * S), dim3(64), 0, st, e, late, pitch, rows, g, n_pairs, level, max_per, points,
                           counts, moved, found);
        MF_HIP_TRY(hipGetLastError());
    }
    return MF_OK;
}

}  // namespace mf
