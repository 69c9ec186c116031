// The device tracker's arithmetic (track_fast.hip, track_pyr.hip, track_lk.hip): sub-frame geometry, the reflect-101 border, the FAST arc
// score, the pyrDown taps, the LK weights and the float32 sequence behind each LK update -- every step as tests/track_model.py writes it,
// which is the specification (OpenCV's fast.cpp / pyramids.cpp / lkpyramid.cpp for CV_8UC1, with the five window sums taken exactly in
// integers).  Plain C++ behind MF_TRACK_HD, so the same functions compile for the host (tools/track_body_check.cpp runs them under the
// address and undefined-behaviour sanitizers against cases dumped from the model).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MF_TRACK_HD __host__ __device__ __forceinline__
#else
#define MF_TRACK_HD inline
#endif

namespace mf {
namespace track {

constexpr int WIN = 21;                 // calcOpticalFlowPyrLK's default window
constexpr int MAX_LEVEL = 3;            // ... and maxLevel
constexpr int W_BITS = 14;
constexpr int MAX_COUNT = 30;
constexpr int POSITIONS = WIN * WIN;    // 441 window positions = 7 per lane of a wavefront (the last lane group is partly idle)
constexpr int PER_LANE = 7;
constexpr int TILE = WIN + 3;           // 24: the early level's pixels under the 22 x 22 bilinear taps and their Scharr ring
constexpr int GRID = WIN + 1;           // 22: positions whose derivatives a window interpolates

// The sub-frame grid of mfs.py:492-516: ceil-sized sub-frames, left outer, top inner; the last column / row may be smaller, and there may
// be FEWER than sub_cols x sub_rows of them (range(0, W, ceil(W / cols))).
struct Geom { int W, H, sub_w, sub_h, ncols, nrows; };
struct Sub { int left, top, w, h; };

MF_TRACK_HD Geom make_geom(int W, int H, int sub_rows, int sub_cols)
{
    Geom g;
    g.W = W; g.H = H;
    g.sub_w = (W + sub_cols - 1) / sub_cols;
    g.sub_h = (H + sub_rows - 1) / sub_rows;
    g.ncols = (W + g.sub_w - 1) / g.sub_w;
    g.nrows = (H + g.sub_h - 1) / g.sub_h;
    return g;
}

MF_TRACK_HD Sub sub_of(const Geom& g, int s)
{
    Sub b;
    b.left = (s / g.nrows) * g.sub_w;
    b.top = (s % g.nrows) * g.sub_h;
    b.w = g.W - b.left < g.sub_w ? g.W - b.left : g.sub_w;
    b.h = g.H - b.top < g.sub_h ? g.H - b.top : g.sub_h;
    return b;
}

// cv::borderInterpolate(p, n, BORDER_REFLECT_101) (n >= 1, any p the tracker forms: |p| stays below n + 2 * WIN + 2)
MF_TRACK_HD int reflect101(int p, int n)
{
    if (n == 1) return 0;
    while (p < 0 || p >= n) p = p < 0 ? -p : 2 * (n - 1) - p;
    return p;
}

// size of pyramid level `level` of a w x h image
MF_TRACK_HD void level_size(int w, int h, int level, int& lw, int& lh)
{
    for (int l = 0; l < level; ++l) { w = (w + 1) / 2; h = (h + 1) / 2; }
    lw = w; lh = h;
}

// the top level buildOpticalFlowPyramid makes for a w x h image: it stops in front of a level not larger than the window
MF_TRACK_HD int top_level(int w, int h)
{
    int level = 0;
    while (level < MAX_LEVEL) {
        w = (w + 1) / 2; h = (h + 1) / 2;
        if (w <= WIN || h <= WIN) break;
        ++level;
    }
    return level;
}

MF_TRACK_HD int imin(int a, int b) { return a < b ? a : b; }
MF_TRACK_HD int imax(int a, int b) { return a > b ? a : b; }

// max over the 16 arcs of 9 contiguous circle pixels of min(d) and of min(-d), d[i] = centre - circle pixel i: the pixel is a corner at
// threshold t iff this exceeds t, and cornerScore<16> is then this minus one.  Sliding minima by doubling (2, 4, 8, then the ninth).
MF_TRACK_HD int fast_best(const int (&d)[16])
{
    int lo2[16], hi2[16], lo4[16], hi4[16], best = -255;
#pragma unroll
    for (int i = 0; i < 16; ++i) { lo2[i] = imin(d[i], d[(i + 1) & 15]); hi2[i] = imax(d[i], d[(i + 1) & 15]); }
#pragma unroll
    for (int i = 0; i < 16; ++i) { lo4[i] = imin(lo2[i], lo2[(i + 2) & 15]); hi4[i] = imax(hi2[i], hi2[(i + 2) & 15]); }
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int lo9 = imin(imin(lo4[i], lo4[(i + 4) & 15]), d[(i + 8) & 15]);
        const int hi9 = imax(imax(hi4[i], hi4[(i + 4) & 15]), d[(i + 8) & 15]);
        best = imax(best, imax(lo9, -hi9));
    }
    return best;
}

MF_TRACK_HD int pyr_taps(int a, int b, int c, int d, int e) { return a + e + 4 * (b + d) + 6 * c; }

MF_TRACK_HD int descale(int v, int bits) { return (v + (1 << (bits - 1))) >> bits; }

// cvFloor of a coordinate, saturating (a diverged track is then simply outside the image, as in the model's int64)
MF_TRACK_HD int floor_sat(float v)
{
    if (!(v > -1.0e9f)) return -1000000000;
    if (v > 1.0e9f) return 1000000000;
    return (int)floorf(v);
}

MF_TRACK_HD bool outside(int ix, int iy, int w, int h) { return ix < -WIN || ix >= w || iy < -WIN || iy >= h; }

struct Weights { int w00, w01, w10, w11; };

// cvRound((1 - a)(1 - b) 2^14) ..., the fourth as the remainder
MF_TRACK_HD Weights lk_weights(float a, float b)
{
    Weights w;
    const float scale = (float)(1 << W_BITS);
    w.w00 = (int)rintf((1.f - a) * (1.f - b) * scale);
    w.w01 = (int)rintf(a * (1.f - b) * scale);
    w.w10 = (int)rintf((1.f - a) * b * scale);
    w.w11 = (1 << W_BITS) - w.w00 - w.w01 - w.w10;
    return w;
}

MF_TRACK_HD int blend(const Weights& w, int v00, int v01, int v10, int v11, int bits)
{
    return descale(v00 * w.w00 + v01 * w.w01 + v10 * w.w10 + v11 * w.w11, bits);
}

MF_TRACK_HD float scaled_sum(long long s) { return (float)s * (1.f / (float)(1 << 20)); }       // one rounding, then FLT_SCALE (exact)

struct Matrix { float a11, a12, a22, inv; };

// the spatial gradient matrix from its three exact sums; false: rejected (minEig < 1e-4 or D < FLT_EPSILON)
MF_TRACK_HD bool lk_matrix(long long s11, long long s12, long long s22, Matrix& m)
{
    m.a11 = scaled_sum(s11); m.a12 = scaled_sum(s12); m.a22 = scaled_sum(s22);
    const float det = m.a11 * m.a22 - m.a12 * m.a12;
    const float diff = m.a11 - m.a22;
    const float min_eig = (m.a22 + m.a11 - sqrtf(diff * diff + 4.f * m.a12 * m.a12)) / (float)(2 * WIN * WIN);
    const bool ok = !((double)min_eig < 1e-4 || det < 1.1920929e-07f);
    m.inv = ok ? 1.f / det : 0.f;
    return ok;
}

MF_TRACK_HD void lk_delta(const Matrix& m, long long sb1, long long sb2, float& dx, float& dy)
{
    const float b1 = scaled_sum(sb1), b2 = scaled_sum(sb2);
    dx = (m.a12 * b2 - m.a22 * b1) * m.inv;
    dy = (m.a12 * b1 - m.a11 * b2) * m.inv;
}

// after an update: 1 = converged (|delta|^2 <= 0.01^2 in float64), 2 = "moved back by less than 0.01 twice" (take half a step back), 0 = go on
MF_TRACK_HD int lk_exit(float dx, float dy, float pdx, float pdy, int iteration)
{
    if ((double)dx * (double)dx + (double)dy * (double)dy <= 0.01 * 0.01) return 1;
    if (iteration > 0 && (double)fabsf(dx + pdx) < 0.01 && (double)fabsf(dy + pdy) < 0.01) return 2;
    return 0;
}

// ---- launch geometry shared by capi.hip's checks and the kernels' hosts ----
constexpr int FAST_OUT_W = 56, FAST_OUT_H = 14;          // pixels a 256-lane block decides: 14 x 14 of its 16 x 16 lanes, 4 pixels each
constexpr int FAST_LDS_W = 72, FAST_LDS_H = 22;          // ... their scores' 1-pixel ring (one more lane each side) + the 3-pixel circle
constexpr int PYR_OUT_W = 32, PYR_OUT_H = 8;
constexpr int PYR_ROWS = 2 * PYR_OUT_H + 3;              // source rows under a tile of the vertical pass

MF_TRACK_HD int mask_pitch(const Geom& g) { return (g.sub_w + 3) / 4; }        // bytes per sub-frame row: 4 corner flags per byte

}  // namespace track
}  // namespace mf
