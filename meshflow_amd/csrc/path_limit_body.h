// The path limiter's predicates, the same on host and device: float64, every operation rounded by itself (tests/path_limit_model.py; the
// library is built with -ffp-contract=off, so a product and the sum it feeds are two roundings here as there).
//   polygon   the mesh's perimeter, B = 2 (R + C) vertices: row 0 from column 0 to C-1, column C from row 0 to R-1, row R from column C down
//             to 1, column 0 from row R down to 1; edge e joins vertex e to vertex (e + 1) mod B
//   vertex    at candidate k: g + f * d, f = (double)k / (double)K, d = p - c, g the integer vertex grid (cell_table_kernel's)
//   clear     an edge is clear of the rectangle [x0, x1] x [y0, y1] when its bounding box is disjoint from it, or the four corners' cross
//             products are all > 0, or all < 0
//   crossing  an edge counts for the centre's rightward ray iff it straddles cy and s has the sign of by - ay
// Every comparison is affirmative: a NaN makes none of them true, so no edge is clear and no edge counts because of one.
#pragma once
#include <stdint.h>

namespace mf {
namespace plimit {

constexpr int LANES = 64;                   // one wavefront per frame; lane j tests candidate j + 1
constexpr int MAX_STEPS = 64;
constexpr int MAX_BOUNDARY = 1024;          // 32 bytes of LDS per boundary vertex

struct Rect { double x0, y0, x1, y1, cx, cy; };

__host__ __device__ inline Rect guarded(int left, int top, int right, int bottom, double guard)
{
    Rect r;
    r.x0 = (double)left - guard; r.x1 = (double)right + guard;
    r.y0 = (double)top - guard; r.y1 = (double)bottom + guard;
    r.cx = (r.x0 + r.x1) * 0.5; r.cy = (r.y0 + r.y1) * 0.5;
    return r;
}

// (row, col) of boundary vertex e, 0 <= e < 2 (R + C)
__host__ __device__ inline void walk(int e, int R, int C, int& row, int& col)
{
    if (e < C) { row = 0; col = e; }
    else if (e < C + R) { row = e - C; col = C; }
    else if (e < 2 * C + R) { row = R; col = C - (e - C - R); }
    else { row = R - (e - 2 * C - R); col = 0; }
}

__host__ __device__ inline double grid_at(int i, int cells, int size) { return ceil((double)(size - 1) * ((double)i / (double)cells)); }

__host__ __device__ inline double lesser(double a, double b) { return a < b ? a : b; }
__host__ __device__ inline double greater(double a, double b) { return a > b ? a : b; }

__host__ __device__ inline double cross(double ex, double ey, double ax, double ay, double px, double py) { return ex * (py - ay) - ey * (px - ax); }

__host__ __device__ inline bool edge_clear(double ax, double ay, double bx, double by, const Rect& r)
{
    // (int, not bool: the verdicts are combined, not branched on)
    const int apart = (int)(lesser(ax, bx) > r.x1) | (int)(greater(ax, bx) < r.x0) | (int)(lesser(ay, by) > r.y1) | (int)(greater(ay, by) < r.y0);
    const double ex = bx - ax, ey = by - ay;
    const double c0 = cross(ex, ey, ax, ay, r.x0, r.y0), c1 = cross(ex, ey, ax, ay, r.x1, r.y0);
    const double c2 = cross(ex, ey, ax, ay, r.x1, r.y1), c3 = cross(ex, ey, ax, ay, r.x0, r.y1);
    const int left_of = (int)(c0 > 0.0) & (int)(c1 > 0.0) & (int)(c2 > 0.0) & (int)(c3 > 0.0);
    const int right_of = (int)(c0 < 0.0) & (int)(c1 < 0.0) & (int)(c2 < 0.0) & (int)(c3 < 0.0);
    return (apart | left_of | right_of) != 0;
}

__host__ __device__ inline bool edge_counts(double ax, double ay, double bx, double by, const Rect& r)
{
    const double s = cross(bx - ax, by - ay, ax, ay, r.cx, r.cy);
    const bool up = by > ay;
    return (((int)(ay > r.cy) ^ (int)(by > r.cy)) & (int)(up ? s > 0.0 : s < 0.0)) != 0;
}

// the trailing passes of a ballot whose bit j is candidate j + 1's verdict: k_raw
__host__ __device__ inline int leading_passes(uint64_t verdicts)
{
    return ~verdicts == 0 ? 64 : __builtin_ctzll(~verdicts);
}

}  // namespace plimit
}  // namespace mf
