// The device outlier step's arithmetic (track_ransac.hip): the sample hash, the draw of four distinct candidates, the degenerate-sample
// test, the closed-form 4-point fit, the division-free error test and the iteration rule -- every step as tests/ransac_model.py writes it,
// which is the specification.  Only float64 + - * /, comparisons and integers, in the order written here: no libm, no reduction of floats,
// and (the library is built with -ffp-contract=off) no fused multiply-add.  Plain C++ behind MF_RANSAC_HD, so the same functions compile for
// the host (tools/ransac_body_check.cpp runs them under the address and undefined-behaviour sanitizers against cases dumped from the model).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MF_RANSAC_HD __host__ __device__ __forceinline__
#else
#define MF_RANSAC_HD inline
#endif

namespace mf {
namespace ransac {

constexpr int OK = 0, TOO_FEW = 1, NO_CONSENSUS = 2;      // d_info[..][0]
constexpr int DRAWS = 16;                                  // hash draws per iteration; the sample is the first four distinct ones
constexpr int STAGED = 1024;                               // candidates a wavefront keeps in LDS (16 bytes each); more are read from the workspace
constexpr int MAX_ITERS_LIMIT = 65536;
constexpr int SQUARINGS = 16;                              // the iteration rule's binary descent covers n < 2^17
constexpr int OVERSAMPLE = 3;                              // ... and the search runs three times as long as cv2's rule asks

// synthetic.hash32: the murmur3 finaliser over a counter and a seed
MF_RANSAC_HD uint32_t hash32(uint32_t idx, uint32_t seed)
{
    uint32_t z = idx + seed * 0x9E3779B1u;
    z = (z ^ (z >> 16)) * 0x85EBCA6Bu;
    z = (z ^ (z >> 13)) * 0xC2B2AE35u;
    return z ^ (z >> 16);
}

// The sample of iteration `it` among k >= 1 candidates: hash32(16 it + j, seed) % k for j = 0 .. 15, the first four distinct values in draw
// order; false where the 16 draws hold fewer than four distinct values.  Stateless: no iteration depends on the draws of another.
MF_RANSAC_HD bool draw_sample(uint32_t it, uint32_t seed, uint32_t k, int (&s)[4])
{
    int n = 0;
    s[0] = s[1] = s[2] = s[3] = -1;
#pragma unroll
    for (int j = 0; j < DRAWS; ++j) {
        const int v = (int)(hash32((uint32_t)DRAWS * it + (uint32_t)j, seed) % k);
        const bool fresh = n < 4 && v != s[0] && v != s[1] && v != s[2] && v != s[3];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (fresh && q == n) s[q] = v;
        n += fresh ? 1 : 0;
    }
    return n == 4;
}

MF_RANSAC_HD double dabs(double v) { return __builtin_fabs(v); }

// finite: v - v is 0 for a number and NaN for an infinity or a NaN
MF_RANSAC_HD bool finite(double v) { return v - v == 0.0; }

// host._degenerate_sample: three of the four points on one line (cv2's checkSubset), the right-hand sum parenthesised per difference
MF_RANSAC_HD bool degenerate4(const double (&p)[4][2])
{
    const int T[4][3] = {{0, 1, 2}, {0, 1, 3}, {0, 2, 3}, {1, 2, 3}};
    bool bad = false;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int i = T[t][0], j = T[t][1], k = T[t][2];
        const double d1x = p[j][0] - p[i][0], d1y = p[j][1] - p[i][1], d2x = p[k][0] - p[i][0], d2y = p[k][1] - p[i][1];
        const double cross = d1x * d2y - d1y * d2x;
        bad = bad || dabs(cross) <= 1.1920929e-07 * ((dabs(d1x) + dabs(d1y)) + (dabs(d2x) + dabs(d2y)));
    }
    return bad;
}

// Heckbert's unit square (0,0), (1,0), (1,1), (0,1) -> p[0], p[1], p[2], p[3], row-major {a, b, c, d, e, f, g, h, 1} (cell_table.hip's
// square_to_quad without its threshold: a vanishing denominator shows as a non-finite entry)
MF_RANSAC_HD void square_to_quad(const double (&p)[4][2], double (&S)[9])
{
    const double sx = ((p[0][0] - p[1][0]) + p[2][0]) - p[3][0];
    const double sy = ((p[0][1] - p[1][1]) + p[2][1]) - p[3][1];
    const double dx1 = p[1][0] - p[2][0], dx2 = p[3][0] - p[2][0];
    const double dy1 = p[1][1] - p[2][1], dy2 = p[3][1] - p[2][1];
    const double den = dx1 * dy2 - dx2 * dy1;
    const double g = (sx * dy2 - dx2 * sy) / den;
    const double h = (dx1 * sy - sx * dy1) / den;
    S[0] = (p[1][0] - p[0][0]) + g * p[1][0]; S[1] = (p[3][0] - p[0][0]) + h * p[3][0]; S[2] = p[0][0];
    S[3] = (p[1][1] - p[0][1]) + g * p[1][1]; S[4] = (p[3][1] - p[0][1]) + h * p[3][1]; S[5] = p[0][1];
    S[6] = g; S[7] = h; S[8] = 1.0;
}

// adjugate of a row-major 3 x 3 whose last entry is 1
MF_RANSAC_HD void adjugate3(const double (&S)[9], double (&A)[9])
{
    const double a = S[0], b = S[1], c = S[2], d = S[3], e = S[4], f = S[5], g = S[6], h = S[7];
    A[0] = e - f * h; A[1] = c * h - b; A[2] = b * f - c * e;
    A[3] = f * g - d; A[4] = a - c * g; A[5] = c * d - a * f;
    A[6] = d * h - e * g; A[7] = b * g - a * h; A[8] = a * e - b * d;
}

// H = S2Q(late) adj(S2Q(early)), every entry a left-to-right sum of three products; neither scaled to h22 = 1 nor normalised.  false where
// an entry is not finite.
MF_RANSAC_HD bool fit4(const double (&early)[4][2], const double (&late)[4][2], double (&H)[9])
{
    double Se[9], Sl[9], A[9];
    square_to_quad(early, Se);
    square_to_quad(late, Sl);
    adjugate3(Se, A);
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            double s = Sl[i * 3 + 0] * A[0 * 3 + j];
            s = s + Sl[i * 3 + 1] * A[1 * 3 + j];
            s = s + Sl[i * 3 + 2] * A[2 * 3 + j];
            H[i * 3 + j] = s;
            ok = ok && finite(s);
        }
    return ok;
}

// |H (x, y, 1) - w (lx, ly)|^2 <= threshold^2 w^2 with w the third coordinate: the reprojection test multiplied through by w^2, so the
// sign and scale of H do not matter and nothing is divided.  A NaN anywhere compares false.
MF_RANSAC_HD bool is_inlier(const double (&H)[9], double x, double y, double lx, double ly, double threshold_sq)
{
    const double X = (H[0] * x + H[1] * y) + H[2];
    const double Y = (H[3] * x + H[4] * y) + H[5];
    const double w = (H[6] * x + H[7] * y) + H[8];
    const double rx = X - lx * w, ry = Y - ly * w;
    const double ww = w * w;
    return ww > 0.0 && rx * rx + ry * ry <= threshold_sq * ww;
}

// n = the largest count with (1 - (c / k)^4)^n > 1 - confidence, by greedy binary descent over repeated squares: n + 1 is cv2's
// RANSACUpdateNumIters -- the iterations after which a sample free of outliers has been drawn with probability `confidence` when c of k
// candidates are inliers -- without log or pow.  The result is 3 n + 1: such a sample is necessary for a good hypothesis, not sufficient
// (four noisy points fix H well only where they lie far apart), and the consensus set is never refitted.  That explains a factor above 1;
// the 3 itself is empirical, chosen on the planted recipe of tests/test_ransac_model.py (tests/ransac_model.py has the figures).  In 1 ..
// max_iters; 1 at c = k.
MF_RANSAC_HD int iterations_needed(int c, int k, double confidence, int max_iters)
{
    const double w = (double)c / (double)k;
    const double q = 1.0 - (w * w) * (w * w);
    const double p1 = 1.0 - confidence;
    double P[SQUARINGS + 1];
    P[0] = q;
#pragma unroll
    for (int j = 0; j < SQUARINGS; ++j) P[j + 1] = P[j] * P[j];
    int n = 0;
    double r = 1.0;
#pragma unroll
    for (int j = SQUARINGS; j >= 0; --j) {
        const double t = r * P[j];
        if (t > p1) { r = t; n += 1 << j; }
    }
    return OVERSAMPLE * n + 1 < max_iters ? OVERSAMPLE * n + 1 : max_iters;
}

}  // namespace ransac
}  // namespace mf
