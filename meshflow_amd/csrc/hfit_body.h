// The device homography fit's arithmetic (track_fit.hip): the per-point terms of the three passes, the collinearity test, the similarity, the
// 9 x 9 normal matrix from its 24 sums, one Jacobi rotation as the lane of column k applies it, the choice of the eigenvector and the way
// back to pixel coordinates -- every step as tests/homography_model.py writes it, which is the specification.  Only float64 + - * /, sqrt,
// comparisons and integers, in the order written here, and (the library is built with -ffp-contract=off) no fused multiply-add.  The ORDER
// OF THE SUMS over a pair's points is the caller's: 256 strided partials, a halving tree per 64, (w0 + w1) + (w2 + w3).  Plain C++ behind
// MF_HFIT_HD, so the same functions compile for the host (tools/hfit_body_check.cpp runs them under the address and undefined-behaviour
// sanitizers against cases dumped from the model).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MF_HFIT_HD __host__ __device__ __forceinline__
#else
#define MF_HFIT_HD inline
#endif

namespace mf {
namespace hfit {

constexpr int OK = 0, TOO_FEW = 1, COLLINEAR = 2, AT_INFINITY = 3, NOT_CONVERGED = 4;     // d_info[..][0]
constexpr int LANES = 256, WAVE = 64;                      // partial sums per pair; partials per halving tree
constexpr int MAX_SWEEPS = 30;
constexpr int MOMENTS = 8, SUMS = 23;                      // ordered sums of the second and of the third pass (the 24th normal sum is K)
constexpr int MAX_PAIRS = 32767;                           // the tracker's own limit: 2 * n_pairs * sub-frames <= 65,535
constexpr double SQRT2 = 1.4142135623730951;
constexpr double EPS = 1.1102230246251565e-16;             // 2^-53

MF_HFIT_HD double dabs(double v) { return __builtin_fabs(v); }
// correctly rounded on both sides: the device's sqrt() as vertex_motion.hip uses it (no fast math), the host's IEEE instruction
MF_HFIT_HD double root(double v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return ::sqrt(v);
#else
    return __builtin_sqrt(v);
#endif
}

// second pass, one point: distance to the centroid and the centred second moments of both clouds
MF_HFIT_HD void moment_terms(double ex, double ey, double lx, double ly, const double (&c)[4], double (&t)[MOMENTS])
{
    const double dex = ex - c[0], dey = ey - c[1], dlx = lx - c[2], dly = ly - c[3];
    t[0] = root(dex * dex + dey * dey); t[1] = dex * dex; t[2] = dex * dey; t[3] = dey * dey;
    t[4] = root(dlx * dlx + dly * dly); t[5] = dlx * dlx; t[6] = dlx * dly; t[7] = dly * dly;
}

// host._collinear on the centred second moments [[a, b], [b, c]]: smaller eigenvalue <= 1e-18 max(larger, 1), without a division.  A NaN
// anywhere is collinear.
MF_HFIT_HD bool collinear(double a, double b, double c)
{
    const double half = (a + c) * 0.5, diff = (a - c) * 0.5;
    const double big = half + root(diff * diff + b * b);
    const double det = a * c - b * b;
    return !(det > (1e-18 * (big > 1.0 ? big : 1.0)) * big);
}

// host._normalisation of both clouds: sim = {s_early, s_late, tx_e, ty_e, tx_l, ty_l} from the sums of distances and the centroids
MF_HFIT_HD void translations(const double (&c)[4], double (&sim)[6])
{
    sim[2] = -(sim[0] * c[0]); sim[3] = -(sim[0] * c[1]); sim[4] = -(sim[1] * c[2]); sim[5] = -(sim[1] * c[3]);
}

MF_HFIT_HD void similarity(double dist_e, double dist_l, double kf, const double (&c)[4], double (&sim)[6])
{
    sim[0] = SQRT2 / (dist_e / kf); sim[1] = SQRT2 / (dist_l / kf);
    translations(c, sim);
}

// third pass, one point: q = (xx, xy, yy, x, y), u q, u, v q, v, w q, w in normalised coordinates
MF_HFIT_HD void normal_terms(double ex, double ey, double lx, double ly, const double (&sim)[6], double (&t)[SUMS])
{
    const double x = ex * sim[0] + sim[2], y = ey * sim[0] + sim[3], u = lx * sim[1] + sim[4], v = ly * sim[1] + sim[5];
    const double w = u * u + v * v;
    t[0] = x * x; t[1] = x * y; t[2] = y * y; t[3] = x; t[4] = y;
#pragma unroll
    for (int i = 0; i < 5; ++i) { t[5 + i] = u * t[i]; t[11 + i] = v * t[i]; t[17 + i] = w * t[i]; }
    t[10] = u; t[16] = v; t[22] = w;
}

// entry (i, j) of the 9 x 9 normal matrix from the 23 sums and K
MF_HFIT_HD double normal_entry(const double* sums, double kf, int i, int j)
{
    const int bi = i / 3, bj = j / 3, a = i % 3, b = j % 3;
    // S(f p p^T)[a][b] sits at {0, 1, 3; 1, 2, 4; 3, 4, 5} of the block's six sums
    const int at = a + b == 0 ? 0 : a + b == 1 ? 1 : a + b == 4 ? 5 : a + b == 3 ? 4 : (a == 1 ? 2 : 3);
    if (bi == bj) {
        if (bi == 2) return sums[17 + at];
        return at == 5 ? kf : sums[at];
    }
    const int lo = bi < bj ? bi : bj, hi = bi < bj ? bj : bi;
    if (hi != 2) return 0.0;
    return -sums[(lo == 0 ? 5 : 11) + at];
}

// the rotation that annihilates a_pq, or false where it is skipped
MF_HFIT_HD bool rotation(double app, double aqq, double apq, double& t, double& c, double& s)
{
    if (dabs(apq) <= EPS * root(dabs(app * aqq))) return false;
    const double theta = (aqq - app) / (2.0 * apq);
    t = (theta >= 0.0 ? 1.0 : -1.0) / (dabs(theta) + root(theta * theta + 1.0));
    c = 1.0 / root(t * t + 1.0);
    s = t * c;
    return true;
}

// What the lane of column k (0 .. 8) does for the rotation (p, q) on the row-major 9 x 9 A and V: rows k of both, the mirror entries of A in
// rows p and q, and -- lanes p and q -- the three entries of the 2 x 2 block.  No two lanes touch the same entry, and no lane reads what
// another writes, so the nine may run side by side or one after the other.
MF_HFIT_HD void rotate_column(double* A, double* V, int k, int p, int q, double app, double aqq, double apq, double t, double c, double s)
{
    if (k != p && k != q) {
        const double akp = A[k * 9 + p], akq = A[k * 9 + q];
        const double np_ = c * akp - s * akq, nq_ = s * akp + c * akq;
        A[k * 9 + p] = np_; A[p * 9 + k] = np_;
        A[k * 9 + q] = nq_; A[q * 9 + k] = nq_;
    } else if (k == p) {
        A[p * 9 + p] = app - t * apq;
        A[p * 9 + q] = 0.0; A[q * 9 + p] = 0.0;
    } else {
        A[q * 9 + q] = aqq + t * apq;
    }
    const double vkp = V[k * 9 + p], vkq = V[k * 9 + q];
    V[k * 9 + p] = c * vkp - s * vkq;
    V[k * 9 + q] = s * vkp + c * vkq;
}

// the first index of the smallest diagonal entry, that entry and the smallest of the others
MF_HFIT_HD int smallest(const double* A, double& least, double& second)
{
    int index = 0;
    for (int i = 1; i < 9; ++i)
        if (A[i * 9 + i] < A[index * 9 + index]) index = i;
    least = A[index * 9 + index];
    bool any = false;
    second = 0.0;
    for (int i = 0; i < 9; ++i)
        if (i != index && (!any || A[i * 9 + i] < second)) { second = A[i * 9 + i]; any = true; }
    return index;
}

// H = inv(T_late) h T_early with h = column `index` of V, then the division by h22; false (H untouched) where |h22| <= 1e-12 max |H|
MF_HFIT_HD bool denormalise(const double* V, int index, const double (&sim)[6], const double (&c)[4], double (&H)[9])
{
    double g[9], out[9];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const double h0 = V[(3 * i) * 9 + index], h1 = V[(3 * i + 1) * 9 + index], h2 = V[(3 * i + 2) * 9 + index];
        g[3 * i] = h0 * sim[0]; g[3 * i + 1] = h1 * sim[0]; g[3 * i + 2] = (h0 * sim[2] + h1 * sim[3]) + h2;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        out[j] = g[j] / sim[1] + c[2] * g[6 + j];
        out[3 + j] = g[3 + j] / sim[1] + c[3] * g[6 + j];
        out[6 + j] = g[6 + j];
    }
    double m = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i)
        if (dabs(out[i]) > m) m = dabs(out[i]);
    if (!(dabs(out[8]) > 1e-12 * m)) return false;
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = out[i] / out[8];
    return true;
}

}  // namespace hfit
}  // namespace mf
