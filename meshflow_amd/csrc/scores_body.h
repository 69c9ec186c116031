// The device feature scores' arithmetic (scores.hip): the cropping ratio and the distortion of ONE (unstabilized -> cropped) homography,
// mfs.py:1203-1209 after the tracker, and the steps of the clip-level fold -- every step as tests/scores_model.py writes it, which is the
// specification.  The two eigenvalues of the affine part's 2 x 2 block come in closed form (no np.linalg.eigvals: a kernel cannot equal
// LAPACK bit for bit).  Only float64 + - * /, sqrt, comparisons, the conversion to float32 and integers, in the order written here, and (the
// library is built with -ffp-contract=off) no fused multiply-add.  The ORDER OF THE FOLD over a clip's pairs is the caller's: 256 strided
// partials, a halving tree per 64, (w0 + w1) + (w2 + w3).  Plain C++ behind MF_SCORES_HD, so the same functions compile for the host
// (tools/scores_body_check.cpp runs them under the address and undefined-behaviour sanitizers against cases dumped from the model).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MF_SCORES_HD __host__ __device__ __forceinline__
#else
#define MF_SCORES_HD inline
#endif

namespace mf {
namespace scores {

constexpr int OK = 0;                                      // the status of a fitted pair in ops.fit_homographies' record (MF_HFIT_OK)
constexpr int LANES = 256, WAVE = 64;                      // partials per clip; partials per halving tree
constexpr int MAX_PAIRS = 1 << 20;                         // one workgroup walks them all: 4,096 pairs per lane at the most

MF_SCORES_HD double dabs(double v) { return __builtin_fabs(v); }
// correctly rounded on both sides: the device's sqrt() as track_fit.hip uses it (no fast math), the host's IEEE instruction
MF_SCORES_HD double root(double v)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return ::sqrt(v);
#else
    return __builtin_sqrt(v);
#endif
}

// THE float32 NaN of the specification (0x7FC00000): a NaN's sign and payload differ between processors
MF_SCORES_HD float quiet_nan() { return __builtin_nanf(""); }
// the correctly rounded float32 of v; every NaN becomes quiet_nan()
MF_SCORES_HD float to_f32(double v)
{
    const float f = (float)v;
    return f != f ? quiet_nan() : f;
}

// one pair: h = the 9 doubles of its row-major homography
MF_SCORES_HD void pair_scores(const double* h, float& ratio32, float& distortion32)
{
    const double a = h[0], b = h[1], c = h[3], d = h[4];
    ratio32 = to_f32(1.0 / (a * d));
    const double m = (a + d) * 0.5, q = (a - d) * 0.5;
    const double disc = q * q + b * c;
    const double det = a * d - b * c;
    double u, v;
    if (disc >= 0.0) {
        const double r = root(disc);
        const double big = m >= 0.0 ? m + r : m - r;
        const double small = big != 0.0 ? det / big : 0.0;
        u = dabs(big); v = dabs(small);
    } else {                                               // a complex pair (or a NaN): both moduli
        u = v = root(det);
    }
    double x = u, y = v, z = 1.0, t;
    if (x > y) { t = x; x = y; y = t; }
    if (y > z) { t = y; y = z; z = t; }
    if (x > y) { t = x; x = y; y = t; }
    (void)x;
    distortion32 = to_f32(y / z);
}

// a step of the fold of the smallest distortion: `other` where it is smaller (a NaN never is)
MF_SCORES_HD float smaller(float mine, float other) { return other < mine ? other : mine; }

// the clip's two scores from the folded sum, count, smallest distortion and whether a scored distortion was a NaN
MF_SCORES_HD void clip_scores(double sum, int count, float least, bool any_nan, float& cropping, float& distortion)
{
    cropping = to_f32(sum / (double)count);                // (count == 0: 0 / 0, a NaN)
    distortion = (count == 0 || any_nan) ? quiet_nan() : least;
}

}  // namespace scores
}  // namespace mf
