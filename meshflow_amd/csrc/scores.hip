// The cropping ratio and the distortion score of a clip from its per-frame (unstabilized -> cropped) homographies, on the device
// (mfs.py:1196-1212 after the tracker).  Bit for bit tests/scores_model.py; the arithmetic is scores_body.h's, the ORDER of the fold is this
// file's -- the homography fit's (track_fit.hip, profiles/homography_fit.md).
//
// feature_scores_kernel: ONE workgroup of 256 lanes for the whole clip.  Lane j scores the pairs j, j + 256, ... in that order -- four
// doubles of a pair's matrix in, its two float32 values out -- and keeps five partials: the float64 sum of the ratios from +0.0, the smallest
// distortion from +inf, whether a distortion was a NaN, the number of scored pairs and the first pair that was not scored.  Each wavefront
// folds its 64 partials in a halving tree of shuffles (step = 32 .. 1), lane 0 of each leaves its totals in LDS and lane 0 of the workgroup
// forms (w0 + w1) + (w2 + w3): no atomics, the same order whatever the launch.  A clip is a few hundred pairs, so the launch is latency:
// one division and one square root chain per lane.  The loop is bounded by P and every index is below 9 P (matrices), 4 P (record of the
// fit) and 2 P (output): no load leaves the inputs whatever they hold.
#include "mf_common.h"
#include "scores_body.h"

namespace mf {

static_assert(scores::OK == MF_HFIT_OK && scores::MAX_PAIRS == MF_SCORES_MAX_PAIRS, "scores_body.h and include/meshflow_hip.h name the same values");
static_assert(scores::LANES == 4 * scores::WAVE, "the total is (w0 + w1) + (w2 + w3)");

struct ScoreParts { double sum; float least; int32_t nan, count, first; };

__device__ __forceinline__ void fold(ScoreParts& v, const ScoreParts& o)
{
    v.sum = v.sum + o.sum;
    v.least = scores::smaller(v.least, o.least);
    v.nan |= o.nan;
    v.count += o.count;
    v.first = o.first < v.first ? o.first : v.first;
}

__global__ void __launch_bounds__(scores::LANES) feature_scores_kernel(const double* __restrict__ hom, const int32_t* __restrict__ info, int P,
                                                                       float* __restrict__ per_pair, float* __restrict__ out,
                                                                       int32_t* __restrict__ record)
{
    __shared__ ScoreParts parts[scores::LANES / scores::WAVE];
    const int lane = threadIdx.x;
    ScoreParts v = {0.0, __builtin_inff(), 0, 0, P};
    for (int p = lane; p < P; p += scores::LANES) {
        float ratio = scores::quiet_nan(), distortion = scores::quiet_nan();
        if (!info || info[4 * (size_t)p] == scores::OK) {
            scores::pair_scores(hom + 9 * (size_t)p, ratio, distortion);
            v.sum = v.sum + (double)ratio;
            v.least = scores::smaller(v.least, distortion);
            v.nan |= distortion != distortion;
            ++v.count;
        } else if (p < v.first) {
            v.first = p;
        }
        per_pair[2 * (size_t)p] = ratio;
        per_pair[2 * (size_t)p + 1] = distortion;
    }
#pragma unroll
    for (int step = scores::WAVE / 2; step > 0; step >>= 1) {
        ScoreParts o;
        o.sum = __shfl_down(v.sum, step); o.least = __shfl_down(v.least, step); o.nan = __shfl_down(v.nan, step);
        o.count = __shfl_down(v.count, step); o.first = __shfl_down(v.first, step);
        fold(v, o);                                                           // (only lanes j < step of the tree hold what the next step reads)
    }
    if ((lane & (scores::WAVE - 1)) == 0) parts[lane / scores::WAVE] = v;
    __syncthreads();
    if (lane != 0) return;
    ScoreParts lo = parts[0], hi = parts[2];
    fold(lo, parts[1]);
    fold(hi, parts[3]);
    fold(lo, hi);
    float cropping, distortion;
    scores::clip_scores(lo.sum, lo.count, lo.least, lo.nan != 0, cropping, distortion);
    out[0] = cropping; out[1] = distortion;
    record[0] = lo.count; record[1] = lo.first < P ? lo.first : -1;
}

static bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes)
{
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return x < y + b_bytes && y < x + a_bytes;
}

}  // namespace mf

using namespace mf;

extern "C" int mf_feature_scores_f64(const double* d_h, const int32_t* d_info, int pairs, float* d_pair_scores, float* d_scores, int32_t* d_record,
                                     void* stream)
{
    const char* name = "mf_feature_scores_f64";
    if (pairs < 1 || pairs > scores::MAX_PAIRS) {
        set_error("%s: pairs must be in 1 .. %d (got %d): %s", name, scores::MAX_PAIRS, pairs, pairs < 1 ? "no pair to score" : "too many for one call");
        return MF_ERR_INVALID_ARG;
    }
    if (!d_h || !d_pair_scores || !d_scores || !d_record) {
        set_error("%s: null pointer (only d_info may be null: every pair is then scored)", name);
        return MF_ERR_INVALID_ARG;
    }
    if (((uintptr_t)d_h & 7) || ((uintptr_t)d_info & 3) || ((uintptr_t)d_pair_scores & 3) || ((uintptr_t)d_scores & 3) || ((uintptr_t)d_record & 3)) {
        set_error("%s: d_h must be 8-byte aligned, d_info, d_pair_scores, d_scores and d_record 4-byte aligned", name);
        return MF_ERR_INVALID_ARG;
    }
    const size_t P = (size_t)pairs;
    const struct { const void* at; size_t bytes; } in[2] = {{d_h, P * 72}, {d_info, d_info ? P * 16 : 0}},
                                                   out[3] = {{d_pair_scores, P * 8}, {d_scores, 8}, {d_record, 8}};
    for (const auto& i : in)
        for (const auto& o : out)
            if (i.bytes && overlap(i.at, i.bytes, o.at, o.bytes)) { set_error("%s: an input aliases an output", name); return MF_ERR_INVALID_ARG; }
    for (int a = 0; a < 3; ++a)
        for (int b = a + 1; b < 3; ++b)
            if (overlap(out[a].at, out[a].bytes, out[b].at, out[b].bytes)) {
                set_error("%s: two of d_pair_scores, d_scores and d_record alias", name);
                return MF_ERR_INVALID_ARG;
            }
    hipLaunchKernelGGL(feature_scores_kernel, dim3(1), dim3(scores::LANES), 0, (hipStream_t)stream, d_h, d_info, pairs, d_pair_scores, d_scores, d_record);
    MF_HIP_TRY(hipGetLastError());
    return MF_OK;
}
