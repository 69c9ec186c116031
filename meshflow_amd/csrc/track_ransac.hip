// The outlier step between LK and the vertex motion, on the device (mfs.py:564-579, 614, 626 and the packing of 521 / 578): RANSAC per
// sub-frame and the gather of the survivors into the layout mf_vertex_motion_f64 takes.  Bit for bit tests/ransac_model.py.
//
// ransac_subframe_kernel: one wavefront per (pair, sub-frame), like lk_level_kernel's one per feature.  The candidates -- points i < min(count,
// max) with found[i] != 0 -- are compacted in index order (ballot + prefix count) into LDS as float32 (ex, ey, lx, ly); a sub-frame with more
// than STAGED of them compacts into its run of the workspace instead and reads them from there (L2-resident: 16 bytes per candidate).  The
// hypothesis loop is wave-uniform: every lane draws the same sample and fits the same H in float64 (ransac_body.h), the lanes stride over the
// candidates, and the consensus count is a ballot popcount summed over the trips -- an integer, so its order does not matter.  No mask is
// kept per hypothesis: the best H is, and its mask is computed once at the end from the inputs themselves (the same arithmetic on the same
// bits).  Every loop is bounded by max_iters, the 16 draws and k.
//
// track_gather_kernel: one wavefront per (pair, sub-frame) again.  Each sums the inlier counts d_info holds -- of the pairs in front of its
// own (pairs below min_features count as empty), of its pair, and of the sub-frames in front of its own -- and so knows where its run starts
// without an atomic: sub-frame order outer, point order inner, which is finish_pair's order.  Counts are clamped to 0 .. max and a wavefront
// writes no more entries than its own count, so no d_info can send a store outside the n * S * max entries of d_early / d_late.
#include "track.h"

namespace mf {
using namespace track;

__device__ __forceinline__ int uniform_int(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int ballot_count(bool v) { return __popcll(__ballot(v)); }
__device__ __forceinline__ int lanes_before(unsigned long long mask, int lane) { return __popcll(mask & ((1ull << lane) - 1ull)); }

__device__ __forceinline__ int wave_sum_int(int v)
{
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) v += __shfl_xor(v, step);
    return v;
}

// the hypothesis loop over k candidates at `cand` (LDS or the workspace: inlined once for each); returns the best count (0 or >= 4)
__device__ __forceinline__ int hypotheses(const float4* cand, int k, int lane, double threshold_sq, double confidence, int max_iters, uint32_t seed,
                                          double (&best_h)[9], int& ran)
{
    int iterations = max_iters, it = 0, best = 0;
    while (it < iterations) {
        int s[4];
        const bool drawn = ransac::draw_sample((uint32_t)it, seed, (uint32_t)k, s);
        ++it;
        if (!uniform_int((int)drawn)) continue;
        double early[4][2], late[4][2];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 c = cand[s[q]];                                    // (0 <= s[q] < k)
            early[q][0] = (double)c.x; early[q][1] = (double)c.y; late[q][0] = (double)c.z; late[q][1] = (double)c.w;
        }
        if (uniform_int((int)(ransac::degenerate4(early) || ransac::degenerate4(late)))) continue;
        double h[9];
        if (!uniform_int((int)ransac::fit4(early, late, h))) continue;
        int count = 0;
        for (int i0 = 0; i0 < k; i0 += 64) {
            const int i = i0 + lane;
            bool in = false;
            if (i < k) {
                const float4 c = cand[i];
                in = ransac::is_inlier(h, (double)c.x, (double)c.y, (double)c.z, (double)c.w, threshold_sq);
            }
            count += ballot_count(in);
        }
        if (count > (best > 3 ? best : 3)) {
            best = count;
#pragma unroll
            for (int q = 0; q < 9; ++q) best_h[q] = h[q];
            const int need = uniform_int(ransac::iterations_needed(count, k, confidence, max_iters));
            iterations = need < iterations ? need : iterations;
        }
    }
    ran = it;
    return best;
}

__global__ void __launch_bounds__(64) ransac_subframe_kernel(const float2* __restrict__ points, const float2* __restrict__ moved,
                                                             const int32_t* __restrict__ counts, const uint8_t* __restrict__ found, int max_per,
                                                             int min_features, double threshold_sq, double confidence, int max_iters, uint32_t seed,
                                                             uint8_t* __restrict__ inlier, int32_t* __restrict__ info, float4* __restrict__ work)
{
    __shared__ float4 staged[ransac::STAGED];
    const int slot = blockIdx.x, lane = threadIdx.x;
    const size_t base = (size_t)slot * max_per;
    const int K = imax(0, imin(counts[slot], max_per));
    int k = 0;
    for (int i0 = 0; i0 < K; i0 += 64) {
        const int i = i0 + lane;
        k += ballot_count(i < K && found[base + i] != 0);
    }
    int status = ransac::OK, best = 0, ran = 0;
    double h[9] = {};
    if (K < min_features || k < min_features || k < 4) {
        status = ransac::TOO_FEW;
    } else {
        const bool in_lds = k <= ransac::STAGED;
        float4* const run = work + base;                                      // (touched only where k > STAGED: the workspace then holds max_per entries per slot)
        int at = 0;
        for (int i0 = 0; i0 < K; i0 += 64) {
            const int i = i0 + lane;
            const bool take = i < K && found[base + i] != 0;
            const unsigned long long mask = __ballot(take);
            const int pos = at + lanes_before(mask, lane);
            if (take && pos < k) {
                const float2 p = points[base + i], m = moved[base + i];
                const float4 c = make_float4(p.x, p.y, m.x, m.y);
                if (in_lds) staged[pos] = c; else run[pos] = c;
            }
            at += __popcll(mask);
        }
        __syncthreads();                                                      // one wavefront: the fence that makes the run visible to its other lanes
        best = in_lds ? hypotheses(staged, k, lane, threshold_sq, confidence, max_iters, seed, h, ran)
                      : hypotheses(run, k, lane, threshold_sq, confidence, max_iters, seed, h, ran);
        if (best < 4) status = ransac::NO_CONSENSUS;
    }
    for (int i0 = 0; i0 < max_per; i0 += 64) {
        const int i = i0 + lane;
        if (i >= max_per) break;
        bool in = false;
        if (status == ransac::OK && i < K && found[base + i] != 0) {
            const float2 p = points[base + i], m = moved[base + i];
            in = ransac::is_inlier(h, (double)p.x, (double)p.y, (double)m.x, (double)m.y, threshold_sq);
        }
        inlier[base + i] = in ? 1 : 0;
    }
    if (lane == 0) {
        int32_t* const out = info + 4 * (size_t)slot;
        out[0] = status; out[1] = k; out[2] = status == ransac::OK ? best : 0; out[3] = ran;
    }
}

__device__ __forceinline__ int kept_count(const int32_t* __restrict__ info, int slot, int max_per)
{
    const int32_t* const r = info + 4 * (size_t)slot;
    return r[0] == ransac::OK ? imax(0, imin(r[2], max_per)) : 0;
}

__global__ void __launch_bounds__(64) track_gather_kernel(const float2* __restrict__ points, const float2* __restrict__ moved,
                                                          const uint8_t* __restrict__ inlier, const int32_t* __restrict__ info, Geom g, int n_pairs,
                                                          int max_per, int min_features, double* __restrict__ early, double* __restrict__ late,
                                                          int32_t* __restrict__ offsets, int32_t* __restrict__ pair_status)
{
    const int S = g.ncols * g.nrows, slot = blockIdx.x, pair = slot / S, s = slot % S, lane = threadIdx.x;
    int before = 0;                                                           // survivors of the pairs in front (n * S * max < 2^31)
    for (int q = lane; q < pair; q += 64) {
        int total = 0;
        for (int j = 0; j < S; ++j) total += kept_count(info, q * S + j, max_per);
        before += total >= min_features ? total : 0;
    }
    before = wave_sum_int(before);
    int mine = 0, ahead = 0;
    for (int j = lane; j < S; j += 64) {
        const int c = kept_count(info, pair * S + j, max_per);
        mine += c;
        ahead += j < s ? c : 0;
    }
    mine = wave_sum_int(mine);
    ahead = wave_sum_int(ahead);
    const bool keep = mine >= min_features;                                   // mfs.py:521
    if (s == 0 && lane == 0) {
        offsets[pair] = before;
        pair_status[pair] = keep ? 0 : MF_TRACK_PAIR_TOO_FEW;
        if (pair == n_pairs - 1) offsets[n_pairs] = before + (keep ? mine : 0);
    }
    if (!keep) return;
    const int want = kept_count(info, slot, max_per);
    const size_t base = (size_t)slot * max_per, at = (size_t)before + ahead;
    const Sub sb = sub_of(g, s);
    int written = 0;
    for (int i0 = 0; i0 < max_per && written < want; i0 += 64) {
        const int i = i0 + lane;
        const bool take = i < max_per && inlier[base + i] != 0;
        const unsigned long long mask = __ballot(take);
        const int pos = written + lanes_before(mask, lane);
        if (take && pos < want) {
            const float2 p = points[base + i], m = moved[base + i];
            // float32 coordinate + the sub-frame's integer offset, in float64 (mfs.py:578): exact
            early[2 * (at + pos)] = (double)p.x + (double)sb.left; early[2 * (at + pos) + 1] = (double)p.y + (double)sb.top;
            late[2 * (at + pos)] = (double)m.x + (double)sb.left; late[2 * (at + pos) + 1] = (double)m.y + (double)sb.top;
        }
        written += __popcll(mask);
    }
}

size_t ransac_workspace_bytes(int n_pairs, int S, int max_per)
{
    return max_per > ransac::STAGED ? (size_t)n_pairs * S * max_per * sizeof(float4) : 16;
}

int launch_ransac(const float* points, const float* moved, const int32_t* counts, const uint8_t* found, int n_pairs, int S, int max_per,
                  int min_features, double threshold, double confidence, int max_iters, uint32_t seed, uint8_t* inlier, int32_t* info, void* work,
                  hipStream_t st)
{
    hipLaunchKernelGGL(ransac_subframe_kernel, dim3(n_pairs * S), dim3(64), 0, st, (const float2*)points, (const float2*)moved, counts, found, max_per,
                       min_features, threshold * threshold, confidence, max_iters, seed, inlier, info, (float4*)work);
    MF_HIP_TRY(hipGetLastError());
    return MF_OK;
}

int launch_track_gather(const float* points, const float* moved, const uint8_t* inlier, const int32_t* info, int n_pairs, const Geom& g, int max_per,
                        int min_features, double* early, double* late, int32_t* offsets, int32_t* pair_status, hipStream_t st)
{
    hipLaunchKernelGGL(track_gather_kernel, dim3(n_pairs * g.ncols * g.nrows), dim3(64), 0, st, (const float2*)points, (const float2*)moved, inlier,
                       info, g, n_pairs, max_per, min_features, early, late, offsets, pair_status);
    MF_HIP_TRY(hipGetLastError());
    return MF_OK;
}

}  // namespace mf
