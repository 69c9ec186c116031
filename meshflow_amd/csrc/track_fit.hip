// The homography over a pair's survivors, on the device (mfs.py:524-526): a normalised DLT per pair through the 9 x 9 normal matrix and
// cyclic Jacobi rotations.  Bit for bit tests/homography_model.py; the arithmetic is hfit_body.h's, the ORDER of every sum is this file's.
//
// hfit_sums_kernel: one workgroup of 256 lanes per pair, three passes over the pair's points (32 bytes each, L2-resident): the centroids, the
// distances and second moments about them, the 23 sums of the normal matrix in normalised coordinates.  Lane j adds the terms of points
// j, j + 256, ... in that order from +0.0; each wavefront folds its 64 partials in a halving tree of shuffles (v[j] += v[j + step], step =
// 32 .. 1), lane 0 of each leaves its total in LDS and every lane forms (w0 + w1) + (w2 + w3): no atomics, the same order whatever the
// launch.  The refusals that need no eigenvector (fewer than 4 points, a cloud on one line) end here: identity, status, what the record
// holds by then.  Otherwise the 23 sums go to the workspace (24 doubles per pair) and the similarity into the record.
//
// hfit_solve_kernel: one wavefront per pair.  The normal matrix and the eigenvectors live in LDS (2 x 81 doubles: indexing register arrays
// by a rotation's (p, q) would cost scratch); every lane reads a_pp, a_qq, a_pq and derives the same rotation, lane k < 9 applies it to
// column k (hfit::rotate_column).  A latency chain of a few hundred rotations with one division and two square roots each.  Lane 0 picks the
// eigenvector, goes back to pixel coordinates and writes the result.  Loops are bounded by K, 30 sweeps and 36 rotations; a pair's range
// comes from d_offsets checked against 0 .. K_total, so no load leaves the inputs whatever d_offsets holds.
#include "track.h"

namespace mf {

static_assert(hfit::OK == MF_HFIT_OK && hfit::TOO_FEW == MF_HFIT_TOO_FEW && hfit::COLLINEAR == MF_HFIT_COLLINEAR &&
              hfit::AT_INFINITY == MF_HFIT_AT_INFINITY && hfit::NOT_CONVERGED == MF_HFIT_NOT_CONVERGED && hfit::MAX_PAIRS == MF_HFIT_MAX_PAIRS,
              "hfit_body.h and include/meshflow_hip.h name the same values");

__device__ __forceinline__ double wave_fold(double v)
{
#pragma unroll
    for (int step = hfit::WAVE / 2; step > 0; step >>= 1) v = v + __shfl_down(v, step);
    return v;
}

// the ordered sums of v over the workgroup's 256 lanes, in every lane (parts: 4 x N doubles of LDS)
template <int N> __device__ __forceinline__ void block_sums(double (&v)[N], double* parts, int lane)
{
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = wave_fold(v[i]);
    __syncthreads();                                                          // (the totals of the pass before have been read)
    if ((lane & (hfit::WAVE - 1)) == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) parts[(lane / hfit::WAVE) * N + i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = (parts[i] + parts[N + i]) + (parts[2 * N + i] + parts[3 * N + i]);
}

__device__ __forceinline__ void write_identity(double* h)
{
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = (i % 4 == 0) ? 1.0 : 0.0;
}

__global__ void __launch_bounds__(hfit::LANES) hfit_sums_kernel(const double* __restrict__ early, const double* __restrict__ late,
                                                                const int32_t* __restrict__ offsets, int K_total, double* __restrict__ hom,
                                                                int32_t* __restrict__ info, double* __restrict__ diag, double* __restrict__ work)
{
    __shared__ double parts[4 * hfit::SUMS];
    const int pair = blockIdx.x, lane = threadIdx.x;
    int lo = offsets[pair], hi = offsets[pair + 1];
    if (lo < 0 || hi < lo || hi > K_total) lo = hi = 0;                       // not a range of the inputs: an empty pair
    const int K = hi - lo;
    const double* const e = early + 2 * (size_t)lo;
    const double* const l = late + 2 * (size_t)lo;
    const double kf = (double)K;
    int status = hfit::OK;
    double c[4] = {0.0, 0.0, 0.0, 0.0}, sim[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (K < 4) {
        status = hfit::TOO_FEW;
    } else {
        double first[4] = {0.0, 0.0, 0.0, 0.0};
        for (int i = lane; i < K; i += hfit::LANES) {
            first[0] = first[0] + e[2 * (size_t)i]; first[1] = first[1] + e[2 * (size_t)i + 1];
            first[2] = first[2] + l[2 * (size_t)i]; first[3] = first[3] + l[2 * (size_t)i + 1];
        }
        block_sums(first, parts, lane);
#pragma unroll
        for (int q = 0; q < 4; ++q) c[q] = first[q] / kf;
        double second[hfit::MOMENTS] = {};
        for (int i = lane; i < K; i += hfit::LANES) {
            double t[hfit::MOMENTS];
            hfit::moment_terms(e[2 * (size_t)i], e[2 * (size_t)i + 1], l[2 * (size_t)i], l[2 * (size_t)i + 1], c, t);
#pragma unroll
            for (int q = 0; q < hfit::MOMENTS; ++q) second[q] = second[q] + t[q];
        }
        block_sums(second, parts, lane);
        if (hfit::collinear(second[1], second[2], second[3]) || hfit::collinear(second[5], second[6], second[7])) {
            status = hfit::COLLINEAR;
        } else {
            hfit::similarity(second[0], second[4], kf, c, sim);
            double third[hfit::SUMS] = {};
            for (int i = lane; i < K; i += hfit::LANES) {
                double t[hfit::SUMS];
                hfit::normal_terms(e[2 * (size_t)i], e[2 * (size_t)i + 1], l[2 * (size_t)i], l[2 * (size_t)i + 1], sim, t);
#pragma unroll
                for (int q = 0; q < hfit::SUMS; ++q) third[q] = third[q] + t[q];
            }
            block_sums(third, parts, lane);
            if (lane == 0) {
                double* const out = work + 24 * (size_t)pair;
#pragma unroll
                for (int q = 0; q < hfit::SUMS; ++q) out[q] = third[q];
            }
        }
    }
    if (lane == 0) {
        int32_t* const r = info + 4 * (size_t)pair;
        r[0] = status; r[1] = K; r[2] = 0; r[3] = 0;
        double* const d = diag + 8 * (size_t)pair;
        d[0] = sim[0]; d[1] = sim[1]; d[2] = c[0]; d[3] = c[1]; d[4] = c[2]; d[5] = c[3]; d[6] = 0.0; d[7] = 0.0;
        if (status != hfit::OK) write_identity(hom + 9 * (size_t)pair);
    }
}

__global__ void __launch_bounds__(hfit::WAVE) hfit_solve_kernel(const double* __restrict__ work, double* __restrict__ hom, int32_t* __restrict__ info,
                                                               double* __restrict__ diag)
{
    __shared__ double A[81], V[81];
    const int pair = blockIdx.x, lane = threadIdx.x;
    int32_t* const r = info + 4 * (size_t)pair;
    if (r[0] != hfit::OK) return;                                             // refused by hfit_sums_kernel: its record stands
    const double kf = (double)r[1];
    const double* const sums = work + 24 * (size_t)pair;
    for (int at = lane; at < 81; at += hfit::WAVE) {
        A[at] = hfit::normal_entry(sums, kf, at / 9, at % 9);
        V[at] = at / 9 == at % 9 ? 1.0 : 0.0;
    }
    __syncthreads();
    int sweeps = 0;
    bool converged = false;
#pragma unroll 1
    for (int sweep = 1; sweep <= hfit::MAX_SWEEPS && !converged; ++sweep) {
        bool rotated = false;
#pragma unroll 1
        for (int p = 0; p < 8; ++p) {
#pragma unroll 1
            for (int q = p + 1; q < 9; ++q) {
                const double app = A[p * 9 + p], aqq = A[q * 9 + q], apq = A[p * 9 + q];
                double t, c, s;
                const bool turn = hfit::rotation(app, aqq, apq, t, c, s);
                if (!__builtin_amdgcn_readfirstlane((int)turn)) continue;     // (every lane read the same three entries)
                rotated = true;
                __syncthreads();                                              // one wavefront: orders the reads above before the writes below
                if (lane < 9) hfit::rotate_column(A, V, lane, p, q, app, aqq, apq, t, c, s);
                __syncthreads();
            }
        }
        sweeps = sweep;
        converged = !rotated;
    }
    if (lane != 0) return;
    double least, second;
    const int index = hfit::smallest(A, least, second);
    double* const d = diag + 8 * (size_t)pair;
    r[2] = sweeps; r[3] = index;
    d[6] = least; d[7] = second;
    double* const h = hom + 9 * (size_t)pair;
    if (!converged) {
        r[0] = hfit::NOT_CONVERGED;
        write_identity(h);
        return;
    }
    double sim[6], c[4] = {d[2], d[3], d[4], d[5]}, H[9];
    sim[0] = d[0]; sim[1] = d[1];
    hfit::translations(c, sim);
    if (!hfit::denormalise(V, index, sim, c, H)) {
        r[0] = hfit::AT_INFINITY;
        write_identity(h);
        return;
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = H[i];
}

size_t hfit_workspace_bytes(int n_pairs) { return (size_t)(n_pairs > 0 ? n_pairs : 1) * 24 * sizeof(double); }

int launch_homography_fit(const double* early, const double* late, const int32_t* offsets, int n_pairs, int K_total, double* hom, int32_t* info,
                          double* diag, void* work, hipStream_t st)
{
    hipLaunchKernelGGL(hfit_sums_kernel, dim3(n_pairs), dim3(hfit::LANES), 0, st, early, late, offsets, K_total, hom, info, diag, (double*)work);
    MF_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(hfit_solve_kernel, dim3(n_pairs), dim3(hfit::WAVE), 0, st, (const double*)work, hom, info, diag);
    MF_HIP_TRY(hipGetLastError());
    return MF_OK;
}

}  // namespace mf
