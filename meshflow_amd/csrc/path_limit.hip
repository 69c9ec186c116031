// The path limiter of an online session: per frame, the largest step k of K at which the mesh placed at g + (k / K) (p - c) still encloses
// the crop rectangle widened by a guard, slew-limited on the way back up, and the path scaled by it (mf_path_limit_f64).  Bit for bit
// tests/path_limit_model.py; the predicates are path_limit_body.h's.  include/meshflow_hip.h has the contract.
//
// path_limit_test_kernel: one workgroup of one wavefront per frame.
//   staging   the B = 2 (R + C) boundary vertices' grid position and d = p - c go to LDS, {gx, gy, dx, dy}: 32 bytes per vertex, B <= 1024,
//             vertex e by lane e mod 64.  Interior vertices are never read.
//   testing   lane j tests candidate j + 1 (f = (j + 1) / K) where j + 1 <= K.  The edge loop runs over the B edges for the whole wavefront
//             at once: every lane reads the SAME vertex from LDS (a broadcast), forms its own position of it, and carries the edge's first
//             vertex over from the iteration before.  Verdicts are combined with selects, no branch per edge: a frame that fails at edge 3
//             costs what a frame that passes costs.
//   verdict   a ballot; the count of its trailing ones is k_raw (a lane past K votes 0).
// Bounds: frame < n; boundary vertex (row <= R, col <= C) of its frame; LDS index e < B <= 1024; d_k_raw[frame].
//
// path_limit_apply_kernel: one workgroup of one wavefront per frame t.  Lane i takes the term k_raw[t - i] + rise i of the closed form for
// i <= t and the lane at i = t + 1 the carry's term k_prev + rise (t + 1); every other lane takes K (a term at i >= 64 is >= rise 64 >= K).
// An integer minimum over the wavefront gives k_t; the 64 lanes then stride over the frame's S series.  k_t == K copies p, k_t == 0 copies c:
// bit for bit, a NaN included.  The carry is read from the device; there is no wait and no atomic anywhere, so the same inputs give the
// same bytes.
//
// path_limit_apply_rows_kernel (mf_path_limit_group_f64): the rows are frames of different streams, each with a carried step of its own; the
// test kernel is per frame already and runs as it is.
#include "mf_common.h"
#include "path_limit_body.h"

namespace mf {

namespace {

struct alignas(16) LimitVertex { double gx, gy, dx, dy; };

__global__ __launch_bounds__(plimit::LANES) void path_limit_test_kernel(const double* __restrict__ unstab, const double* __restrict__ stab,
                                                                        int W, int H, int R, int C, plimit::Rect rect, int steps,
                                                                        int32_t* __restrict__ k_raw)
{
    __shared__ LimitVertex ring[plimit::MAX_BOUNDARY];
    const int lane = threadIdx.x, B = 2 * (R + C);
    const size_t base = (size_t)blockIdx.x * (size_t)(R + 1) * (size_t)(C + 1);
    for (int e = lane; e < B; e += plimit::LANES) {
        int row, col;
        plimit::walk(e, R, C, row, col);
        const size_t v = base + (size_t)row * (size_t)(C + 1) + (size_t)col;
        LimitVertex q;
        q.gx = plimit::grid_at(col, C, W);
        q.gy = plimit::grid_at(row, R, H);
        q.dx = stab[2 * v] - unstab[2 * v];
        q.dy = stab[2 * v + 1] - unstab[2 * v + 1];
        ring[e] = q;
    }
    __syncthreads();

    const bool live = lane < steps;
    const double f = (double)(lane + 1) / (double)steps;
    const LimitVertex first = ring[0];
    const double fx = first.gx + f * first.dx, fy = first.gy + f * first.dy;
    double ax = fx, ay = fy;
    int clear = 1, odd = 0;
    for (int e = 1; e <= B; ++e) {
        double bx = fx, by = fy;
        if (e < B) {                                                     // (wave-uniform)
            const LimitVertex q = ring[e];
            bx = q.gx + f * q.dx;
            by = q.gy + f * q.dy;
        }
        clear &= (int)plimit::edge_clear(ax, ay, bx, by, rect);
        odd ^= (int)plimit::edge_counts(ax, ay, bx, by, rect);
        ax = bx; ay = by;
    }
    const uint64_t verdicts = __ballot(live && (clear & odd));
    if (lane == 0) k_raw[blockIdx.x] = plimit::leading_passes(verdicts);
}

// The scaling statement of both apply kernels: the 64 lanes stride over the S series of the row that starts at `row`.
__device__ __forceinline__ void scale_row(const double* __restrict__ unstab, const double* __restrict__ stab, size_t row, int S, int k, int steps,
                                          int lane, double* __restrict__ out)
{
    const double f = (double)k / (double)steps;
    for (int s = lane; s < S; s += plimit::LANES) {
        const double c = unstab[row + s], p = stab[row + s];
        const double scaled = c + f * (p - c);
        out[row + s] = k == steps ? p : (k == 0 ? c : scaled);
    }
}

__global__ __launch_bounds__(plimit::LANES) void path_limit_apply_kernel(const double* __restrict__ unstab, const double* __restrict__ stab,
                                                                         const int32_t* __restrict__ k_raw, const int32_t* __restrict__ k_prev,
                                                                         int S, int steps, int rise, int32_t* __restrict__ k_out,
                                                                         double* __restrict__ out)
{
    const int lane = threadIdx.x;
    const long long t = blockIdx.x;
    int term = steps;
    if (lane <= t) {
        term = k_raw[t - lane] + rise * lane;                            // <= 64 + 64 * 63
    } else if (lane == t + 1 && k_prev) {
        int carried = *k_prev;
        carried = carried < 0 ? 0 : (carried > steps ? steps : carried);
        term = carried + rise * lane;
    }
#pragma unroll
    for (int step = 32; step >= 1; step >>= 1) {
        const int other = __shfl_xor(term, step, plimit::LANES);
        term = other < term ? other : term;
    }
    const int k = term < steps ? term : steps;
    if (lane == 0) k_out[t] = k;
    scale_row(unstab, stab, (size_t)t * (size_t)S, S, k, steps, lane, out);
}

// The apply step of a group (mf_path_limit_group_f64): row t is a frame of a stream of its own with its own carried step, so nothing is
// chained between rows: k = min(steps, k_raw[t], clamp(k_prev[t], 0, steps) + rise), the rise term left out where k_prev[t] is negative --
// what path_limit_apply_kernel gives a one-frame call with that k_prev, or with none.  Every lane forms the same k (wave-uniform loads).
__global__ __launch_bounds__(plimit::LANES) void path_limit_apply_rows_kernel(const double* __restrict__ unstab, const double* __restrict__ stab,
                                                                              const int32_t* __restrict__ k_raw, const int32_t* __restrict__ k_prev,
                                                                              int S, int steps, int rise, int32_t* __restrict__ k_out,
                                                                              double* __restrict__ out)
{
    const int lane = threadIdx.x;
    const size_t t = blockIdx.x;
    int k = k_raw[t];
    const int carried = k_prev[t];
    if (carried >= 0) {
        const int risen = (carried > steps ? steps : carried) + rise;
        k = risen < k ? risen : k;
    }
    k = k < steps ? k : steps;
    if (lane == 0) k_out[t] = k;
    scale_row(unstab, stab, t * (size_t)S, S, k, steps, lane, out);
}

}  // namespace

int launch_path_limit(const double* unstab, const double* stab, int n, int W, int H, int R, int C, int left, int top, int right, int bottom,
                      double guard, int steps, int rise, const int32_t* k_prev, int32_t* k_raw, int32_t* k, double* out, hipStream_t st)
{
    static_assert(MF_PATH_LIMIT_MAX_STEPS == plimit::MAX_STEPS && MF_PATH_LIMIT_MAX_STEPS == plimit::LANES, "one lane per candidate");
    static_assert(MF_PATH_LIMIT_MAX_BOUNDARY == plimit::MAX_BOUNDARY, "one LDS record per boundary vertex");
    const plimit::Rect rect = plimit::guarded(left, top, right, bottom, guard);
    path_limit_test_kernel<<<dim3((unsigned)n), plimit::LANES, 0, st>>>(unstab, stab, W, H, R, C, rect, steps, k_raw);
    MF_HIP_TRY(hipGetLastError());
    path_limit_apply_kernel<<<dim3((unsigned)n), plimit::LANES, 0, st>>>(unstab, stab, k_raw, k_prev, (R + 1) * (C + 1) * 2, steps, rise, k, out);
    MF_HIP_TRY(hipGetLastError());
    return MF_OK;
}

int launch_path_limit_group(const double* unstab, const double* stab, int K, int W, int H, int R, int C, int left, int top, int right, int bottom,
                            double guard, int steps, int rise, const int32_t* k_prev, int32_t* k_raw, int32_t* k, double* out, hipStream_t st)
{
    const plimit::Rect rect = plimit::guarded(left, top, right, bottom, guard);
    path_limit_test_kernel<<<dim3((unsigned)K), plimit::LANES, 0, st>>>(unstab, stab, W, H, R, C, rect, steps, k_raw);
    MF_HIP_TRY(hipGetLastError());
    path_limit_apply_rows_kernel<<<dim3((unsigned)K), plimit::LANES, 0, st>>>(unstab, stab, k_raw, k_prev, (R + 1) * (C + 1) * 2, steps, rise, k,
                                                                               out);
    MF_HIP_TRY(hipGetLastError());
    return MF_OK;
}

}  // namespace mf
