// Online path smoothing: frames pushed in blocks, every frame smoothed over a sliding window that ends at it (zero latency).  The
// arithmetic is a specification of the project's own -- tests/online_model.py, which this file follows operation by operation; the
// reference (meshflowstabilizer.py) has the offline optimisation only.  include/meshflow_hip.h (mf_online_smooth_f64) has the contract.
//
// Per series s of S = V*2, frames numbered from 0 since the session began, `seen` of them before this call:
//   C_t       C_0 = 0, C_t = C_{t-1} + (double)vel_t            the running sum of accumulate_kernel (vertex_motion.hip), carried
//   window xi newest frame xi, frames Phi = [max(0, xi - L + 1), xi]
//   start     x_t = q_t (window xi - 1's solution) for t < xi;  x_xi = C_xi + (q_{xi-1} - C_{xi-1});  x_0 = C_0 in window 0
//   sweep     acc = sum w_|d| x_{t+d}, sw = sum w_|d| over d = -omega .. omega ascending, d != 0, t + d in Phi, from 0.0, one rounded
//             multiply and one rounded add per term (-ffp-contract=off: nothing fuses);
//             x'_t = ((C_t + beta_t q_t) + (2 lam_t) acc) / ((1 + beta_t) + (2 lam_t) sw);  beta_t = beta for t < xi, and for t = xi
//             the q term is left out: x'_xi = (C_xi + (2 lam_xi) acc) / (1.0 + (2 lam_xi) sw)
//   result    P_xi = x_xi after `iters` sweeps; the whole x is window xi + 1's q
//
// Mapping (gfx950): one wavefront per series, one workgroup per wavefront.  The window is a RING: frame t lives in lane t mod L
// (L <= 64) for as long as it is in the window, so C_t, q_t, lam_t stay in that lane's registers from window to window and a new
// frame touches one lane.  x lives in LDS, 2 x 64 doubles per workgroup, double-buffered; a sweep is 2 min(omega, L - 1) ds_read_b64
// per lane (a neighbour further than L - 1 frames away is in no window), predicated on "t + d is in Phi" = "0 <= age - d < frames in
// the window" with age = xi - t.  The taps are wave-uniform (scalar loads).  sw does not depend on x: once per window.  The barrier
// between sweeps is that of a one-wavefront workgroup.  Nothing is shared between workgroups and there are no atomics: a launch on
// the same inputs gives the same bytes, and a non-finite value stays in its series.
// The work is a dependent chain of n x iters short sweeps: latency-bound by nature.
//
// State ([L-1][S] C, [L-1][S] q, [L-1] lam): row j holds frame seen - (L - 1) + j, zero where that frame does not exist yet; the last
// row of lam (the newest frame, whose weight is not known before its successor arrives) holds lam_newest.  The C and q columns are a
// workgroup's own and are updated by it in place; every workgroup READS the L - 1 weights, so they are shifted by a 64-lane launch of
// its own behind the sweep kernel -- two launches per call whatever n is.
//
// Fixed lag (mf_online_smooth_lag_f64; tests/online_lag_model.py): window xi's solution also holds refined values of frames xi - 1,
// xi - 2, ...; the lagged kernel hands out frame xi - lag -- the registers c and x of the lane whose age is `lag`, after the last sweep --
// instead of the newest.  Both kernels are online_smooth_body.h, included with MF_ONLINE_LAG 0 and 1; they differ in that store alone.
//
// Groups (mf_online_smooth_group_f64): K rows of n frames, each row a different stream of B whose states lie stacked.  The grid is (S, K):
// workgroup (s, r) sets up row r's slices -- its velocities, weights and outputs, its stream's three state slices, its stream's `seen` -- under
// the names the body reads and then IS the plain kernel's text, so a row's bytes are those of the single call on those slices.  A row whose
// stream id is outside 0 .. B - 1, or whose `seen` is negative, touches no memory.  The weights launch is one workgroup per row.
// mf_online_smooth_group_lag_f64 is that prologue in front of the lagged text: the two group kernels differ as the two single ones do.
#include "mf_common.h"

namespace mf {

namespace {

constexpr int kOnlineMaxWindow = 64;

__global__ __launch_bounds__(64) void online_smooth_kernel(const float* __restrict__ vel, const double* __restrict__ lam_known,
                                                           const double* __restrict__ taps, int n, int S, int omega, int L, int iters,
                                                           double beta, double lam_newest, long long seen, double* c_state,
                                                           double* q_state, const double* __restrict__ lam_state,
                                                           double* __restrict__ c_out, double* __restrict__ p_out)
{
#define MF_ONLINE_LAG 0
#include "online_smooth_body.h"
#undef MF_ONLINE_LAG
}

__global__ __launch_bounds__(64) void online_smooth_lag_kernel(const float* __restrict__ vel, const double* __restrict__ lam_known,
                                                               const double* __restrict__ taps, int n, int S, int omega, int L, int iters,
                                                               double beta, double lam_newest, long long seen, int lag, double* c_state,
                                                               double* q_state, const double* __restrict__ lam_state,
                                                               double* __restrict__ c_out, double* __restrict__ p_out)
{
#define MF_ONLINE_LAG 1
#include "online_smooth_body.h"
#undef MF_ONLINE_LAG
}

// The plain kernel per row r = blockIdx.y of a group: the body's names are bound to the row's slices in front of it.
__global__ __launch_bounds__(64) void online_smooth_group_kernel(const float* __restrict__ vel_rows, const double* __restrict__ lam_known_rows,
                                                                 const double* __restrict__ taps, const int32_t* __restrict__ ids,
                                                                 const long long* __restrict__ seen_rows, int B, int n, int S, int omega, int L,
                                                                 int iters, double beta, double lam_newest, double* c_stack, double* q_stack,
                                                                 const double* __restrict__ lam_stack, double* __restrict__ c_out_rows,
                                                                 double* __restrict__ p_out_rows)
{
    const size_t r = blockIdx.y, held = (size_t)(L - 1), block = (size_t)n * (size_t)S;
    const int id = ids[r];
    const long long seen = seen_rows[r];
    if ((unsigned)id >= (unsigned)B || seen < 0) return;                     // (workgroup-uniform, before the first barrier)
    const float* __restrict__ vel = vel_rows + r * block;
    const double* __restrict__ lam_known = lam_known_rows + r * (size_t)n;
    double* c_state = c_stack + (size_t)id * held * (size_t)S;
    double* q_state = q_stack + (size_t)id * held * (size_t)S;
    const double* __restrict__ lam_state = lam_stack + (size_t)id * held;
    double* __restrict__ c_out = c_out_rows + r * block;
    double* __restrict__ p_out = p_out_rows + r * block;
#define MF_ONLINE_LAG 0
#include "online_smooth_body.h"
#undef MF_ONLINE_LAG
}

// ... and the lagged kernel per row: the same prologue, the body's fourth inclusion (MF_ONLINE_LAG 1).  Row r hands out frame
// seen_r + i - lag, so rows of one launch may differ in how many of their n outputs are real frames (the others are the body's zeros).
__global__ __launch_bounds__(64) void online_smooth_group_lag_kernel(const float* __restrict__ vel_rows, const double* __restrict__ lam_known_rows,
                                                                     const double* __restrict__ taps, const int32_t* __restrict__ ids,
                                                                     const long long* __restrict__ seen_rows, int B, int n, int S, int omega, int L,
                                                                     int iters, double beta, double lam_newest, int lag, double* c_stack,
                                                                     double* q_stack, const double* __restrict__ lam_stack,
                                                                     double* __restrict__ c_out_rows, double* __restrict__ p_out_rows)
{
    const size_t r = blockIdx.y, held = (size_t)(L - 1), block = (size_t)n * (size_t)S;
    const int id = ids[r];
    const long long seen = seen_rows[r];
    if ((unsigned)id >= (unsigned)B || seen < 0) return;                     // (workgroup-uniform, before the first barrier)
    const float* __restrict__ vel = vel_rows + r * block;
    const double* __restrict__ lam_known = lam_known_rows + r * (size_t)n;
    double* c_state = c_stack + (size_t)id * held * (size_t)S;
    double* q_state = q_stack + (size_t)id * held * (size_t)S;
    const double* __restrict__ lam_state = lam_stack + (size_t)id * held;
    double* __restrict__ c_out = c_out_rows + r * block;
    double* __restrict__ p_out = p_out_rows + r * block;
#define MF_ONLINE_LAG 1
#include "online_smooth_body.h"
#undef MF_ONLINE_LAG
}

// What lane j of a weights launch stores in lam_state row j: frame seen + n - (L - 1) + j.
__device__ __forceinline__ double shifted_lam(const double* __restrict__ lam_known, int n, int L, double lam_newest, long long seen,
                                              const double* lam_state, int j)
{
    double v = 0.0;
    if (j < L - 1) {
        const long long t = seen + n - (L - 1) + j;
        if (t == seen + n - 1) v = lam_newest;
        else if (t >= 0 && t >= seen - 1) v = lam_known[t - seen + 1];      // (t >= 0: entry 0 of an empty state is not read)
        else if (t >= 0) v = lam_state[j + n];                               // frame t was row t - (seen - (L - 1)) = j + n
    }
    return v;
}

// lam_state row j: frame seen + n - (L - 1) + j.  One workgroup, after the sweep kernel on the same stream.
__global__ __launch_bounds__(64) void online_lam_state_kernel(const double* __restrict__ lam_known, int n, int L, double lam_newest,
                                                              long long seen, double* lam_state)
{
    const int j = threadIdx.x;
    const double v = shifted_lam(lam_known, n, L, lam_newest, seen, lam_state, j);
    __syncthreads();
    if (j < L - 1) lam_state[j] = v;
}

// ... and of a group: workgroup r shifts the weights of row r's stream, skipping the rows the sweep kernel skipped.
__global__ __launch_bounds__(64) void online_lam_state_group_kernel(const double* __restrict__ lam_known_rows, const int32_t* __restrict__ ids,
                                                                    const long long* __restrict__ seen_rows, int B, int n, int L,
                                                                    double lam_newest, double* lam_stack)
{
    const size_t r = blockIdx.x;
    const int id = ids[r], j = threadIdx.x;
    const long long seen = seen_rows[r];
    if ((unsigned)id >= (unsigned)B || seen < 0) return;                     // (workgroup-uniform, before the barrier)
    double* lam_state = lam_stack + (size_t)id * (size_t)(L - 1);
    const double v = shifted_lam(lam_known_rows + r * (size_t)n, n, L, lam_newest, seen, lam_state, j);
    __syncthreads();
    if (j < L - 1) lam_state[j] = v;
}

}  // namespace

int launch_online_smooth(const float* vel, const double* lam_known, const double* taps, int n, int S, int omega, int L, int iters,
                         double beta, double lam_newest, long long seen, double* c_state, double* q_state, double* lam_state,
                         double* c_out, double* p_out, hipStream_t st)
{
    static_assert(MF_ONLINE_MAX_WINDOW == kOnlineMaxWindow, "one lane per window slot");
    online_smooth_kernel<<<dim3((unsigned)S), 64, 0, st>>>(vel, lam_known, taps, n, S, omega, L, iters, beta, lam_newest, seen, c_state,
                                                            q_state, lam_state, c_out, p_out);
    MF_HIP_TRY(hipGetLastError());
    online_lam_state_kernel<<<1, 64, 0, st>>>(lam_known, n, L, lam_newest, seen, lam_state);
    MF_HIP_TRY(hipGetLastError());
    return MF_OK;
}

int launch_online_smooth_lag(const float* vel, const double* lam_known, const double* taps, int n, int S, int omega, int L, int lag, int iters,
                             double beta, double lam_newest, long long seen, double* c_state, double* q_state, double* lam_state,
                             double* c_out, double* p_out, hipStream_t st)
{
    online_smooth_lag_kernel<<<dim3((unsigned)S), 64, 0, st>>>(vel, lam_known, taps, n, S, omega, L, iters, beta, lam_newest, seen, lag,
                                                                c_state, q_state, lam_state, c_out, p_out);
    MF_HIP_TRY(hipGetLastError());
    online_lam_state_kernel<<<1, 64, 0, st>>>(lam_known, n, L, lam_newest, seen, lam_state);
    MF_HIP_TRY(hipGetLastError());
    return MF_OK;
}

int launch_online_smooth_group(const float* vel, const double* lam_known, const double* taps, const int32_t* ids, const long long* seen, int K,
                               int B, int n, int S, int omega, int L, int iters, double beta, double lam_newest, double* c_state, double* q_state,
                               double* lam_state, double* c_out, double* p_out, hipStream_t st)
{
    static_assert(MF_ONLINE_GROUP_MAX_ROWS <= 65535, "a row per grid y");
    online_smooth_group_kernel<<<dim3((unsigned)S, (unsigned)K), 64, 0, st>>>(vel, lam_known, taps, ids, seen, B, n, S, omega, L, iters, beta,
                                                                               lam_newest, c_state, q_state, lam_state, c_out, p_out);
    MF_HIP_TRY(hipGetLastError());
    online_lam_state_group_kernel<<<dim3((unsigned)K), 64, 0, st>>>(lam_known, ids, seen, B, n, L, lam_newest, lam_state);
    MF_HIP_TRY(hipGetLastError());
    return MF_OK;
}

int launch_online_smooth_group_lag(const float* vel, const double* lam_known, const double* taps, const int32_t* ids, const long long* seen,
                                   int K, int B, int n, int S, int omega, int L, int lag, int iters, double beta, double lam_newest,
                                   double* c_state, double* q_state, double* lam_state, double* c_out, double* p_out, hipStream_t st)
{
    online_smooth_group_lag_kernel<<<dim3((unsigned)S, (unsigned)K), 64, 0, st>>>(vel, lam_known, taps, ids, seen, B, n, S, omega, L, iters, beta,
                                                                                   lam_newest, lag, c_state, q_state, lam_state, c_out, p_out);
    MF_HIP_TRY(hipGetLastError());
    online_lam_state_group_kernel<<<dim3((unsigned)K), 64, 0, st>>>(lam_known, ids, seen, B, n, L, lam_newest, lam_state);
    MF_HIP_TRY(hipGetLastError());
    return MF_OK;
}

}  // namespace mf
