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

// lam_state row j: frame seen + n - (L - 1) + j.  One workgroup, after the sweep kernel on the same stream.
__global__ __launch_bounds__(64) void online_lam_state_kernel(const double* __restrict__ lam_known, int n, int L, double lam_newest,
                                                              long long seen, double* lam_state)
{
    const int j = threadIdx.x;
    double v = 0.0;
    if (j < L - 1) {
        const long long t = seen + n - (L - 1) + j;
        if (t == seen + n - 1) v = lam_newest;
        else if (t >= 0 && t >= seen - 1) v = lam_known[t - seen + 1];      // (t >= 0: entry 0 of an empty state is not read)
        else if (t >= 0) v = lam_state[j + n];                               // frame t was row t - (seen - (L - 1)) = j + n
    }
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

}  // namespace mf
