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
    __shared__ double xs[2][kOnlineMaxWindow];
    const int s = blockIdx.x, lane = threadIdx.x;
    const bool ring = lane < L;
    const int reach = omega < L - 1 ? omega : L - 1;
    int slot = (int)(seen % L);                              // the lane of frame `seen`

    // the frame this lane holds from the state: frame seen - 1 - k sits in lane (slot - 1 - k) mod L, state row L - 2 - k
    double c = 0.0, lam = 0.0, x = 0.0;
    {
        int k = slot - 1 - lane;
        if (k < 0) k += L;
        if (ring && k <= L - 2 && (long long)k < seen) {
            const int j = L - 2 - k;
            c = c_state[(size_t)j * S + s];
            x = q_state[(size_t)j * S + s];
            lam = lam_state[j];
        }
    }
    double c_run = seen > 0 ? c_state[(size_t)(L - 2) * S + s] : 0.0;        // C of frame seen - 1
    int cur = 0;
    xs[0][lane] = x;
    xs[1][lane] = 0.0;
    __syncthreads();

    for (int i = 0; i < n; ++i) {
        const long long xi = seen + i;
        const int count = xi + 1 < (long long)L ? (int)(xi + 1) : L;         // frames in window xi
        int age = slot - lane;                                               // xi - (the frame this lane holds)
        if (age < 0) age += L;
        const bool in = ring && age < count;
        const bool newest = lane == slot;
        const double c_prev = c_run;
        if (xi > 0) c_run = c_prev + (double)vel[(size_t)i * S + s];         // (row 0 of an empty state is not read)
        if (xi > 0 && ring && age == 1) lam = lam_known[i];                  // the weight of frame xi - 1 has become known
        double rhs, one;
        if (newest) {
            int before = slot - 1;
            if (before < 0) before += L;
            c = c_run;
            lam = lam_newest;
            x = xi > 0 ? c_run + (xs[cur][before] - c_prev) : c_run;
            rhs = c;
            one = 1.0;
        } else {
            rhs = c + beta * x;                                              // x still holds q_t
            one = 1.0 + beta;
        }
        if (newest) xs[cur][lane] = x;                                       // (the slot of frame xi - L, which no window holds any more)
        const double two_lam = 2.0 * lam;
        double sw = 0.0;
        for (int d = -reach; d <= reach; ++d) {
            if (d == 0) continue;
            if (in && (unsigned)(age - d) < (unsigned)count) sw = sw + taps[(d < 0 ? -d : d) - 1];
        }
        const double den = one + two_lam * sw;
        __syncthreads();

        for (int it = 0; it < iters; ++it) {
            const double* __restrict__ from = xs[cur];
            double acc = 0.0;
            // (every slot is read and a select keeps or drops the term: no branch per tap, so the reads of a sweep are in flight together;
            // a dropped term never enters the sum, whatever the slot holds)
#pragma unroll 4
            for (int d = -reach; d < 0; ++d) {                               // the older frames, oldest first
                int at = lane + d;
                if (at < 0) at += L;
                const double sum = acc + taps[-d - 1] * from[at & (kOnlineMaxWindow - 1)];
                acc = in && (unsigned)(age - d) < (unsigned)count ? sum : acc;
            }
#pragma unroll 4
            for (int d = 1; d <= reach; ++d) {                               // the newer ones
                int at = lane + d;
                if (at >= L) at -= L;
                const double sum = acc + taps[d - 1] * from[at & (kOnlineMaxWindow - 1)];
                acc = in && (unsigned)(age - d) < (unsigned)count ? sum : acc;
            }
            x = (rhs + two_lam * acc) / den;
            if (in) xs[cur ^ 1][lane] = x;
            cur ^= 1;
            __syncthreads();
        }
        if (newest) {
            c_out[(size_t)i * S + s] = c;
            p_out[(size_t)i * S + s] = x;
        }
        if (++slot == L) slot = 0;
    }

    // the last L - 1 frames back into the state (slot is now the lane of frame seen + n)
    if (ring) {
        int k = slot - 1 - lane;
        if (k < 0) k += L;
        if (k <= L - 2) {
            const int j = L - 2 - k;
            const bool exists = (long long)k < seen + n;
            c_state[(size_t)j * S + s] = exists ? c : 0.0;
            q_state[(size_t)j * S + s] = exists ? x : 0.0;
        }
    }
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

}  // namespace mf
