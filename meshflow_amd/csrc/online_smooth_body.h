// The statements of online_smooth.hip's two kernels, included into each between its braces with MF_ONLINE_LAG defined as 0 or 1 -- text, not
// a function, so that the plain kernel compiles to the instructions it had before the lagged one existed (an inlined template body did not:
// tools/isa_compare.py, profiles/online_lag.md).  It reads the kernel's parameters by name: vel, lam_known, taps, n, S, omega, L, iters, beta,
// lam_newest, seen, c_state, q_state, lam_state, c_out, p_out, and with MF_ONLINE_LAG also lag.  The group kernel includes it a third time
// (MF_ONLINE_LAG 0) behind locals of those names bound to one row's slices; s is blockIdx.x there too, the row is blockIdx.y.  The lagged group
// kernel is the fourth inclusion (MF_ONLINE_LAG 1) behind the same locals.
// MF_ONLINE_LAG 0: row i of the outputs is the newest frame of window seen + i, written by its lane.  MF_ONLINE_LAG 1: row i is frame
// seen + i - lag -- the lane whose age in window seen + i is `lag` writes its own C and x after the last sweep --, or 0.0 from the newest lane
// while the session has fewer than lag + 1 frames.  Nothing else differs: the lag selects what is handed out and never enters the solve or
// the state.
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
#if MF_ONLINE_LAG
        {
            // frame xi - lag exists iff the window holds more than `lag` frames (lag <= L - 1); the ring wrap is in `age` already
            const bool exists = count > lag;
            if (exists ? in && age == lag : newest) {
                c_out[(size_t)i * S + s] = exists ? c : 0.0;
                p_out[(size_t)i * S + s] = exists ? x : 0.0;
            }
        }
#else
        if (newest) {
            c_out[(size_t)i * S + s] = c;
            p_out[(size_t)i * S + s] = x;
        }
#endif
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
