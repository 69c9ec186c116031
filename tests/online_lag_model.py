"""NumPy model of the online smoother with a fixed lag (include/meshflow_hip.h, mf_online_smooth_lag_f64), written on top of
tests/online_model.py: the solve and the state are that model's, bit for bit, whatever `lag` is -- the lag selects what is handed out and
never enters the solve.

  P^lag_t = x_t in window t + lag's solution after its last sweep;  C^lag_t = C_t

Window xi's solution is what `online_model.online_smooth` leaves in the state after a push of frame xi alone: state row j holds frame
seen - (L - 1) + j, so frame xi - lag sits in row L - 2 - lag of `c` and `q`.  The state keeps the newest L - 1 frames of a window of L; the
one lag that reaches the frame it has just let go, lag = L - 1, takes that frame from the same window solved again from the state before
the push (`_oldest_of_window`).  0 <= lag <= L - 1: the lagged frame must be in the window, and the state must still hold every frame that
has not been handed out (`pending`)."""
import numpy as np

import online_model as om


def check_lag(lag, L):
    assert isinstance(lag, int) and not isinstance(lag, bool) and 0 <= lag <= L - 1, (lag, L)


def _oldest_of_window(before, vel_row, lam_known_i, taps, omega, iters, beta, lam_newest):
    """(C, x) of the oldest frame of the FULL window that ends at the frame pushed onto `before` (a State with seen >= L - 1): the window
    `online_model.online_smooth` solves for it, built from the same values in the same order."""
    C = list(before.c) + [before.c[-1] + vel_row.astype(np.float64)]
    lam = list(before.lam[:-1]) + [lam_known_i, lam_newest]
    with np.errstate(all='ignore'):
        x = om.solve_window(np.array(C), before.q.copy(), np.array(lam, dtype=np.float64), taps, omega, iters, beta)
    return C[0], x[0], x[1:]


def online_smooth_lag(vel, lam_known, state, taps, omega, iters, beta, lam_newest, lag):
    """One block of n new frames, as `online_model.online_smooth` takes it; updates `state` in place exactly as that does.  Returns (c, p),
    both (m, S) float64 with m = max(0, seen + n - lag) - max(0, seen - lag): the frames seen + i - lag that exist, i = 0 .. n - 1, each as
    it stands after window seen + i's last sweep."""
    vel, lam_known, taps = np.asarray(vel, dtype=np.float32), np.asarray(lam_known, dtype=np.float64), np.asarray(taps, dtype=np.float64)
    n, S, L = vel.shape[0], state.S, state.L
    check_lag(lag, L)
    c_out, p_out = [], []
    for i in range(n):
        xi = state.seen
        before = state.copy() if lag == L - 1 and xi >= lag else None
        c, p = om.online_smooth(vel[i:i + 1], lam_known[i:i + 1], state, taps, omega, iters, beta, lam_newest)
        if lag == 0:
            c_out.append(c[0])
            p_out.append(p[0])
        elif xi - lag < 0:
            continue
        elif before is not None:
            c_t, x_t, rest = _oldest_of_window(before, vel[i], lam_known[i], taps, omega, iters, beta, lam_newest)
            assert rest.tobytes() == state.q.tobytes()                  # (the same window: its other frames are the state's)
            c_out.append(c_t)
            p_out.append(x_t)
        else:
            c_out.append(state.c[L - 2 - lag].copy())
            p_out.append(state.q[L - 2 - lag].copy())
    m = max(0, state.seen - lag) - max(0, state.seen - n - lag)
    assert len(c_out) == m
    return np.array(c_out).reshape(m, S), np.array(p_out).reshape(m, S)


def pending(state, lag):
    """The frames not yet handed out when the stream ends: (c, p), the last min(lag, seen) rows of `state.c` / `state.q` -- the final
    window's solution for frames seen - min(lag, seen) .. seen - 1, oldest first."""
    check_lag(lag, state.L)
    rows = min(lag, state.seen)
    return state.c[state.L - 1 - rows:].copy(), state.q[state.L - 1 - rows:].copy()
