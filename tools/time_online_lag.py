"""What `lag` frames of look-ahead cost on the MI355X (profiles/online_lag.md), at tools/time_online.py's mesh and windows (S = 578, window
40, radius 10, 10 sweeps): `ops.online_smooth_lag` against `ops.online_smooth` by HIP events, the two calls alternating in one run, for a
300-frame block from an empty state and for a 1-frame block on a full window; and the whole synchronised `OnlineSession.push` of 32 frames and
of 1 frame of 1080p grey on a running session, lag against lag 0, by the host clock, alternating too -- the difference is what holding and
joining `lag` frames of pixels costs.  The better and the median of --repeats after a warm-up pass each.  One JSON line.
    python tools/time_online_lag.py [--lag 5] [--frames 300] [--window 40] [--omega 10] [--iters 10] [--height 1080] [--width 1920]
                                    [--push 32] [--max-per-subframe 128] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lag', type=int, default=5)
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--mesh', type=int, default=16)
    ap.add_argument('--window', type=int, default=40)
    ap.add_argument('--omega', type=int, default=10)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--push', type=int, default=32)
    ap.add_argument('--max-per-subframe', type=int, default=128)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    from meshflow_amd import host, ops, synthetic
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    if not torch.cuda.is_available():
        raise SystemExit('time_online_lag.py measures on an MI355X: no GPU visible')
    dev = torch.device('cuda:0')
    S = (a.mesh + 1) * (a.mesh + 1) * 2
    out = dict(S=S, lag=a.lag, frames=a.frames, window=a.window, omega=a.omega, iters=a.iters, width=a.width, height=a.height, push=a.push,
               max_per_subframe=a.max_per_subframe, repeats=a.repeats)

    def report(key, samples):
        out[key + '_best'], out[key + '_median'] = min(samples), statistics.median(samples)

    rng = np.random.default_rng(1)
    vel = torch.from_numpy((rng.standard_normal((a.frames, S)) * 2.0).astype(np.float32)).to(dev)
    lam = torch.from_numpy(rng.uniform(0.0, 0.95, a.frames)).to(dev)
    taps = torch.from_numpy(host.online_taps(a.omega)).to(dev)

    def smooth(state, n, lag):
        if lag is None:
            ops.online_smooth(vel[:n], lam[:n], state, taps, a.omega, a.iters, 1.0, 0.95)
        else:
            ops.online_smooth_lag(vel[:n], lam[:n], state, taps, a.omega, a.iters, 1.0, 0.95, lag)

    # the smoother alone: plain, lagged, plain, lagged, ... (the first pass of each warms up and is dropped)
    full = {lag: ops.OnlineState(S, a.window, dev) for lag in (None, a.lag)}
    for lag, state in full.items():
        smooth(state, a.frames, lag)
    for n, fresh, key in ((a.frames, True, 'block'), (1, False, 'one_frame')):
        samples = {None: [], a.lag: []}
        for i in range(a.repeats + 1):
            for lag in (None, a.lag):
                state = ops.OnlineState(S, a.window, dev) if fresh else full[lag]
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                ev[0].record()
                smooth(state, n, lag)
                ev[1].record()
                torch.cuda.synchronize()
                if i:
                    samples[lag].append(ev[0].elapsed_time(ev[1]))
        report(f'smooth_{key}_ms', samples[None])
        report(f'smooth_lag_{key}_ms', samples[a.lag])

    # whole pushes on running sessions, lag 0 and lag alternating
    count = a.push * 2 + 1 + a.repeats
    grey = torch.cat([synthetic.frames_torch(min(50, count - lo), a.height, a.width, dev, seed=1, first_frame=lo)[..., 1].contiguous()
                      for lo in range(0, count, 50)])
    s = MeshFlowStabilizer(mesh_row_count=a.mesh, mesh_col_count=a.mesh, temporal_smoothing_radius=a.omega, device='cuda:0')
    lost = 0
    for n, key in ((a.push, f'{a.push}_frames'), (1, '1_frame')):
        samples, sessions = {0: [], a.lag: []}, {}
        for i in range(a.repeats + 1):
            for lag in (0, a.lag):
                if n > 1 or i == 0:                                     # (the timed frames always follow the ones pushed before them)
                    sessions[lag] = s.online_session(window=a.window, iters=a.iters, max_per_subframe=a.max_per_subframe, lag=lag)
                    sessions[lag].push(grey[:a.push])                   # (fills the window and warms every kernel up)
                session = sessions[lag]
                at = session.seen
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                frames, r = session.push(grey[at:at + n])
                torch.cuda.synchronize()
                w1 = time.perf_counter()
                assert frames.shape[0] == n                             # (a running session hands out as many frames as it takes in)
                lost += len(r.lost)
                if i:
                    samples[lag].append((w1 - w0) * 1e3)
        report(f'push_{key}_ms', samples[0])
        report(f'push_lag_{key}_ms', samples[a.lag])
    out['lost_pairs'] = lost
    out['held_bytes'] = a.lag * a.height * a.width
    print(json.dumps(out))


if __name__ == '__main__':
    main()
