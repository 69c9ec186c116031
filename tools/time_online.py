"""What online stabilization costs on the MI355X (profiles/online.md): `ops.online_smooth` alone by HIP events at the cfg2 mesh (S = 578,
window 40, radius 10, 10 sweeps) for a 300-frame block from an empty state and for a 1-frame block on a full window; the whole
`OnlineSession.push` -- luma frames in, stabilized and cropped frames out, synchronised -- for 1 and for 32 frames of 1080p grey on a running
session, by the host clock; and, as context only, the offline `ops.jacobi` of a 300-frame clip of the same mesh at the offline default of 100
sweeps and at 10.  The better and the median of --repeats after a warm-up pass each.  One JSON line.
    python tools/time_online.py [--frames 300] [--window 40] [--omega 10] [--iters 10] [--height 1080] [--width 1920] [--push 32]
                                [--max-per-subframe 128] [--repeats 5]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
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
        raise SystemExit('time_online.py measures on an MI355X: no GPU visible')
    dev = torch.device('cuda:0')
    S = (a.mesh + 1) * (a.mesh + 1) * 2
    out = dict(S=S, frames=a.frames, window=a.window, omega=a.omega, iters=a.iters, width=a.width, height=a.height, push=a.push,
               max_per_subframe=a.max_per_subframe, repeats=a.repeats)

    def report(key, samples):
        out[key + '_best'], out[key + '_median'] = min(samples), statistics.median(samples)

    def events(fn):
        samples = []
        for i in range(a.repeats + 1):                                  # (the first pass warms up and is dropped)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            prepared = fn(None)
            ev[0].record()
            fn(prepared)
            ev[1].record()
            torch.cuda.synchronize()
            if i:
                samples.append(ev[0].elapsed_time(ev[1]))
        return samples

    # the smoother alone
    rng = np.random.default_rng(1)
    vel = torch.from_numpy((rng.standard_normal((a.frames, S)) * 2.0).astype(np.float32)).to(dev)
    lam = torch.from_numpy(rng.uniform(0.0, 0.95, a.frames)).to(dev)
    taps = torch.from_numpy(host.online_taps(a.omega)).to(dev)

    def block(prepared):
        if prepared is None:
            return ops.OnlineState(S, a.window, dev)
        ops.online_smooth(vel, lam, prepared, taps, a.omega, a.iters, 1.0, 0.95)

    report('smooth_block_ms', events(block))
    full = ops.OnlineState(S, a.window, dev)
    ops.online_smooth(vel, lam, full, taps, a.omega, a.iters, 1.0, 0.95)

    def one(prepared):
        if prepared is None:
            return full
        ops.online_smooth(vel[:1], lam[:1], prepared, taps, a.omega, a.iters, 1.0, 0.95)

    report('smooth_one_frame_ms', events(one))

    # the offline sweep of the same clip, as context
    disp = torch.cumsum(vel.double(), 0)
    for iters in (100, 10):
        jt, jl, ji = (torch.from_numpy(np.ascontiguousarray(x)).to(dev)
                      for x in host.jacobi_band_coefficients(a.frames, a.width, a.height, 2, None, a.omega))
        report(f'offline_jacobi_{iters}_sweeps_ms', events(lambda prepared: True if prepared is None else ops.jacobi(disp, jt, jl, ji, a.omega, iters)))

    # whole pushes on a running session
    count = a.push * 2 + 1
    grey = torch.cat([synthetic.frames_torch(min(50, count - lo), a.height, a.width, dev, seed=1, first_frame=lo)[..., 1].contiguous()
                      for lo in range(0, count, 50)])
    s = MeshFlowStabilizer(mesh_row_count=a.mesh, mesh_col_count=a.mesh, temporal_smoothing_radius=a.omega, device='cuda:0')
    lost = 0
    for n, key in ((a.push, f'push_{a.push}_frames_ms'), (1, 'push_1_frame_ms')):
        samples = []
        for i in range(a.repeats + 1):
            if n > 1 or i == 0:                                         # (the timed frames always follow the ones pushed before them)
                session = s.online_session(window=a.window, iters=a.iters, max_per_subframe=a.max_per_subframe)
                session.push(grey[:a.push])                             # (fills the window and warms every kernel up)
            at = session.seen
            torch.cuda.synchronize()
            w0 = time.perf_counter()
            frames, r = session.push(grey[at:at + n])
            torch.cuda.synchronize()
            w1 = time.perf_counter()
            lost += len(r.lost)
            if i:
                samples.append((w1 - w0) * 1e3)
        report(key, samples)
    out['lost_pairs'] = lost
    print(json.dumps(out))


if __name__ == '__main__':
    main()
