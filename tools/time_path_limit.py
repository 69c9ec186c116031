"""What the path limiter costs on the MI355X (profiles/path_limit.md): `ops.path_limit` alone by HIP events at the cfg2 mesh (16 x 16, S = 578,
B = 64 boundary vertices, 32 steps) for 1, 32 and --frames frames of a 1080p geometry, on fields that limit about half of the frames; and, by
the host clock around a synchronised `OnlineSession.push` as tools/time_online.py and tools/time_cuts.py do, --push frames and 1 frame of 1080p
grey on a running session with on_uncovered='report' -- the parent commit's push -- and 'limit', alternating.  The better and the median of
--repeats after a warm-up pass each.  One JSON line.
    python tools/time_path_limit.py [--frames 300] [--mesh 16] [--height 1080] [--width 1920] [--push 32] [--window 40] [--omega 10]
                                    [--iters 10] [--max-per-subframe 128] [--repeats 5]"""
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
    from meshflow_amd import online, ops, synthetic
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    if not torch.cuda.is_available():
        raise SystemExit('time_path_limit.py measures on an MI355X: no GPU visible')
    dev = torch.device('cuda:0')
    W, H, M = a.width, a.height, a.mesh
    S = (M + 1) * (M + 1) * 2
    out = dict(S=S, boundary=4 * M, frames=a.frames, width=W, height=H, push=a.push, window=a.window, omega=a.omega, iters=a.iters,
               max_per_subframe=a.max_per_subframe, repeats=a.repeats)

    def report(key, samples):
        out[key + '_best'], out[key + '_median'] = min(samples), statistics.median(samples)

    # the operator alone: a shift of up to twice the margin per frame, 0.3 px of noise per vertex
    rect = online.margin_rectangle(0.08, W, H)
    rng = np.random.default_rng(1)
    c = rng.standard_normal((a.frames, S)) * 5.0
    shift = rng.uniform(-2.0, 2.0, (a.frames, 1, 2)) * np.array([rect[0], rect[1]], np.float64)
    d = np.broadcast_to(shift, (a.frames, S // 2, 2)).reshape(a.frames, S) + rng.uniform(-0.3, 0.3, (a.frames, S))
    d_c, d_p = torch.from_numpy(c).to(dev), torch.from_numpy(c + d).to(dev)
    for n in sorted({1, min(32, a.frames), a.frames}):
        into = torch.empty((n, S), dtype=torch.float64, device=dev)
        samples = []
        for i in range(a.repeats + 1):                                  # (the first pass warms up and is dropped)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            _, k = ops.path_limit(d_c[:n], d_p[:n], W, H, M, M, rect, out=into)
            ev[1].record()
            torch.cuda.synchronize()
            if i:
                samples.append(ev[0].elapsed_time(ev[1]))
        report(f'path_limit_{n}_frames_ms', samples)
        out[f'path_limit_{n}_frames_limited'] = int((k < ops.PATH_LIMIT_STEPS).sum().item())

    # whole pushes on a running session: the parent commit's ('report') and the limited one, alternating
    count = a.push * 2 + 1
    grey = torch.cat([synthetic.frames_torch(min(50, count - lo), H, W, dev, seed=1, first_frame=lo)[..., 1].contiguous()
                      for lo in range(0, count, 50)])
    s = MeshFlowStabilizer(mesh_row_count=M, mesh_col_count=M, temporal_smoothing_radius=a.omega, device='cuda:0')
    lost, limited = 0, 0
    for n in (a.push, 1):
        samples, sessions = {'report': [], 'limit': []}, {}
        for i in range(a.repeats + 1):
            for mode in ('report', 'limit'):
                if n > 1 or i == 0:                                     # (the timed frames always follow the ones pushed before them)
                    sessions[mode] = s.online_session(window=a.window, iters=a.iters, max_per_subframe=a.max_per_subframe, on_uncovered=mode)
                    sessions[mode].push(grey[:a.push])                  # (fills the window and warms every kernel up)
                session = sessions[mode]
                at = session.seen
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                frames, r = session.push(grey[at:at + n])
                torch.cuda.synchronize()
                w1 = time.perf_counter()
                lost += len(r.lost)
                if mode == 'limit':
                    limited += int((session.last_limit < session.limit_steps).sum().item())
                if i:
                    samples[mode].append((w1 - w0) * 1e3)
        for mode, v in samples.items():
            report(f'push_{n}_frames_{mode}_ms', v)
        out[f'push_{n}_frames_overhead_ms'] = out[f'push_{n}_frames_limit_ms_median'] - out[f'push_{n}_frames_report_ms_median']
    out['lost_pairs'], out['frames_limited_in_pushes'] = lost, limited
    print(json.dumps(out))


if __name__ == '__main__':
    main()
