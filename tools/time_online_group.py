"""What a tick of many live streams costs on the MI355X (profiles/online_group.md): one `OnlineGroup.push` of one new frame of each of
--streams streams against that many `OnlineSession.push` calls of the same frames -- the existing path, one session per stream --, both on
running streams (--warm ticks pushed first), both synchronised, by the host clock, ALTERNATED within the process: repetition i times the
group first when i is even and the sessions first when it is odd.  The sessions' figure is the sum of their pushes with ONE wait at the
end, which favours them.  Beside it `ops.online_smooth_group` at K = --streams against K `ops.online_smooth` calls on a full window, by HIP
events.  The better and the median of --repeats after a warm-up pass each.  One JSON line; run it in a fresh process per sample.
    python tools/time_online_group.py [--streams 16] [--form grey|bgr|nv12] [--mesh 16] [--window 40] [--omega 10] [--iters 10]
                                      [--height 1080] [--width 1920] [--warm 32] [--max-per-subframe 128] [--chunk-pairs 32] [--repeats 5]
--lag k times the tick of an `OnlineLagGroup` instead (`lagged` below; profiles/online_group_lag.md)."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--streams', type=int, default=16)
    ap.add_argument('--form', choices=('grey', 'bgr', 'nv12'), default='grey')
    ap.add_argument('--mesh', type=int, default=16)
    ap.add_argument('--window', type=int, default=40)
    ap.add_argument('--omega', type=int, default=10)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--warm', type=int, default=32)
    ap.add_argument('--max-per-subframe', type=int, default=128)
    ap.add_argument('--chunk-pairs', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--no-sessions', action='store_true', help='time the group alone')
    ap.add_argument('--lag', type=int, default=0, help='k >= 1: time the lagged group tick against lagged sessions and the lag-0 group tick')
    ap.add_argument('--contenders', default='lag_group,group,sessions',
                    help='--lag: which of the three to time (group,sessions is what a build without online_lag_group can run)')
    a = ap.parse_args()
    if a.lag:
        return lagged(a)
    import numpy as np
    import torch
    from meshflow_amd import host, ops, synthetic
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    if not torch.cuda.is_available():
        raise SystemExit('time_online_group.py measures on an MI355X: no GPU visible')
    dev = torch.device('cuda:0')
    B, S = a.streams, (a.mesh + 1) * (a.mesh + 1) * 2
    out = dict(streams=B, form=a.form, S=S, window=a.window, omega=a.omega, iters=a.iters, width=a.width, height=a.height, warm=a.warm,
               max_per_subframe=a.max_per_subframe, chunk_pairs=a.chunk_pairs, repeats=a.repeats)

    def report(key, samples):
        out[key + '_best'], out[key + '_median'] = min(samples), statistics.median(samples)

    # the smoother alone: K rows of one frame on full windows, against K single calls
    rng = np.random.default_rng(1)
    fill = torch.from_numpy((rng.standard_normal((B, a.window, S)) * 2.0).astype(np.float32)).to(dev)
    lam = torch.from_numpy(rng.uniform(0.0, 0.95, (B, a.window))).to(dev)
    taps = torch.from_numpy(host.online_taps(a.omega)).to(dev)
    stacked, singles = ops.OnlineGroupState(B, S, a.window, dev), [ops.OnlineState(S, a.window, dev) for _ in range(B)]
    ops.online_smooth_group(fill, lam, stacked, range(B), taps, a.omega, a.iters, 1.0, 0.95)
    for b in range(B):
        ops.online_smooth(fill[b], lam[b], singles[b], taps, a.omega, a.iters, 1.0, 0.95)
    one_v, one_l = fill[:, :1].contiguous(), lam[:, :1].contiguous()
    together, apart = [], []
    for i in range(a.repeats + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        ops.online_smooth_group(one_v, one_l, stacked, range(B), taps, a.omega, a.iters, 1.0, 0.95)
        ev[1].record()
        ev[2].record()
        for b in range(B):
            ops.online_smooth(one_v[b], one_l[b], singles[b], taps, a.omega, a.iters, 1.0, 0.95)
        ev[3].record()
        torch.cuda.synchronize()
        if i:
            together.append(ev[0].elapsed_time(ev[1]))
            apart.append(ev[2].elapsed_time(ev[3]))
    report('smooth_group_ms', together)
    report('smooth_singles_ms', apart)

    # whole ticks on running streams: stream b's frame t is frame t + b of one pool, so no two streams show the same picture at a tick
    ticks = a.warm + a.repeats + 1
    count = ticks + B
    pool = torch.cat([synthetic.frames_torch(min(50, count - lo), a.height, a.width, dev, seed=1, first_frame=lo) for lo in range(0, count, 50)])
    if a.form != 'bgr':
        pool = pool[..., 1].contiguous()
    uv = torch.randint(0, 256, (count, a.height // 2, a.width // 2, 2), dtype=torch.uint8, device=dev) if a.form == 'nv12' else None
    rows = torch.arange(B, device=dev)

    def tick(t):
        return (pool[rows + t], uv[rows + t]) if uv is not None else pool[rows + t]

    def row(frames, b):
        return tuple(p[b:b + 1] for p in frames) if uv is not None else frames[b:b + 1]

    s = MeshFlowStabilizer(mesh_row_count=a.mesh, mesh_col_count=a.mesh, temporal_smoothing_radius=a.omega, device='cuda:0')
    kw = dict(window=a.window, iters=a.iters, max_per_subframe=a.max_per_subframe, chunk_pairs=a.chunk_pairs)
    group = s.online_group(B, **kw)
    sessions = [] if a.no_sessions else [s.online_session(**kw) for _ in range(B)]
    lost = [0, 0]

    def push_group(frames):
        _, reports = group.push(frames)
        torch.cuda.synchronize()
        lost[0] += sum(len(r.lost) for r in reports)

    def push_sessions(frames):
        for b, session in enumerate(sessions):
            lost[1] += len(session.push(row(frames, b))[1].lost)
        torch.cuda.synchronize()

    def timed(fn, frames):
        w0 = time.perf_counter()
        fn(frames)
        return (time.perf_counter() - w0) * 1e3

    for t in range(a.warm):                                             # (fills the windows and warms every kernel up)
        frames = tick(t)
        push_group(frames)
        push_sessions(frames)
    together, apart = [], []
    for i in range(a.repeats + 1):
        frames = tick(a.warm + i)
        torch.cuda.synchronize()
        order = (push_group, push_sessions) if i % 2 == 0 else (push_sessions, push_group)
        ms = {fn: timed(fn, frames) for fn in order}
        if i:
            together.append(ms[push_group])
            apart.append(ms[push_sessions])
    report('group_push_ms', together)
    out['lost_pairs_group'] = lost[0]
    if sessions:
        report('sessions_push_ms', apart)
        out['lost_pairs_sessions'] = lost[1]
        out['group_over_sessions_median'] = out['group_push_ms_median'] / out['sessions_push_ms_median']
    print(json.dumps(out))


def lagged(a):
    """--lag k (profiles/online_group_lag.md): per tick of --streams running streams, by HIP events around each and one wait behind it, in an
    order that turns with the repetition, (a) one `OnlineLagGroup.push`, (b) that many `online_session(lag=k)` pushes, (c) one lag-0
    `OnlineGroup.push`; and, alone, one `ops.ring_exchange` per plane of a steady tick (about 4 N K bytes) against `Tensor.copy_` of 2 N K
    bytes, which moves as many."""
    import numpy as np
    import torch
    from meshflow_amd import ops, synthetic
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    if not torch.cuda.is_available():
        raise SystemExit('time_online_group.py measures on an MI355X: no GPU visible')
    dev = torch.device('cuda:0')
    B, k = a.streams, a.lag
    out = dict(streams=B, lag=k, form=a.form, mesh=a.mesh, window=a.window, omega=a.omega, iters=a.iters, width=a.width, height=a.height,
               warm=a.warm, max_per_subframe=a.max_per_subframe, chunk_pairs=a.chunk_pairs, repeats=a.repeats)

    def report(key, samples):
        out[key + '_best'], out[key + '_median'] = min(samples), statistics.median(samples)

    ticks = a.warm + a.repeats + 1
    count = ticks + B
    pool = torch.cat([synthetic.frames_torch(min(50, count - lo), a.height, a.width, dev, seed=1, first_frame=lo) for lo in range(0, count, 50)])
    if a.form != 'bgr':
        pool = pool[..., 1].contiguous()
    uv = torch.randint(0, 256, (count, a.height // 2, a.width // 2, 2), dtype=torch.uint8, device=dev) if a.form == 'nv12' else None
    rows = torch.arange(B, device=dev)

    def tick(t):
        return (pool[rows + t], uv[rows + t]) if uv is not None else pool[rows + t]

    def row(frames, b):
        return tuple(p[b:b + 1] for p in frames) if uv is not None else frames[b:b + 1]

    s = MeshFlowStabilizer(mesh_row_count=a.mesh, mesh_col_count=a.mesh, temporal_smoothing_radius=a.omega, device='cuda:0')
    kw = dict(window=a.window, iters=a.iters, max_per_subframe=a.max_per_subframe, chunk_pairs=a.chunk_pairs)
    wanted = [name for name in a.contenders.split(',') if not (name == 'sessions' and a.no_sessions)]
    if not wanted or set(wanted) - {'lag_group', 'group', 'sessions'}:
        raise SystemExit(f'--contenders takes lag_group, group and sessions (got {a.contenders!r})')
    lag_group = s.online_lag_group(B, k, **kw) if 'lag_group' in wanted else None
    plain_group = s.online_group(B, **kw) if 'group' in wanted else None
    sessions = [s.online_session(lag=k, **kw) for _ in range(B)] if 'sessions' in wanted else []

    def push_lag_group(frames):
        lag_group.push(frames)

    def push_sessions(frames):
        for b, session in enumerate(sessions):
            session.push(row(frames, b))

    def push_plain_group(frames):
        plain_group.push(frames)

    contenders = [dict(lag_group=push_lag_group, group=push_plain_group, sessions=push_sessions)[name] for name in wanted]
    out['contenders'] = wanted

    def timed(fn, frames):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        w0 = time.perf_counter()
        ev[0].record()
        fn(frames)
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]), (time.perf_counter() - w0) * 1e3

    for t in range(a.warm):                                             # (fills the windows and the rings, warms every kernel up)
        frames = tick(t)
        for fn in contenders:
            fn(frames)
    torch.cuda.synchronize()
    assert lag_group is None or lag_group.pending == [k] * B
    samples = {fn: [] for fn in contenders}
    for i in range(a.repeats + 1):
        frames = tick(a.warm + i)
        torch.cuda.synchronize()
        turn = i % len(contenders)
        for fn in contenders[turn:] + contenders[:turn]:
            ms = timed(fn, frames)
            if i:
                samples[fn].append(ms)
    for fn, key in ((push_lag_group, 'lag_group_push'), (push_plain_group, 'group_push'), (push_sessions, 'lag_sessions_push')):
        if fn in samples:
            report(key + '_event_ms', [e for e, _ in samples[fn]])
            report(key + '_wall_ms', [w for _, w in samples[fn]])
    if lag_group is not None and plain_group is not None:
        out['lag_group_over_group_median'] = out['lag_group_push_wall_ms_median'] / out['group_push_wall_ms_median']
    if lag_group is not None and sessions:
        out['lag_group_over_lag_sessions_median'] = out['lag_group_push_wall_ms_median'] / out['lag_sessions_push_wall_ms_median']
    if lag_group is None:
        print(json.dumps(out))
        return

    # the exchange of a steady tick alone, per plane, against a device copy that moves as many bytes
    frames = tick(ticks - 1)
    planes = frames if uv is not None else (frames,)
    exchange, copy, runs = [], [], 20                                   # 20 ticks per sample, the slot turning as it does in a group
    rings = [torch.zeros((B, k) + tuple(p.shape[1:]), dtype=p.dtype, device=dev) for p in planes]
    twice = [torch.zeros((2,) + tuple(p.shape), dtype=p.dtype, device=dev) for p in planes]
    landing = [torch.empty_like(t) for t in twice]
    for i in range(a.repeats + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        for j in range(runs):
            table = np.array([(b, j % k, b) for b in range(B)], dtype=np.int32)
            for ring, p in zip(rings, planes):
                ops.ring_exchange(ring, p, table, B)
        ev[1].record()
        ev[2].record()
        for j in range(runs):
            for src, dst in zip(twice, landing):
                dst.copy_(src)
        ev[3].record()
        torch.cuda.synchronize()
        if i:
            exchange.append(ev[0].elapsed_time(ev[1]) / runs)
            copy.append(ev[2].elapsed_time(ev[3]) / runs)
    moved = sum(4 * p.numel() * p.element_size() for p in planes)
    report('exchange_ms', exchange)
    report('copy_ms', copy)
    out['exchange_bytes_moved'] = moved
    out['exchange_tb_per_s_median'] = moved / (out['exchange_ms_median'] * 1e-3) / 1e12
    out['copy_tb_per_s_median'] = moved / (out['copy_ms_median'] * 1e-3) / 1e12
    print(json.dumps(out))


if __name__ == '__main__':
    main()
