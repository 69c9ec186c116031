"""What scene-cut detection costs on the MI355X (profiles/cuts.md).  By HIP events, --calls back-to-back calls per sample: `ops.frame_signatures`
(mf_frame_signature_u8) of --push frames and of 1 frame of 1080p, noisy content and constant content, once on ONE stack again and again (66 MB:
it stays in the 256 MiB Infinity Cache) and once ROTATING over --rotate stacks (past the cache: what HBM delivers); beside each `ops.luma` of a
uint16 stack of the same shape, a streaming kernel that reads twice the bytes and writes as many as the signature reads, as the yardstick; and
`ops.cut_distances`; and the --push stacks of the rotation as one call, where the launch path no longer counts.  By the host clock around a synchronised `OnlineSession.push`, as tools/time_online.py does: --push frames and 1 frame of
1080p grey on a running session, with on_cut='ignore' -- the parent commit's push -- and on_cut='reset', alternating, no cut in the frames.
The better and the median of --repeats after a warm-up pass each.  One JSON line.
    python tools/time_cuts.py [--height 1080] [--width 1920] [--push 32] [--rotate 5] [--calls 20] [--repeats 5] [--max-per-subframe 128]"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

HBM_SPEC_TBS = 8.0              # the data sheet's HBM3E rate of the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--push', type=int, default=32)
    ap.add_argument('--rotate', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--mesh', type=int, default=16)
    ap.add_argument('--window', type=int, default=40)
    ap.add_argument('--omega', type=int, default=10)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--max-per-subframe', type=int, default=128)
    ap.add_argument('--repeats', type=int, default=5)
    a = ap.parse_args()
    import torch
    from meshflow_amd import ops, synthetic
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    if not torch.cuda.is_available():
        raise SystemExit('time_cuts.py measures on an MI355X: no GPU visible')
    dev = torch.device('cuda:0')
    H, W = a.height, a.width
    out = dict(width=W, height=H, push=a.push, rotate=a.rotate, calls=a.calls, repeats=a.repeats, max_per_subframe=a.max_per_subframe)

    def report(key, samples):
        out[key + '_best'], out[key + '_median'] = min(samples), statistics.median(samples)

    def events(fn):
        """ms per call: a.calls calls between two events; the first pass warms up and is dropped."""
        samples = []
        for i in range(a.repeats + 1):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            for k in range(a.calls):
                fn(k)
            ev[1].record()
            torch.cuda.synchronize()
            if i:
                samples.append(ev[0].elapsed_time(ev[1]) / a.calls)
        return samples

    # the kernels alone
    gen = torch.Generator(device=dev).manual_seed(1)
    for n in (a.push, 1):
        stacks = {'noisy': torch.randint(0, 256, (a.rotate * n, H, W), dtype=torch.uint8, device=dev, generator=gen),
                  'constant': torch.full((a.rotate * n, H, W), 16, dtype=torch.uint8, device=dev)}
        deep = torch.randint(0, 256, (a.rotate * n, H, W, 2), dtype=torch.uint8, device=dev, generator=gen).view(torch.uint16).reshape(a.rotate * n, H, W)
        luma_out = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
        read = n * H * W
        for content, stack in stacks.items():
            for how, step in (('same', 0), ('rotating', n)):
                key = f'signature_{n}_{content}_{how}_ms'
                report(key, events(lambda k: ops.frame_signatures(stack[(k % a.rotate) * step:(k % a.rotate) * step + n])))
                out[key.replace('_ms', '_gbs')] = read / out[key + '_best'] / 1e6
                out[key.replace('_ms', '_hbm_spec_fraction')] = read / (out[key + '_best'] * 1e-3) / (HBM_SPEC_TBS * 1e12)
        for how, step in (('same', 0), ('rotating', n)):
            key = f'luma_u16_{n}_{how}_ms'
            report(key, events(lambda k: ops.luma(deep[(k % a.rotate) * step:(k % a.rotate) * step + n], out=luma_out)))
            out[key.replace('_ms', '_gbs')] = 3 * read / out[key + '_best'] / 1e6                   # 2 bytes read and 1 written per pixel
        if n > 1:
            # the whole rotation as ONE stack, past the Infinity Cache in a single call: the launch path no longer counts
            every = a.rotate * n
            for content, stack in stacks.items():
                key = f'signature_{every}_{content}_ms'
                report(key, events(lambda k: ops.frame_signatures(stack)))
                out[key.replace('_ms', '_gbs')] = every * H * W / out[key + '_best'] / 1e6
                out[key.replace('_ms', '_hbm_spec_fraction')] = every * H * W / (out[key + '_best'] * 1e-3) / (HBM_SPEC_TBS * 1e12)
            whole_out = torch.empty((every, H, W), dtype=torch.uint8, device=dev)
            key = f'luma_u16_{every}_ms'
            report(key, events(lambda k: ops.luma(deep, out=whole_out)))
            out[key.replace('_ms', '_gbs')] = 3 * every * H * W / out[key + '_best'] / 1e6
            del whole_out
        sig = ops.frame_signatures(stacks['noisy'][:n])
        report(f'distance_{n}_ms', events(lambda k: ops.cut_distances(sig, sig[0])))
        want = ops.frame_signatures(stacks['constant'][:n]).cpu()
        assert int(want.sum()) == read and int(want[:, 1::16].sum()) == read                     # (every pixel of the constant frames in bin 1)
        del stacks, deep

    # whole pushes on a running session: the parent commit's ('ignore') and the scored one ('reset'), alternating
    count = a.push * 2 + 1
    grey = torch.cat([synthetic.frames_torch(min(50, count - lo), H, W, dev, seed=1, first_frame=lo)[..., 1].contiguous()
                      for lo in range(0, count, 50)])
    s = MeshFlowStabilizer(mesh_row_count=a.mesh, mesh_col_count=a.mesh, temporal_smoothing_radius=a.omega, device='cuda:0')
    lost = cuts = 0
    for n in (a.push, 1):
        samples = {'ignore': [], 'reset': []}
        sessions = {}
        for i in range(a.repeats + 1):
            for on_cut in ('ignore', 'reset'):
                if n > 1 or i == 0:                                     # (the timed frames always follow the ones pushed before them)
                    sessions[on_cut] = s.online_session(window=a.window, iters=a.iters, max_per_subframe=a.max_per_subframe, on_cut=on_cut)
                    sessions[on_cut].push(grey[:a.push])                # (fills the window and warms every kernel up)
                session = sessions[on_cut]
                at = session.seen
                torch.cuda.synchronize()
                w0 = time.perf_counter()
                frames, r = session.push(grey[at:at + n])
                torch.cuda.synchronize()
                w1 = time.perf_counter()
                lost += len(r.lost)
                cuts += len(session.last_cuts)
                if i:
                    samples[on_cut].append((w1 - w0) * 1e3)
        for on_cut, v in samples.items():
            report(f'push_{n}_frames_{on_cut}_ms', v)
        out[f'push_{n}_frames_overhead_ms'] = out[f'push_{n}_frames_reset_ms_median'] - out[f'push_{n}_frames_ignore_ms_median']
    out['lost_pairs'], out['cuts_found'] = lost, cuts
    print(json.dumps(out))


if __name__ == '__main__':
    main()
