"""Crop-resize to a caller-chosen output size on one MI355X: the device kernels (mf_crop_resize_to_*) at the sizes users ask for, each
beside today's same-size call on the same frames, interleaved in one process and timed with device events; then the host pipeline
(stabilize_clip(crop=True, keep_uncropped=False)) on a 4K clip with output_size=(1920, 1080) against no output_size, interleaved.

    python tools/time_crop_resize_to.py [--reps 5] [--host-frames 48] [--json out.json]
    python tools/time_crop_resize_to.py --cutover meshflow_amd/variants/libmf_direct.so     # staged / direct sweep of the u8c3 down kernel

(--cutover: this build against another one, interleaved, on u8c3 downscales across the staged / direct cut-over; the all-direct build is
`make -C meshflow_amd/csrc variant NAME=direct EXTRA=-DMF_RESIZE_TO_STAGE_BYTES=16`.)

Bytes: what the tables make a kernel touch -- the distinct source rows times the distinct source columns (taps sx and sx + 1) of the
rectangle, per frame -- plus the output, as a share of 8 TB/s."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from meshflow_amd import ops, synthetic  # noqa: E402
from oracle import meshflow_oracle as mo  # noqa: E402

PEAK = 8e12


def touched_bytes(cw, ch, ow, oh, px_bytes):
    sx, _ = mo.resize_linear_tables(cw, ow)
    sx = np.clip(sx, 0, cw - 1)
    cols = np.unique(np.concatenate([sx, np.minimum(sx + 1, cw - 1)]))
    sy, _ = mo.resize_linear_tables(ch, oh)
    rows = np.unique(np.concatenate([np.clip(sy, 0, ch - 1), np.clip(sy + 1, 0, ch - 1)]))
    return len(rows) * len(cols) * px_bytes


def frames_for(fmt, n, H, W, dev):
    base = synthetic.frames_torch(n, H, W, dev, seed=0)                   # (n, H, W, 3) uint8
    if fmt == 'u8c3':
        return base
    if fmt == 'u8c1':
        return base[..., 1].contiguous()
    return torch.stack([base, base], dim=-1).view(torch.uint16).squeeze(-1)      # 257 v (bytes only: no uint16 torch kernels)


def time_calls(calls, reps, inner=5):
    """calls: {name: fn}; interleaved, device events; median ms per call over reps."""
    t = {k: [] for k in calls}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            torch.cuda.synchronize()
            t[k].append(e0.elapsed_time(e1) / inner)
    return {k: (float(np.median(v)), float(np.min(v))) for k, v in t.items()}


def kernels(reps, dev):
    rows = []
    # (label, n, H, W, rect, sizes)
    setups = [('cfg4 shard', 150, 2160, 3840, (96, 54, 3743, 2105), [(1920, 1080)]),
              ('cfg2', 300, 1080, 1920, (13, 11, 1909, 1068), [(1280, 720), (3840, 2160)])]
    for label, n, H, W, rect, sizes in setups:
        l, t, r, b = rect
        cw, ch = r - l + 1, b - t + 1
        for fmt in ('u8c3', 'u8c1', 'u16c3'):
            frames = frames_for(fmt, n, H, W, dev)
            pxb = frames.element_size() * (3 if frames.dim() == 4 else 1)
            outs = {(W, H): torch.empty_like(frames)}
            for s in sizes:
                outs[s] = torch.empty((n, s[1], s[0]) + tuple(frames.shape[3:]), dtype=frames.dtype, device=dev)
            calls = {'same-size (today)': lambda: ops.crop_resize(frames, rect, out=outs[(W, H)])}
            for s in sizes:
                calls[f'to {s[0]}x{s[1]}'] = (lambda s=s: ops.crop_resize(frames, rect, out=outs[s], size=s))
            res = time_calls(calls, reps)
            for k, (med, mn) in res.items():
                ow, oh = (W, H) if k.startswith('same') else tuple(int(v) for v in k[3:].split('x'))
                by = n * (touched_bytes(cw, ch, ow, oh, pxb) + ow * oh * pxb)
                rows.append(dict(setup=label, fmt=fmt, n=n, frame=f'{W}x{H}', rect=rect, call=k, ms=round(med, 4), ms_min=round(mn, 4),
                                 bytes=int(by), share_of_8TBs=round(by / (med * 1e-3) / PEAK, 4)))
                print(f'{label:10s} {fmt:6s} {k:20s} {med:8.4f} ms (min {mn:.4f})  {by / 1e9:7.3f} GB  {by / (med * 1e-3) / PEAK:6.3f} of 8 TB/s',
                      flush=True)
            del frames, outs
            torch.cuda.empty_cache()
    return rows


def host(reps, F):
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    H, W = 2160, 3840
    frames = synthetic.frames_torch(F, H, W, torch.device('cuda:0'), seed=1).cpu().numpy()
    disp, hom = synthetic.motion(F, 16, 16, seed=1, jitter_sigma=0.5)
    s = MeshFlowStabilizer(device='cuda:0')
    frames = list(frames)
    runs = {'no output_size (4K)': None, 'output_size=(1920, 1080)': (1920, 1080)}
    t = {k: [] for k in runs}
    for k, size in runs.items():                       # warm-up: allocations, ring, page faults of fresh outputs
        s.stabilize_clip(frames, disp, hom, crop=True, keep_uncropped=False, output_size=size)
    for _ in range(reps):
        for k, size in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            s.stabilize_clip(frames, disp, hom, crop=True, keep_uncropped=False, output_size=size)
            t[k].append(time.perf_counter() - t0)
    out = []
    for k, v in t.items():
        med = float(np.median(v))
        out.append(dict(call=k, frames=F, s_median=round(med, 4), s_min=round(float(np.min(v)), 4), frames_per_s=round(F / med, 1)))
        print(f'host {k:28s} {F / med:8.1f} frames/s (median {med * 1e3:.1f} ms over {len(v)}, min {np.min(v) * 1e3:.1f})', flush=True)
    return out


def cutover(other, reps, dev):
    """u8c3, 150 frames of 1080p rows cropped to widths that put 256 output pixels across ~1.5 .. 6 x as many source pixels (the staged
    span holds up to 2,033 bytes: ~2.6 x), against a build of the same library with another kDownPitch, interleaved."""
    import ctypes
    lib = ctypes.CDLL(os.path.abspath(other))
    lib.mf_crop_resize_to_u8c3.argtypes = [ctypes.c_void_p, ctypes.c_void_p] + [ctypes.c_int] * 9 + [ctypes.c_void_p, ctypes.c_void_p]
    from meshflow_amd import _lib
    n, H, W = 150, 1080, 3840
    frames = synthetic.frames_torch(n, H, W, dev, seed=0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = []
    for ratio in (1.5, 2.0, 2.4, 2.6, 2.8, 3.2, 4.0, 6.0):
        ow, oh = 640, 360
        cw, ch = min(W, int(round(ow * ratio))), min(H, int(round(oh * ratio)))
        rect = (0, 0, cw - 1, ch - 1)
        out_a = torch.empty((n, oh, ow, 3), dtype=torch.uint8, device=dev)
        out_b = torch.empty_like(out_a)
        work = torch.empty(_lib.lib.mf_crop_resize_workspace_bytes(ow, oh), dtype=torch.uint8, device=dev)
        calls = {'this build': lambda: ops.crop_resize(frames, rect, out=out_a, size=(ow, oh)),
                 os.path.basename(other): lambda: lib.mf_crop_resize_to_u8c3(frames.data_ptr(), out_b.data_ptr(), n, W, H, *rect, ow, oh,
                                                                            work.data_ptr(), st)}
        res = time_calls(calls, reps)
        same = bool(torch.equal(out_a, out_b))
        by = n * (touched_bytes(cw, ch, ow, oh, 3) + ow * oh * 3)
        line = dict(ratio=ratio, crop=f'{cw}x{ch}', out=f'{ow}x{oh}', identical=same,
                    **{k: dict(ms=round(v[0], 4), share_of_8TBs=round(by / (v[0] * 1e-3) / PEAK, 4)) for k, v in res.items()})
        rows.append(line)
        print(json.dumps(line), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--host-frames', type=int, default=48)
    ap.add_argument('--no-host', action='store_true')
    ap.add_argument('--json', default='')
    ap.add_argument('--cutover', default='', metavar='LIB')
    a = ap.parse_args()
    dev = torch.device('cuda:0')
    if a.cutover:
        res = dict(device=torch.cuda.get_device_name(0), cutover=cutover(a.cutover, a.reps, dev))
        if a.json:
            with open(a.json, 'w') as f:
                json.dump(res, f, indent=1)
        return
    res = dict(device=torch.cuda.get_device_name(0), kernels=kernels(a.reps, dev))
    if not a.no_host:
        res['host'] = host(a.reps, a.host_frames)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, 'w') as f:
            json.dump(res, f, indent=1)


if __name__ == '__main__':
    main()
