"""The device-rectangle crop-resize (mf_crop_resize_dev_*, ops.crop_resize_resident) and `stabilize_resident(crop=True)` on one MI355X,
in one process, the calls of a comparison alternating, HIP events around each launch:

  parity   device-rectangle call against the host-rectangle call (ops.crop_resize), the same frames, rectangle and size, per format:
           the same-size call and a sure upscale (larger than the frame) -- the same instantiation behind one scalar load
  policy   sizes where the host, knowing the rectangle, picks another instantiation: an upscale of the crop that stays below the frame
           (host: up, device rectangle: down) and a reduction beyond the staged span (host: direct, device rectangle: down, LDS reserved)
  pipeline K clips back to back at cfg2 with check='deferred': stabilize_resident then ops.crop_resize(frames, bounds) per clip (the
           host reads the rectangle) against stabilize_resident(crop=True); wall time per clip between two synchronisations

at cfg2 geometry (1920x1080, 300 frames), cfg3 (600 frames) and a 150-frame 4K shard.  One JSON line per measurement.

    python tools/time_resident_crop.py [--reps 15] [--clips 20] [--json profiles/resident_crop_time.jsonl]
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from meshflow_amd import ops, synthetic  # noqa: E402
from meshflow_amd.stabilizer import MeshFlowStabilizer  # noqa: E402

SHAPES = {'cfg2': (300, 1080, 1920), 'cfg3': (600, 1080, 1920), '4k-shard': (150, 2160, 3840)}
FORMATS = ('u8c3', 'u8c1', 'u16c3', 'u8c4')


def frames_of(fmt, n, H, W, dev):
    base = synthetic.frames_torch(min(n, 30), H, W, dev, seed=0, kind='pattern')
    base = base.repeat((n + base.shape[0] - 1) // base.shape[0], 1, 1, 1)[:n].contiguous()
    if fmt == 'u8c1':
        return base[..., 1].contiguous()
    if fmt == 'u8c4':
        return torch.cat([base, base[..., :1]], dim=-1).contiguous()
    if fmt == 'u16c3':
        return (base.to(torch.int32) * 257).to(torch.uint16)
    return base


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def summary(v):
    return {'min_ms': round(min(v), 4), 'median_ms': round(statistics.median(v), 4), 'max_ms': round(max(v), 4)}


def kernels(args, dev, emit):
    for shape, (n, H, W) in SHAPES.items():
        rect = (int(W * 0.075), int(H * 0.075), W - 1 - int(W * 0.075), H - 1 - int(H * 0.075))          # a typical 85 % crop
        cw, ch = rect[2] - rect[0] + 1, rect[3] - rect[1] + 1
        bounds = torch.tensor(rect, dtype=torch.int32, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        # (kind, size): parity = the same instantiation on both sides; policy = the host would pick another one
        sizes = [('parity', None), ('parity', (W + W // 4, H + H // 4)),
                 ('policy up-below-frame', (cw + (W - cw) // 2, ch + (H - ch) // 2)), ('policy down-beyond-span', (cw // 5, ch // 5))]
        for fmt in FORMATS:
            frames = frames_of(fmt, n, H, W, dev)
            for kind, size in sizes:
                ow, oh = size or (W, H)
                out = torch.empty((n, oh, ow) + tuple(frames.shape[3:]), dtype=frames.dtype, device=dev)
                host = lambda: ops.crop_resize(frames, rect, out=out, size=size)                                    # noqa: E731
                devr = lambda: ops.crop_resize_resident(frames, bounds, out=out, size=size, status=status)          # noqa: E731
                for _ in range(3):
                    host(), devr()
                torch.cuda.synchronize()
                ms = {'host_rectangle': [], 'device_rectangle': []}
                for _ in range(args.reps):                                       # alternating
                    ms['host_rectangle'].append(timed(host))
                    ms['device_rectangle'].append(timed(devr))
                h, d = summary(ms['host_rectangle']), summary(ms['device_rectangle'])
                emit({'what': kind, 'shape': shape, 'format': fmt, 'frames': n, 'rect': rect, 'size': [ow, oh], 'reps': args.reps,
                      'host_rectangle': h, 'device_rectangle': d, 'ratio_of_medians': round(d['median_ms'] / h['median_ms'], 4),
                      'inside_host_band': h['min_ms'] <= d['median_ms'] <= h['max_ms']})
            del frames, out
            torch.cuda.empty_cache()
        assert int(status.item()) == 0


def pipeline(args, dev, emit):
    F, H, W, R, C = 300, 1080, 1920, 16, 16
    s = MeshFlowStabilizer(device=str(dev))
    disp, hom = synthetic.motion(F, R, C, seed=0)
    d_disp = torch.from_numpy(disp).to(dev)
    d_frames = synthetic.frames_torch(F, H, W, dev, seed=0, kind='pattern')
    out, cropped = torch.empty_like(d_frames), torch.empty_like(d_frames)
    K = args.clips

    def parent_way():
        for _ in range(K):
            frames, bounds, _ = s.stabilize_resident(d_frames, d_disp, hom, out=out, check='deferred')
            ops.crop_resize(frames, bounds, out=cropped)               # int(v) for v in bounds: four blocking reads per clip
        s.finish()

    def resident():
        for _ in range(K):
            s.stabilize_resident(d_frames, d_disp, hom, out=out, check='deferred', crop=True, cropped_out=cropped)
        s.finish()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / K

    for fn in (parent_way, resident):
        wall(fn)
    ms = {'stabilize_resident + ops.crop_resize': [], 'stabilize_resident(crop=True)': []}
    for _ in range(args.reps):
        ms['stabilize_resident + ops.crop_resize'].append(wall(parent_way))
        ms['stabilize_resident(crop=True)'].append(wall(resident))
    a, b = (summary(v) for v in ms.values())
    emit({'what': 'pipeline', 'shape': 'cfg2', 'clips': K, 'reps': args.reps, 'unit': 'ms per clip, wall, between two synchronisations',
          'stabilize_resident + ops.crop_resize': a, 'stabilize_resident(crop=True)': b,
          'ratio_of_medians': round(b['median_ms'] / a['median_ms'], 4)})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--clips', type=int, default=20)
    ap.add_argument('--json', default=None)
    ap.add_argument('--only', choices=['kernels', 'pipeline'], default=None)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    fh = open(args.json, 'w') if args.json else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if fh:
            fh.write(line + '\n')
            fh.flush()
    if args.only != 'pipeline':
        kernels(args, dev, emit)
    if args.only != 'kernels':
        pipeline(args, dev, emit)


if __name__ == '__main__':
    main()
