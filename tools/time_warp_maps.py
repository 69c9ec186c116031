"""The coordinate-map kernel (ops.warp_maps) against the uint8 BGR warp (ops.warp), in ONE process, alternating, on the same table (HIP events
around the launches only).  Shapes: cfg2 geometry (300 x 1920x1080, 16x16 mesh), cfg3 (600 frames, 32x32) and a 150-frame 4K shard (16x16).
Frames: uint8 noise generated on the host from a seed (the maps kernel reads none).  Timed per shape:
  warp_maps             float32 [n][H][W][2] out, the table in: 8 H W algorithmic bytes per frame
  warp_u8c3             the yardstick: 6 H W algorithmic bytes per frame (each source byte read once, each output byte written once)
One JSON line per shape: median and spread in ms, algorithmic bytes, the fraction of the 8 TB/s peak, and ratio = warp_maps / warp_u8c3
(medians; the target is <= 1.0).  Before timing, the maps are checked once against the warp: same crop rows and rectangle on fresh tables.

    python tools/time_warp_maps.py [--reps 15] [--shapes cfg2,cfg3,4k]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from meshflow_amd import ops, synthetic  # noqa: E402
from meshflow_amd.stabilizer import MeshFlowStabilizer  # noqa: E402

SHAPES = {'cfg2': (1080, 1920, 300, 16, 16), 'cfg3': (1080, 1920, 600, 32, 32), '4k': (2160, 3840, 150, 16, 16)}
PEAK = 8.0e12


def noise_frames(n, H, W, dev, seed):
    x = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(seed)
    for i in range(0, n, 8):
        a = rng.integers(0, 256, (min(8, n - i), H, W, 3), dtype=np.uint8)
        x[i:i + len(a)].copy_(torch.from_numpy(a))
    return x


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def stats(ms, nbytes):
    med = float(np.median(ms))
    return {'median_ms': round(med, 4), 'min_ms': round(float(np.min(ms)), 4), 'max_ms': round(float(np.max(ms)), 4),
            'algorithmic_bytes': nbytes, 'peak_fraction': round(nbytes / (med * 1e-3) / PEAK, 4)}


def run(name, reps, warmup, dev):
    H, W, F, R, C = SHAPES[name]
    disp, hom = synthetic.motion(F, R, C, seed=0)
    s = MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, device=str(dev))
    d_disp = torch.from_numpy(disp).to(dev)
    d_stab = s._stabilized_vertex_displacements_device(d_disp, W, H, 0, hom)
    c = noise_frames(F, H, W, dev, seed=1)
    oc = torch.empty_like(c)
    maps = torch.empty((F, H, W, 2), dtype=torch.float32, device=dev)
    table = ops.cell_table(d_disp, d_stab, W, H, R, C)
    ops.warp_maps(table, out=maps)
    torch.cuda.synchronize()
    table.check()
    t2 = ops.cell_table(d_disp, d_stab, W, H, R, C)
    ops.warp(c, t2, out=oc)
    torch.cuda.synchronize()
    assert torch.equal(table.crop, t2.crop) and torch.equal(table.clip_bounds, t2.clip_bounds), 'maps and warp disagree on the crop values'
    unowned = int(((maps[..., 0] == W + 1) & (maps[..., 1] == H + 1)).sum())
    cases = {'warp_maps': (lambda: ops.warp_maps(table, out=maps), 8 * F * H * W),
             'warp_u8c3': (lambda: ops.warp(c, table, out=oc), 6 * F * H * W)}
    for _ in range(warmup):
        for fn, _ in cases.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):                      # alternating: both see the same clocks and the same neighbours on the machine
        for k, (fn, _) in cases.items():
            ms[k].append(timed(fn))
    rec = {'shape': name, 'frames': F, 'H': H, 'W': W, 'mesh': [R, C], 'reps': reps, 'warmup': warmup, 'unowned_pixels': unowned}
    for k, (_, nbytes) in cases.items():
        rec[k] = stats(ms[k], nbytes)
    rec['ratio_maps_over_u8c3'] = round(rec['warp_maps']['median_ms'] / rec['warp_u8c3']['median_ms'], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--shapes', default='cfg2,cfg3,4k')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    for name in args.shapes.split(','):
        rec = run(name, max(args.reps, 15), args.warmup, dev)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
