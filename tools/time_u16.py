"""uint16 warp and crop-resize against the uint8 ones, in ONE process, alternating, on the same tables (HIP events around the kernel
launch only).  Shapes: cfg2 geometry (300 x 1920x1080, 16x16 mesh), cfg3 (600 frames, 32x32) and a 150-frame 4K shard (16x16).
Frames: full-range uint16 noise generated on the host from a seed (the uint8 frames are its high bytes).  One JSON line per shape:
median and spread of the kernel ms, algorithmic bytes (2 n H W 3 bytes-per-sample) and the fraction of the 8 TB/s peak.

    python tools/time_u16.py [--reps 15] [--shapes cfg2,cfg3,4k]"""
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
    """(uint16 (n, H, W, 3), uint8 high bytes) on the device, generated on the host in slices of 8 frames."""
    f16 = torch.empty((n, H, W, 6), dtype=torch.uint8, device=dev)
    f8 = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(seed)
    for i in range(0, n, 8):
        a = rng.integers(0, 65536, (min(8, n - i), H, W, 3), dtype=np.uint16)
        f16[i:i + len(a)].copy_(torch.from_numpy(a.view(np.uint8)))
        f8[i:i + len(a)].copy_(torch.from_numpy((a >> 8).astype(np.uint8)))
    return f16.view(torch.uint16), f8


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


def run(name, reps, dev):
    H, W, F, R, C = SHAPES[name]
    disp, hom = synthetic.motion(F, R, C, seed=0)
    s = MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, device=str(dev))
    d_disp = torch.from_numpy(disp).to(dev)
    d_stab = s._stabilized_vertex_displacements_device(d_disp, W, H, 0, hom)
    f16, f8 = noise_frames(F, H, W, dev, seed=1)
    o16, o8 = torch.empty_like(f16), torch.empty_like(f8)
    table = ops.cell_table(d_disp, d_stab, W, H, R, C)
    ops.warp(f8, table, out=o8)
    ops.warp(f16, table, out=o16)
    torch.cuda.synchronize()
    table.check()
    rect = tuple(int(v) for v in table.clip_bounds.tolist())
    if rect[2] < rect[0] or rect[3] < rect[1]:
        rect = (W // 50, H // 50, W - 1 - W // 50, H - 1 - H // 50)
    c16, c8 = torch.empty_like(f16), torch.empty_like(f8)
    ms = {'warp_u8': [], 'warp_u16': [], 'crop_resize_u8': [], 'crop_resize_u16': []}
    for i in range(reps + 2):                                 # two warm-up rounds, then alternating
        r = {'warp_u8': timed(lambda: ops.warp(f8, table, out=o8)),
             'warp_u16': timed(lambda: ops.warp(f16, table, out=o16)),
             'crop_resize_u8': timed(lambda: ops.crop_resize(o8, rect, out=c8)),
             'crop_resize_u16': timed(lambda: ops.crop_resize(o16, rect, out=c16))}
        if i >= 2:
            for k, v in r.items():
                ms[k].append(v)
    px = F * H * W * 3
    res = {'shape': name, 'frames': F, 'H': H, 'W': W, 'R': R, 'C': C, 'reps': reps, 'crop_rect': rect}
    for k, v in ms.items():
        res[k] = stats(v, 2 * px * (2 if k.endswith('u16') else 1))
    res['warp_u16_over_u8'] = round(res['warp_u16']['median_ms'] / res['warp_u8']['median_ms'], 3)
    res['crop_resize_u16_over_u8'] = round(res['crop_resize_u16']['median_ms'] / res['crop_resize_u8']['median_ms'], 3)
    print(json.dumps(res), flush=True)
    del f16, f8, o16, o8, c16, c8, table
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--shapes', default='cfg2,cfg3,4k')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    for name in args.shapes.split(','):
        run(name, args.reps, dev)


if __name__ == '__main__':
    main()
