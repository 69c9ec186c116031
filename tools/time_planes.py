"""The side-plane warps (ops.warp_planes: float32 linear, 1- and 4-byte nearest) against the two things they are measured by, in ONE process,
alternating, on the same table (HIP events around the launches only):
  the recipe they replace   ops.warp_maps followed by torch's grid_sample (float32) or INTEGRATION.md's gather (labels), temporaries included
  warp_u8c1                 the single-channel uint8 warp on the same table
Shapes: cfg2 geometry (300 x 1920x1080, 16x16 mesh), cfg3 (600 frames, 32x32) and a 150-frame 4K shard (16x16).  Planes: noise generated on
the host from a seed.  One JSON line per shape: median and spread in ms per case, algorithmic bytes (2 x element size x H W per frame: each
element read once and written once), the fraction of the 8 TB/s peak, and per plane warp ratio_over_recipe and ratio_over_u8c1 (medians).
Before timing, the nearest warps are checked once against the gather (equal bytes) and the crop rows against the u8c1 warp's.

    python tools/time_planes.py [--reps 15] [--shapes cfg2,cfg3,4k] [--out profiles/planes_time.jsonl]"""
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


def noise(n, H, W, dev, seed, dtype):
    x = torch.empty((n, H, W), dtype=dtype, device=dev)
    rng = np.random.default_rng(seed)
    for i in range(0, n, 8):
        m = min(8, n - i)
        if dtype == torch.float32:
            a = rng.random((m, H, W), dtype=np.float32)
        else:
            a = rng.integers(0, 200, (m, H, W), dtype=np.uint8).astype({torch.uint8: np.uint8, torch.int32: np.int32}[dtype])
        x[i:i + m].copy_(torch.from_numpy(a))
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


def gather_recipe(table, maps, labels, fill):
    """INTEGRATION.md's nearest-neighbour recipe, the maps launch included."""
    F, H, W = labels.shape
    ops.warp_maps(table, out=maps)
    idx = maps.round().long()
    ix, iy = idx[..., 0], idx[..., 1]
    inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
    flat = (iy.clamp(0, H - 1) * W + ix.clamp(0, W - 1)).view(F, -1)
    return torch.where(inside, labels.view(F, -1).gather(1, flat).view(F, H, W), torch.full_like(labels, fill))


def grid_recipe(table, maps, planes):
    """INTEGRATION.md's float32 recipe, the maps launch included (zeros outside: grid_sample has no other constant)."""
    ops.warp_maps(table, out=maps)
    return torch.nn.functional.grid_sample(planes[:, None], ops.maps_to_grid(maps), mode='bilinear', padding_mode='zeros', align_corners=True)


def run(name, reps, warmup, dev):
    H, W, F, R, C = SHAPES[name]
    disp, hom = synthetic.motion(F, R, C, seed=0)
    s = MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, device=str(dev))
    d_disp = torch.from_numpy(disp).to(dev)
    d_stab = s._stabilized_vertex_displacements_device(d_disp, W, H, 0, hom)
    f32, u8, i32 = (noise(F, H, W, dev, seed, dt) for seed, dt in ((1, torch.float32), (2, torch.uint8), (3, torch.int32)))
    o32, o8, oi, og = torch.empty_like(f32), torch.empty_like(u8), torch.empty_like(i32), torch.empty_like(u8)
    maps = torch.empty((F, H, W, 2), dtype=torch.float32, device=dev)
    table = ops.cell_table(d_disp, d_stab, W, H, R, C)
    ops.warp_planes(u8, table, 'nearest', fill=255, out=o8)
    torch.cuda.synchronize()
    table.check()
    t2 = ops.cell_table(d_disp, d_stab, W, H, R, C)
    ops.warp(u8, t2, out=og)
    torch.cuda.synchronize()
    assert torch.equal(table.crop, t2.crop) and torch.equal(table.clip_bounds, t2.clip_bounds), 'planes and warp disagree on the crop values'
    assert torch.equal(o8, gather_recipe(table, maps, u8, 255)), 'the nearest warp and the gather disagree'
    assert torch.equal(ops.warp_planes(i32, table, 'nearest', fill=-1, out=oi), gather_recipe(table, maps, i32, -1))
    cases = {'planes_f32_linear': (lambda: ops.warp_planes(f32, table, 'linear', out=o32), 8 * F * H * W),
             'recipe_f32_grid_sample': (lambda: grid_recipe(table, maps, f32), 8 * F * H * W),
             'planes_u8_nearest': (lambda: ops.warp_planes(u8, table, 'nearest', fill=255, out=o8), 2 * F * H * W),
             'recipe_u8_gather': (lambda: gather_recipe(table, maps, u8, 255), 2 * F * H * W),
             'planes_i32_nearest': (lambda: ops.warp_planes(i32, table, 'nearest', fill=-1, out=oi), 8 * F * H * W),
             'recipe_i32_gather': (lambda: gather_recipe(table, maps, i32, -1), 8 * F * H * W),
             'warp_u8c1': (lambda: ops.warp(u8, table, out=og), 2 * F * H * W)}
    for _ in range(warmup):
        for fn, _ in cases.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):                      # alternating: all see the same clocks and the same neighbours on the machine
        for k, (fn, _) in cases.items():
            ms[k].append(timed(fn))
    rec = {'shape': name, 'frames': F, 'H': H, 'W': W, 'mesh': [R, C], 'reps': reps, 'warmup': warmup}
    for k, (_, nbytes) in cases.items():
        rec[k] = stats(ms[k], nbytes)
    for k, recipe in (('planes_f32_linear', 'recipe_f32_grid_sample'), ('planes_u8_nearest', 'recipe_u8_gather'), ('planes_i32_nearest', 'recipe_i32_gather')):
        rec[k]['ratio_over_recipe'] = round(rec[k]['median_ms'] / rec[recipe]['median_ms'], 4)
        rec[k]['ratio_over_u8c1'] = round(rec[k]['median_ms'] / rec['warp_u8c1']['median_ms'], 4)
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
