"""The NV12 warp (ops.warp_nv12: the grey warp of the luma planes, then the chroma launch) against what it is measured by, in ONE process,
alternating, on the same table (HIP events around the launches only):
  nv12          ops.warp_nv12, both launches
  luma          its first launch alone: ops.warp on the luma planes (the same kernel, the same arguments)
  chroma        its second launch: the C ABI has no entry that launches it alone, so this is nv12 - luma of the same repetition -- the two
                launches run back to back on one stream and each fills the device
  warp_u8c3     the BGR warp of a clip of the same size
  recipe        what a resident NV12 clip pays today: NV12 -> BGR with torch ops (BT.601 limited range, chroma repeated 2 x 2), the u8c3 warp,
                BGR -> NV12 (chroma averaged 2 x 2), in chunks of 30 frames so that the float temporaries stay small
Shapes: cfg2 geometry (300 x 1920x1080, 16x16 mesh), cfg3 (600 frames, 32x32) and a 150-frame 4K shard (16x16).  Planes: noise generated on
the host from a seed.  One JSON line per shape: median and spread in ms per case, algorithmic bytes (every sample read once and written once),
the fraction of the 8 TB/s peak, and the ratios chroma / luma, nv12 / warp_u8c3 and nv12 / recipe (medians).  Before timing, the luma output
is checked once against ops.warp (equal bytes) and the crop rows against the grey warp's.

    python tools/time_nv12.py [--reps 15] [--shapes cfg2,cfg3,4k] [--out profiles/nv12_time.jsonl]"""
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
CHUNK = 30


def noise(shape, dev, seed):
    x = torch.empty(shape, dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(seed)
    for i in range(0, shape[0], 8):
        m = min(8, shape[0] - i)
        x[i:i + m].copy_(torch.from_numpy(rng.integers(0, 256, (m,) + tuple(shape[1:]), dtype=np.uint8)))
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


def nv12_to_bgr(y, uv, out):
    """BT.601 limited range, chroma repeated 2 x 2; out: (m, H, W, 3) uint8."""
    yf = (y.float() - 16.0) * 1.164383
    c = (uv.float() - 128.0).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    u, v = c[..., 0], c[..., 1]
    out[..., 0] = (yf + 2.017232 * u).round_().clamp_(0, 255)
    out[..., 1] = (yf - 0.391762 * u - 0.812968 * v).round_().clamp_(0, 255)
    out[..., 2] = (yf + 1.596027 * v).round_().clamp_(0, 255)


def bgr_to_nv12(bgr, y, uv):
    b, g, r = bgr[..., 0].float(), bgr[..., 1].float(), bgr[..., 2].float()
    y.copy_((16.0 + 0.256788 * r + 0.504129 * g + 0.097906 * b).round_().clamp_(0, 255))
    cu = 128.0 - 0.148223 * r - 0.290993 * g + 0.439216 * b
    cv = 128.0 + 0.439216 * r - 0.367788 * g - 0.071427 * b
    c = torch.nn.functional.avg_pool2d(torch.stack([cu, cv], dim=1), 2)
    uv.copy_(c.permute(0, 2, 3, 1).round_().clamp_(0, 255))


def recipe(y, uv, table, bgr, warped, oy, ouv):
    for i in range(0, y.shape[0], CHUNK):
        nv12_to_bgr(y[i:i + CHUNK], uv[i:i + CHUNK], bgr[i:i + CHUNK])
    ops.warp(bgr, table, out=warped)
    for i in range(0, y.shape[0], CHUNK):
        bgr_to_nv12(warped[i:i + CHUNK], oy[i:i + CHUNK], ouv[i:i + CHUNK])


def run(name, reps, warmup, dev):
    H, W, F, R, C = SHAPES[name]
    disp, hom = synthetic.motion(F, R, C, seed=0)
    s = MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, device=str(dev))
    d_disp = torch.from_numpy(disp).to(dev)
    d_stab = s._stabilized_vertex_displacements_device(d_disp, W, H, 0, hom)
    y, uv = noise((F, H, W), dev, 1), noise((F, H // 2, W // 2, 2), dev, 2)
    oy, ouv, og = torch.empty_like(y), torch.empty_like(uv), torch.empty_like(y)
    bgr = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    warped = torch.empty_like(bgr)
    table = ops.cell_table(d_disp, d_stab, W, H, R, C)
    ops.warp_nv12(y, uv, table, out=(oy, ouv))
    torch.cuda.synchronize()
    table.check()
    t2 = ops.cell_table(d_disp, d_stab, W, H, R, C)
    ops.warp(y, t2, (81,), out=og)
    torch.cuda.synchronize()
    assert torch.equal(oy, og), 'the luma planes and the grey warp disagree'
    assert torch.equal(table.crop, t2.crop) and torch.equal(table.clip_bounds, t2.clip_bounds), 'nv12 and warp disagree on the crop values'
    px = F * H * W
    cases = {'nv12': (lambda: ops.warp_nv12(y, uv, table, out=(oy, ouv)), 3 * px),
             'luma': (lambda: ops.warp(y, table, (81,), out=og), 2 * px),
             'warp_u8c3': (lambda: ops.warp(bgr, table, out=warped), 6 * px),
             'recipe': (lambda: recipe(y, uv, table, bgr, warped, oy, ouv), 3 * px)}
    for _ in range(warmup):
        for fn, _ in cases.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):                      # alternating: all see the same clocks and the same neighbours on the machine
        for k, (fn, _) in cases.items():
            ms[k].append(timed(fn))
    rec = {'shape': name, 'frames': F, 'H': H, 'W': W, 'mesh': [R, C], 'reps': reps, 'warmup': warmup, 'lane_mapping': '4 luma pixels per lane'}
    for k, (_, nbytes) in cases.items():
        rec[k] = stats(ms[k], nbytes)
    rec['chroma'] = stats([a - b for a, b in zip(ms['nv12'], ms['luma'])], px)
    rec['chroma']['derived'] = 'nv12 - luma per repetition'
    rec['chroma_over_luma'] = round(rec['chroma']['median_ms'] / rec['luma']['median_ms'], 4)
    rec['nv12_over_warp_u8c3'] = round(rec['nv12']['median_ms'] / rec['warp_u8c3']['median_ms'], 4)
    rec['nv12_over_recipe'] = round(rec['nv12']['median_ms'] / rec['recipe']['median_ms'], 4)
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
