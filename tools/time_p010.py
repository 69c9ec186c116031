"""The P010 warp (ops.warp_p010: the uint16 luma launch, then the chroma launch) against what it is measured by, in ONE process, alternating,
on the same table (HIP events around the launches only):
  p010          ops.warp_p010, both launches
  warp_u16c3    the uint16 BGR warp of a clip of the same size
  nv12          the 8-bit ops.warp_nv12 of a clip of the same size
  recipe        what a resident P010 clip pays without the call: P010 -> uint16 BGR with torch ops (BT.601 limited range, chroma repeated
                2 x 2), the u16c3 warp, BGR -> P010 (chroma averaged 2 x 2), in chunks of 30 frames so that the float temporaries stay small
  luma, chroma  the two launches of p010.  The C ABI has no entry that launches either alone, so HIP events cannot separate them: after the
                timed repetitions the call runs a few more times under torch.profiler and the two kernels' own device durations are read
                from its records (median per call); 'split': 'unavailable: ...' where the profiler gives none
Shapes: cfg2 geometry (300 x 1920x1080, 16x16 mesh), cfg3 (600 frames, 32x32) and a 150-frame 4K shard (16x16).  Planes: noise generated on
the host from a seed, the whole 16-bit range.  One JSON line per shape: median and spread in ms per case, algorithmic bytes (every sample
read once and written once), the fraction of the 8 TB/s peak, and the ratios p010 / warp_u16c3, p010 / nv12 and p010 / recipe (medians).
Before timing, the luma output is checked once against channel 0 of ops.warp on stack(Y, Y, Y) for the first frames, and the crop rows
against the u16c3 warp's.

    python tools/time_p010.py [--reps 15] [--shapes cfg2,cfg3,4k] [--out profiles/p010_time.jsonl]"""
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


def noise(shape, dev, seed, dtype):
    x = torch.empty(shape, dtype=dtype, device=dev)
    rng = np.random.default_rng(seed)
    np_dtype, top = (np.uint16, 65536) if dtype == torch.uint16 else (np.uint8, 256)
    for i in range(0, shape[0], 8):
        m = min(8, shape[0] - i)
        x[i:i + m].copy_(torch.from_numpy(rng.integers(0, top, (m,) + tuple(shape[1:]), dtype=np_dtype)))
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


def p010_to_bgr(y, uv, out):
    """BT.601 limited range on samples / 256, chroma repeated 2 x 2; out: (m, H, W, 3) uint16."""
    yf = (y.float() * (1.0 / 256.0) - 16.0) * 1.164383
    c = (uv.float() * (1.0 / 256.0) - 128.0).repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    u, v = c[..., 0], c[..., 1]
    out[..., 0] = ((yf + 2.017232 * u) * 256.0).round_().clamp_(0, 65535)
    out[..., 1] = ((yf - 0.391762 * u - 0.812968 * v) * 256.0).round_().clamp_(0, 65535)
    out[..., 2] = ((yf + 1.596027 * v) * 256.0).round_().clamp_(0, 65535)


def bgr_to_p010(bgr, y, uv):
    b, g, r = (bgr[..., k].float() * (1.0 / 256.0) for k in range(3))
    y.copy_(((16.0 + 0.256788 * r + 0.504129 * g + 0.097906 * b) * 256.0).round_().clamp_(0, 65535))
    cu = 128.0 - 0.148223 * r - 0.290993 * g + 0.439216 * b
    cv = 128.0 + 0.439216 * r - 0.367788 * g - 0.071427 * b
    c = torch.nn.functional.avg_pool2d(torch.stack([cu, cv], dim=1), 2)
    uv.copy_((c.permute(0, 2, 3, 1) * 256.0).round_().clamp_(0, 65535))


def recipe(y, uv, table, bgr, warped, oy, ouv):
    for i in range(0, y.shape[0], CHUNK):
        p010_to_bgr(y[i:i + CHUNK], uv[i:i + CHUNK], bgr[i:i + CHUNK])
    ops.warp(bgr, table, out=warped)
    for i in range(0, y.shape[0], CHUNK):
        bgr_to_p010(warped[i:i + CHUNK], oy[i:i + CHUNK], ouv[i:i + CHUNK])


def kernel_split(fn, calls=5):
    """Median device duration in ms of the call's two kernels, from torch.profiler's kernel records of `calls` calls."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
    found = {'luma': [], 'chroma': []}
    for e in prof.events():
        for key, frag in (('luma', 'warp16c1_footprint'), ('chroma', 'p010_chroma_footprint')):
            if frag in e.name:
                found[key].append(float(getattr(e, 'device_time', None) or getattr(e, 'cuda_time', 0.0)) * 1e-3)
    if len(found['luma']) < calls or len(found['chroma']) < calls:
        raise RuntimeError(f"the profiler recorded {len(found['luma'])} luma and {len(found['chroma'])} chroma kernels of {calls} calls")
    # (a clip of more than 65,535 frames would be several launches per call; the shapes here are one each)
    return {k: round(float(np.median(v)), 4) for k, v in found.items()}


def run(name, reps, warmup, dev):
    H, W, F, R, C = SHAPES[name]
    disp, hom = synthetic.motion(F, R, C, seed=0)
    s = MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, device=str(dev))
    d_disp = torch.from_numpy(disp).to(dev)
    d_stab = s._stabilized_vertex_displacements_device(d_disp, W, H, 0, hom)
    y, uv = noise((F, H, W), dev, 1, torch.uint16), noise((F, H // 2, W // 2, 2), dev, 2, torch.uint16)
    oy, ouv = torch.empty_like(y), torch.empty_like(uv)
    y8, uv8 = noise((F, H, W), dev, 3, torch.uint8), noise((F, H // 2, W // 2, 2), dev, 4, torch.uint8)
    oy8, ouv8 = torch.empty_like(y8), torch.empty_like(uv8)
    bgr = torch.empty((F, H, W, 3), dtype=torch.uint16, device=dev)
    warped = torch.empty_like(bgr)
    table = ops.cell_table(d_disp, d_stab, W, H, R, C)
    ops.warp_p010(y, uv, table, out=(oy, ouv))
    torch.cuda.synchronize()
    table.check()
    # luma against the u16c3 warp of stack(Y, Y, Y), the first frames; the crop rows of the whole clip
    m = min(F, 4)
    t2 = ops.cell_table(d_disp, d_stab, W, H, R, C)
    for k in range(3):
        bgr[..., k].copy_(y)
    ops.warp(bgr, t2, (20736,) * 3, out=warped)
    torch.cuda.synchronize()
    assert np.array_equal(oy[:m].cpu().numpy(), warped[:m, ..., 0].cpu().numpy()), 'the luma planes and the u16c3 warp disagree'
    assert torch.equal(table.crop, t2.crop) and torch.equal(table.clip_bounds, t2.clip_bounds), 'p010 and warp disagree on the crop values'
    px = F * H * W
    cases = {'p010': (lambda: ops.warp_p010(y, uv, table, out=(oy, ouv)), 6 * px),
             'warp_u16c3': (lambda: ops.warp(bgr, table, out=warped), 12 * px),
             'nv12': (lambda: ops.warp_nv12(y8, uv8, table, out=(oy8, ouv8)), 3 * px),
             'recipe': (lambda: recipe(y, uv, table, bgr, warped, oy, ouv), 6 * px)}
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
    rec['p010_over_warp_u16c3'] = round(rec['p010']['median_ms'] / rec['warp_u16c3']['median_ms'], 4)
    rec['p010_over_nv12'] = round(rec['p010']['median_ms'] / rec['nv12']['median_ms'], 4)
    rec['p010_over_recipe'] = round(rec['p010']['median_ms'] / rec['recipe']['median_ms'], 4)
    try:
        split = kernel_split(cases['p010'][0])
        rec['luma'] = {'median_ms': split['luma'], 'source': 'torch.profiler kernel records'}
        rec['chroma'] = {'median_ms': split['chroma'], 'source': 'torch.profiler kernel records'}
        rec['luma_over_warp_u16c3'] = round(split['luma'] / rec['warp_u16c3']['median_ms'], 4)
        rec['chroma_over_warp_u16c3'] = round(split['chroma'] / rec['warp_u16c3']['median_ms'], 4)
    except Exception as e:                     # (no kernel records on this stack: the totals above stand on their own)
        rec['split'] = f'unavailable: {type(e).__name__}: {e}'
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
