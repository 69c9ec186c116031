"""Single-channel uint8 warp and crop-resize against the BGR ones, in ONE process, alternating, on the same tables (HIP events around
the launches only).  Shapes: cfg2 geometry (300 x 1920x1080, 16x16 mesh), cfg3 (600 frames, 32x32) and a 150-frame 4K shard (16x16).
Frames: uint8 noise generated on the host from a seed; the BGR frames repeat the grey one three times.  Timed per shape:
  warp_u8c1, warp_u8c3              the two warps on the same table
  workaround                        what a caller without the grey kernels does: expand to BGR -> u8c3 warp -> channel 0 (torch copies)
  crop_resize_u8c1, crop_resize_u8c3
One JSON line per shape (median and spread in ms, algorithmic bytes, fraction of the 8 TB/s peak).  --host adds, at cfg2, the host-to-host
`stabilize_clip(crop=True, keep_uncropped=False)` frames/s of the grey clip against the BGR clip (alternating, wall clock).

    python tools/time_grey.py [--reps 15] [--shapes cfg2,cfg3,4k] [--host 3]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from meshflow_amd import ops, synthetic  # noqa: E402
from meshflow_amd.stabilizer import MeshFlowStabilizer  # noqa: E402

SHAPES = {'cfg2': (1080, 1920, 300, 16, 16), 'cfg3': (1080, 1920, 600, 32, 32), '4k': (2160, 3840, 150, 16, 16)}
PEAK = 8.0e12


def noise_frames(n, H, W, dev, seed):
    """(grey uint8 (n, H, W), BGR uint8 (n, H, W, 3) = the grey frame three times) on the device."""
    g = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(seed)
    for i in range(0, n, 8):
        a = rng.integers(0, 256, (min(8, n - i), H, W), dtype=np.uint8)
        g[i:i + len(a)].copy_(torch.from_numpy(a))
    return g, g.unsqueeze(-1).expand(n, H, W, 3).contiguous()


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
    g, c = noise_frames(F, H, W, dev, seed=1)
    og, oc = torch.empty_like(g), torch.empty_like(c)
    table = ops.cell_table(d_disp, d_stab, W, H, R, C)
    ops.warp(g, table, out=og)
    ops.warp(c, table, out=oc)
    torch.cuda.synchronize()
    table.check()
    assert torch.equal(og, oc[..., 0]), 'grey warp differs from channel 0 of the BGR warp'
    rect = tuple(int(v) for v in table.clip_bounds.tolist())
    if rect[2] < rect[0] or rect[3] < rect[1]:
        rect = (W // 50, H // 50, W - 1 - W // 50, H - 1 - H // 50)
    cg, cc = torch.empty_like(g), torch.empty_like(c)
    wa_in, wa_mid, wa_out = torch.empty_like(c), torch.empty_like(c), torch.empty_like(g)

    def workaround():
        wa_in.copy_(g.unsqueeze(-1).expand(F, H, W, 3))
        ops.warp(wa_in, table, out=wa_mid)
        wa_out.copy_(wa_mid[..., 0])

    ms = {'warp_u8c1': [], 'warp_u8c3': [], 'workaround': [], 'crop_resize_u8c1': [], 'crop_resize_u8c3': []}
    for i in range(reps + 2):                                 # two warm-up rounds, then alternating
        r = {'warp_u8c1': timed(lambda: ops.warp(g, table, out=og)),
             'warp_u8c3': timed(lambda: ops.warp(c, table, out=oc)),
             'workaround': timed(workaround),
             'crop_resize_u8c1': timed(lambda: ops.crop_resize(og, rect, out=cg)),
             'crop_resize_u8c3': timed(lambda: ops.crop_resize(oc, rect, out=cc))}
        if i >= 2:
            for k, v in r.items():
                ms[k].append(v)
    assert torch.equal(wa_out, og) and torch.equal(cg, cc[..., 0])
    px = F * H * W
    res = {'shape': name, 'frames': F, 'H': H, 'W': W, 'R': R, 'C': C, 'reps': reps, 'crop_rect': rect}
    for k, v in ms.items():
        res[k] = stats(v, 2 * px * (1 if k.endswith('c1') else 3) + (2 * px * 4 if k == 'workaround' else 0))
    res['warp_u8c1_over_u8c3'] = round(res['warp_u8c1']['median_ms'] / res['warp_u8c3']['median_ms'], 3)
    res['warp_u8c1_over_workaround'] = round(res['warp_u8c1']['median_ms'] / res['workaround']['median_ms'], 3)
    res['crop_resize_u8c1_over_u8c3'] = round(res['crop_resize_u8c1']['median_ms'] / res['crop_resize_u8c3']['median_ms'], 3)
    print(json.dumps(res), flush=True)
    del g, c, og, oc, cg, cc, wa_in, wa_mid, wa_out, table
    torch.cuda.empty_cache()
    return res


def run_host(reps, dev):
    """Host-to-host stabilize_clip(crop=True, keep_uncropped=False) at cfg2: grey against BGR frames/s, alternating."""
    H, W, F, R, C = SHAPES['cfg2']
    disp, hom = synthetic.motion(F, R, C, seed=0)
    s = MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, device=str(dev))
    g = np.random.default_rng(1).integers(0, 256, (F, H, W), dtype=np.uint8)
    c = np.ascontiguousarray(np.repeat(g[..., None], 3, axis=-1))
    gl, cl = list(g), list(c)
    secs = {'grey': [], 'bgr': []}
    kept = {}
    for i in range(reps + 1):                                 # one warm-up round
        for k, frames in (('grey', gl), ('bgr', cl)):
            res = None                                        # (the previous call's output is freed OUTSIDE the timed interval)
            t0 = time.perf_counter()
            res = s.stabilize_clip(frames, disp, hom, crop=True, keep_uncropped=False)
            dt = time.perf_counter() - t0
            if i >= 1:
                secs[k].append(dt)
            kept[k] = [f.copy() for f in res[4][:2]]
    assert np.array_equal(np.stack(kept['grey']), np.stack(kept['bgr'])[..., 0])
    out = {'shape': 'cfg2_host_stabilize_clip_crop', 'frames': F, 'H': H, 'W': W, 'reps': reps}
    for k, v in secs.items():
        med = float(np.median(v))
        out[k] = {'median_s': round(med, 4), 'min_s': round(float(np.min(v)), 4), 'max_s': round(float(np.max(v)), 4),
                  'frames_per_s': round(F / med, 1)}
    out['grey_over_bgr_frames_per_s'] = round(out['grey']['frames_per_s'] / out['bgr']['frames_per_s'], 3)
    print(json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--shapes', default='cfg2,cfg3,4k')
    ap.add_argument('--host', type=int, default=0, help='repetitions of the host-to-host measurement (0: skip)')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    for name in [n for n in args.shapes.split(',') if n]:
        run(name, args.reps, dev)
    if args.host:
        run_host(args.host, dev)


if __name__ == '__main__':
    main()
