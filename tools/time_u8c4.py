"""4-channel uint8 warp and crop-resize against the BGR ones, in ONE process, alternating, on the same tables (HIP events around the
launches only).  Shapes: cfg2 geometry (300 x 1920x1080, 16x16 mesh), cfg3 (600 frames, 32x32) and a 150-frame 4K shard (16x16).  Frames:
uint8 noise generated on the host from a seed; the BGR frames are channels 0-2 of the BGRA ones.  Timed per shape:
  warp_u8c4, warp_u8c3              the two warps on the same table
  workaround                        what a caller without the 4-channel kernels does: split into BGR + alpha -> u8c3 warp + u8c1 warp ->
                                    interleave (torch copies)
  crop_resize_u8c4, crop_resize_u8c3                same size
  crop_resize_to_u8c4, crop_resize_to_u8c3          4K -> 1080p (the 4k shape only)
One JSON line per shape (median and spread in ms, algorithmic bytes -- every input byte read once, every output byte written once --, the
fraction of the 8 TB/s peak, and the ratios the targets are stated in).

    python tools/time_u8c4.py [--reps 15] [--shapes cfg2,cfg3,4k]"""
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
    """(BGRA uint8 (n, H, W, 4), BGR uint8 (n, H, W, 3) = its channels 0-2) on the device."""
    x = torch.empty((n, H, W, 4), dtype=torch.uint8, device=dev)
    rng = np.random.default_rng(seed)
    for i in range(0, n, 8):
        a = rng.integers(0, 256, (min(8, n - i), H, W, 4), dtype=np.uint8)
        x[i:i + len(a)].copy_(torch.from_numpy(a))
    return x, x[..., :3].contiguous()


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
    x, c = noise_frames(F, H, W, dev, seed=1)
    ox, oc = torch.empty_like(x), torch.empty_like(c)
    table = ops.cell_table(d_disp, d_stab, W, H, R, C)
    ops.warp(x, table, out=ox)
    ops.warp(c, table, out=oc)
    torch.cuda.synchronize()
    table.check()
    assert torch.equal(ox[..., :3], oc), 'channels 0-2 of the 4-channel warp differ from the BGR warp'
    rect = tuple(int(v) for v in table.clip_bounds.tolist())
    if rect[2] < rect[0] or rect[3] < rect[1]:
        rect = (W // 50, H // 50, W - 1 - W // 50, H - 1 - H // 50)
    cx, cc = torch.empty_like(x), torch.empty_like(c)
    wa_c, wa_a = torch.empty_like(c), torch.empty((F, H, W), dtype=torch.uint8, device=dev)
    wa_oc, wa_oa, wa_out = torch.empty_like(c), torch.empty_like(wa_a), torch.empty_like(x)

    def workaround():
        wa_c.copy_(x[..., :3])
        wa_a.copy_(x[..., 3])
        ops.warp(wa_c, table, out=wa_oc)
        ops.warp(wa_a, table, (0,), out=wa_oa)
        wa_out[..., :3].copy_(wa_oc)
        wa_out[..., 3].copy_(wa_oa)

    fns = {'warp_u8c4': lambda: ops.warp(x, table, out=ox),
           'warp_u8c3': lambda: ops.warp(c, table, out=oc),
           'workaround': workaround,
           'crop_resize_u8c4': lambda: ops.crop_resize(ox, rect, out=cx),
           'crop_resize_u8c3': lambda: ops.crop_resize(oc, rect, out=cc)}
    size = (1920, 1080) if name == '4k' else None
    if size:
        tx = torch.empty((F, size[1], size[0], 4), dtype=torch.uint8, device=dev)
        tc = torch.empty((F, size[1], size[0], 3), dtype=torch.uint8, device=dev)
        fns['crop_resize_to_u8c4'] = lambda: ops.crop_resize(ox, rect, out=tx, size=size)
        fns['crop_resize_to_u8c3'] = lambda: ops.crop_resize(oc, rect, out=tc, size=size)
    ms = {k: [] for k in fns}
    for i in range(reps + 2):                                 # two warm-up rounds, then alternating
        r = {k: timed(fn) for k, fn in fns.items()}
        if i >= 2:
            for k, v in r.items():
                ms[k].append(v)
    assert torch.equal(wa_out, ox) and torch.equal(cx[..., :3], cc)
    if size:
        assert torch.equal(tx[..., :3], tc)
    px, opx = F * H * W, F * (size[0] * size[1] if size else 0)
    nbytes = {'warp_u8c4': 8 * px, 'warp_u8c3': 6 * px, 'workaround': 8 * px + 2 * 8 * px, 'crop_resize_u8c4': 8 * px,
              'crop_resize_u8c3': 6 * px, 'crop_resize_to_u8c4': 4 * px + 4 * opx, 'crop_resize_to_u8c3': 3 * px + 3 * opx}
    res = {'shape': name, 'frames': F, 'H': H, 'W': W, 'R': R, 'C': C, 'reps': reps, 'crop_rect': rect}
    for k, v in ms.items():
        res[k] = stats(v, nbytes[k])
    res['warp_u8c4_over_u8c3'] = round(res['warp_u8c4']['median_ms'] / res['warp_u8c3']['median_ms'], 3)
    res['warp_u8c4_over_workaround'] = round(res['warp_u8c4']['median_ms'] / res['workaround']['median_ms'], 3)
    res['crop_resize_u8c4_over_u8c3'] = round(res['crop_resize_u8c4']['median_ms'] / res['crop_resize_u8c3']['median_ms'], 3)
    if size:
        res['crop_resize_to_u8c4_over_u8c3'] = round(res['crop_resize_to_u8c4']['median_ms'] / res['crop_resize_to_u8c3']['median_ms'], 3)
    print(json.dumps(res), flush=True)
    del x, c, ox, oc, cx, cc, wa_c, wa_a, wa_oc, wa_oa, wa_out, table
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--shapes', default='cfg2,cfg3,4k')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    for name in [n for n in args.shapes.split(',') if n]:
        run(name, args.reps, dev)


if __name__ == '__main__':
    main()
