"""The P210 / Y210 calls (10-bit 4:2:2) against what they are measured by, in ONE process, alternating (HIP events around the launches only),
64 frames of 1920x1080, noise planes, a 16 x 16 mesh, a rectangle that keeps about 5 % off every side with an odd left and top:
  warp          ops.warp_p210 and ops.warp_p010 on the same cell table; per kernel (torch.profiler's kernel records): p210_chroma_footprint
                against p010_chroma_footprint (twice the samples) and against the luma kernel both share
  crop          ops.crop_resize_p210 and ops.crop_resize_p010 with the same rectangle back to size; per kernel: wide422_resize_kernel against
                hdr_uv_resize_kernel (twice the samples) and against hdr_luma_resize_kernel (the same bytes)
  pack          ops.unpack_y210 and ops.pack_y210 beside a device copy of the same bytes (torch's copy_ of the packed clip: it reads and
                writes what each of the two kernels reads and writes)
  packed        ops.warp_y210 and ops.crop_resize_y210: pack + unpack as a share of the packed calls (packed - planar per repetition)
One JSON line.  Before timing, the packed calls are checked against pack_y210 of the planar calls' planes, and the device-rectangle crop against
the host-rectangle one.

    python tools/time_p210.py [--reps 15] [--frames 64] [--out profiles/p210_time.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from meshflow_amd import ops, synthetic  # noqa: E402
from meshflow_amd.stabilizer import MeshFlowStabilizer  # noqa: E402
from time_p010 import noise, stats, timed  # noqa: E402

KERNELS = ('p210_chroma_footprint', 'p010_chroma_footprint', 'warp16c1_footprint', 'wide422_resize_kernel', 'hdr_uv_resize_kernel',
           'hdr_luma_resize_kernel', 'unpack_y210_kernel', 'pack_y210_kernel')


def same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def kernel_times(fns, calls=5):
    """{kernel name fragment: median device duration in ms} over `calls` calls of every function, from torch.profiler's kernel records."""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(calls):
            for fn in fns:
                fn()
        torch.cuda.synchronize()
    found = {k: [] for k in KERNELS}
    for e in prof.events():
        for frag in KERNELS:
            if frag in e.name and not (frag == 'pack_y210_kernel' and 'unpack_y210_kernel' in e.name):
                found[frag].append(float(getattr(e, 'device_time', None) or getattr(e, 'cuda_time', 0.0)) * 1e-3)
    return {k: {'median_ms': round(float(np.median(v)), 4), 'records': len(v)} for k, v in found.items() if v}


def run(F, reps, warmup, dev):
    H, W, R, C = 1080, 1920, 16, 16
    rect = (W // 20 | 1, H // 20 | 1, W - 1 - W // 20, H - 1 - H // 20)
    disp, hom = synthetic.motion(F, R, C, seed=0)
    s = MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, device=str(dev))
    d_disp = torch.from_numpy(disp).to(dev)
    d_stab = s._stabilized_vertex_displacements_device(d_disp, W, H, 0, hom)
    table = ops.cell_table(d_disp, d_stab, W, H, R, C)
    y, uv = noise((F, H, W), dev, 1, torch.uint16), noise((F, H, W // 2, 2), dev, 2, torch.uint16)
    uv420 = noise((F, H // 2, W // 2, 2), dev, 3, torch.uint16)
    oy, ouv, ouv420 = torch.empty_like(y), torch.empty_like(uv), torch.empty_like(uv420)
    packed = ops.pack_y210(y, uv)
    opacked, copied = torch.empty_like(packed), torch.empty_like(packed)
    ops.warp_p210(y, uv, table, out=(oy, ouv))
    torch.cuda.synchronize()
    table.check()
    assert same(ops.warp_y210(packed, table), ops.pack_y210(oy, ouv)), 'warp_y210 is not unpack, warp_p210, pack'
    cy, cuv = ops.crop_resize_p210(y, uv, rect)
    dy, duv, status = ops.crop_resize_p210(y, uv, torch.tensor(rect, dtype=torch.int32, device=dev))
    assert int(status.item()) == 0 and same(cy, dy) and same(cuv, duv), 'the host-rectangle and the device-rectangle crop disagree'
    assert same(ops.crop_resize_y210(packed, rect), ops.pack_y210(cy, cuv)), 'crop_resize_y210 is not unpack, crop_resize_p210, pack'
    del cy, cuv, dy, duv
    px = F * H * W
    crop_px = F * (rect[2] - rect[0] + 1) * (rect[3] - rect[1] + 1)
    cases = {'warp_p210': (lambda: ops.warp_p210(y, uv, table, out=(oy, ouv)), 8 * px),
             'warp_p010': (lambda: ops.warp_p010(y, uv420, table, out=(oy, ouv420)), 6 * px),
             'warp_y210': (lambda: ops.warp_y210(packed, table, out=opacked), 8 * px),
             'crop_p210': (lambda: ops.crop_resize_p210(y, uv, rect, out=(oy, ouv)), 4 * (px + crop_px)),
             'crop_p010': (lambda: ops.crop_resize_p010(y, uv420, rect, out=(oy, ouv420)), 3 * (px + crop_px)),
             'crop_y210': (lambda: ops.crop_resize_y210(packed, rect, out=opacked), 4 * (px + crop_px)),
             'unpack_y210': (lambda: ops.unpack_y210(packed, out=(oy, ouv)), 8 * px),
             'pack_y210': (lambda: ops.pack_y210(y, uv, out=opacked), 8 * px),
             'device_copy': (lambda: copied.copy_(packed), 8 * px)}
    for _ in range(warmup):
        for fn, _ in cases.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):                      # alternating: all see the same clocks and the same neighbours on the machine
        for k, (fn, _) in cases.items():
            ms[k].append(timed(fn))
    rec = {'frames': F, 'H': H, 'W': W, 'mesh': [R, C], 'rectangle': list(rect), 'reps': reps, 'warmup': warmup}
    for k, (_, nbytes) in cases.items():
        rec[k] = stats(ms[k], nbytes)
        rec[k]['TB_per_s'] = round(nbytes / (rec[k]['median_ms'] * 1e-3) / 1e12, 3)
    for call, planar in (('warp_y210', 'warp_p210'), ('crop_y210', 'crop_p210')):
        d = float(np.median([a - b for a, b in zip(ms[call], ms[planar])]))
        rec[call]['pack_unpack_ms'] = round(d, 4)
        rec[call]['pack_unpack_share'] = round(d / rec[call]['median_ms'], 4)
    try:
        k = kernel_times([cases[c][0] for c in ('warp_p210', 'warp_p010', 'crop_p210', 'crop_p010', 'unpack_y210', 'pack_y210')])
        rec['kernels'] = k
        med = lambda name: k[name]['median_ms']  # noqa: E731
        rec['p210_chroma_over_p010_chroma_warp'] = round(med('p210_chroma_footprint') / med('p010_chroma_footprint'), 4)
        rec['p210_chroma_over_luma_warp'] = round(med('p210_chroma_footprint') / med('warp16c1_footprint'), 4)
        rec['wide422_over_hdr_uv_resize'] = round(med('wide422_resize_kernel') / med('hdr_uv_resize_kernel'), 4)
        rec['wide422_over_hdr_luma_resize'] = round(med('wide422_resize_kernel') / med('hdr_luma_resize_kernel'), 4)
    except Exception as e:                     # (no kernel records on this stack: the totals above stand on their own)
        rec['kernels'] = f'unavailable: {type(e).__name__}: {e}'
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--frames', type=int, default=64)
    ap.add_argument('--out', default=None, help='append the JSON line to this file as well')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_p210.py needs a GPU: nothing is measured without one')
    rec = run(args.frames, max(args.reps, 5), args.warmup, torch.device('cuda:0'))
    line = json.dumps(rec)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
