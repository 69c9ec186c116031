"""The 4:2:2 calls against what they are measured by, in ONE process, alternating, on the same table (HIP events around the launches only):
  nv16          ops.warp_nv16, both launches (the grey warp of the luma planes, then nv16_chroma_footprint)
  nv12          ops.warp_nv12 on the same table and luma planes, chroma rows halved (nv12_chroma_footprint)
  luma          their first launch alone: ops.warp on the luma planes (the same kernel, the same arguments)
  chroma16 / chroma12
                their second launches: the C ABI has no entry that launches them alone, so these are nv16 - luma and nv12 - luma of the same
                repetition -- the launches run back to back on one stream and each fills the device.  (Kernel times of their own: run this
                tool under `rocprofv3 --kernel-trace --stats`.)
  unpack / pack ops.unpack_422 / ops.pack_422 of the packed clip (UYVY), all buffers from the allocator: the wide path
  luma_bgr      ops.luma on a BGR clip of the same pixel count: the streaming kernel the two were built after
  copy          a device-to-device copy of the packed clip (Tensor.copy_)
  packed        ops.warp_packed_422: unpack, nv16, pack, temporaries included
Shapes: 64 frames of 1920x1080 and of 3840x2160, 16x16 mesh.  Planes: noise generated on the host from a seed.  One JSON line per shape: median
and spread in ms per case, algorithmic bytes (every sample read once and written once), bytes per second, the fraction of the 8 TB/s peak, and
the ratios chroma16 / chroma12, chroma16 / luma and (unpack + pack) / packed (medians).  Before timing, the luma output is checked once against
ops.warp (equal bytes), pack(unpack(x)) against x, and the packed warp against pack(nv16(unpack(x))).

    python tools/time_nv16.py [--reps 15] [--shapes 1080p,4k] [--out profiles/nv16_time.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from meshflow_amd import ops, synthetic  # noqa: E402
from meshflow_amd.stabilizer import MeshFlowStabilizer  # noqa: E402

SHAPES = {'1080p': (1080, 1920, 64, 16, 16), '4k': (2160, 3840, 64, 16, 16), 'tiny': (96, 128, 4, 4, 4)}
PEAK = 8.0e12
ORDER = 'uyvy'


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
            'algorithmic_bytes': nbytes, 'bytes_per_s': round(nbytes / (med * 1e-3), 1), 'peak_fraction': round(nbytes / (med * 1e-3) / PEAK, 4)}


def run(name, reps, warmup, dev):
    H, W, F, R, C = SHAPES[name]
    disp, hom = synthetic.motion(F, R, C, seed=0)
    s = MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, device=str(dev))
    d_disp = torch.from_numpy(disp).to(dev)
    d_stab = s._stabilized_vertex_displacements_device(d_disp, W, H, 0, hom)
    y, uv16 = noise((F, H, W), dev, 1), noise((F, H, W // 2, 2), dev, 2)
    uv12 = uv16[:, ::2].contiguous()
    oy, ouv16, ouv12, og = torch.empty_like(y), torch.empty_like(uv16), torch.empty_like(uv12), torch.empty_like(y)
    packed = ops.pack_422(y, uv16, ORDER)
    packed_out, packed_copy = torch.empty_like(packed), torch.empty_like(packed)
    py, puv = torch.empty_like(y), torch.empty_like(uv16)
    bgr = noise((F, H, W, 3), dev, 3)
    bgr_luma = torch.empty_like(y)
    table = ops.cell_table(d_disp, d_stab, W, H, R, C)
    ops.warp_nv16(y, uv16, table, out=(oy, ouv16))
    torch.cuda.synchronize()
    table.check()
    t2 = ops.cell_table(d_disp, d_stab, W, H, R, C)
    ops.warp(y, t2, (81,), out=og)
    torch.cuda.synchronize()
    assert torch.equal(oy, og), 'the luma planes and the grey warp disagree'
    assert torch.equal(table.crop, t2.crop) and torch.equal(table.clip_bounds, t2.clip_bounds), 'nv16 and warp disagree on the crop values'
    ops.unpack_422(packed, ORDER, out=(py, puv))
    assert torch.equal(py, y) and torch.equal(puv, uv16) and torch.equal(ops.pack_422(py, puv, ORDER), packed), 'pack / unpack round trip'
    ops.warp_packed_422(packed, table, ORDER, out=packed_out)
    assert torch.equal(packed_out, ops.pack_422(oy, ouv16, ORDER)), 'the packed warp is not pack(nv16(unpack))'
    px = F * H * W
    cases = {'nv16': (lambda: ops.warp_nv16(y, uv16, table, out=(oy, ouv16)), 4 * px),
             'nv12': (lambda: ops.warp_nv12(y, uv12, table, out=(oy, ouv12)), 3 * px),
             'luma': (lambda: ops.warp(y, table, (81,), out=og), 2 * px),
             'unpack': (lambda: ops.unpack_422(packed, ORDER, out=(py, puv)), 4 * px),
             'pack': (lambda: ops.pack_422(y, uv16, ORDER, out=packed_copy), 4 * px),
             'luma_bgr': (lambda: ops.luma(bgr, out=bgr_luma), 4 * px),
             'copy': (lambda: packed_copy.copy_(packed), 4 * px),
             'packed': (lambda: ops.warp_packed_422(packed, table, ORDER, out=packed_out), 12 * px)}
    for _ in range(warmup):
        for fn, _ in cases.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):                      # alternating: all see the same clocks and the same neighbours on the machine
        for k, (fn, _) in cases.items():
            ms[k].append(timed(fn))
    rec = {'shape': name, 'frames': F, 'H': H, 'W': W, 'mesh': [R, C], 'reps': reps, 'warmup': warmup, 'order': ORDER}
    for k, (_, nbytes) in cases.items():
        rec[k] = stats(ms[k], nbytes)
    rec['packed']['bytes_note'] = 'unpack 4 + nv16 4 + pack 4 B/px; the temporaries come from the caching allocator inside the window'
    for key, whole, nbytes in (('chroma16', 'nv16', 2 * px), ('chroma12', 'nv12', px)):
        rec[key] = stats([a - b for a, b in zip(ms[whole], ms['luma'])], nbytes)
        rec[key]['derived'] = whole + ' - luma per repetition'
    rec['chroma16_over_chroma12'] = round(rec['chroma16']['median_ms'] / rec['chroma12']['median_ms'], 4)
    rec['chroma16_over_luma'] = round(rec['chroma16']['median_ms'] / rec['luma']['median_ms'], 4)
    rec['pack_plus_unpack_over_packed'] = round((rec['unpack']['median_ms'] + rec['pack']['median_ms']) / rec['packed']['median_ms'], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--shapes', default='1080p,4k')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_nv16.py needs a GPU: nothing is measured without one')
    dev = torch.device('cuda:0')
    for name in args.shapes.split(','):
        rec = run(name, args.reps, args.warmup, dev)
        line = json.dumps(rec)
        print(line, flush=True)
        if args.out:
            with open(args.out, 'a') as f:
                f.write(line + '\n')
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
