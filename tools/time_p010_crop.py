"""The P010 crop-resize (ops.crop_resize_p010: the luma tables and kernel, then the chroma tables and kernel) against what it is measured by, in
ONE process, alternating, with the same host rectangle (HIP events around the launches only):
  p010          ops.crop_resize_p010, all four launches
  crop_u16c3    the uint16 BGR crop-resize of a clip of the same size (one pixel per thread, 12-byte taps)
  nv12          the 8-bit ops.crop_resize_nv12 of a clip of the same size
  recipe        what a resident P010 clip pays without the call: P010 -> uint16 BGR with torch ops (tools/time_p010.py's conversion), the
                u16c3 crop-resize, BGR -> P010, in chunks of 30 frames so that the float temporaries stay small
Shapes: cfg2 geometry (300 x 1920x1080 cropped back to size), a 150-frame 4K shard cropped back to size, and the same shard cropped to
1920x1080.  The rectangle keeps about 5 % off every side and has an odd left and top.  Planes: noise generated on the host from a seed, the
whole 16-bit range.  One JSON line per shape: median and spread in ms per case, algorithmic bytes (every output sample written once, every
crop sample read once), the fraction of the 8 TB/s peak, and the ratios p010 / crop_u16c3, p010 / nv12 and p010 / recipe (medians).  Before
timing, the luma output of the first frames is checked once against channel 0 of ops.crop_resize on stack(Y, Y, Y), and both planes against
ops.crop_resize_p010 with the rectangle on the device.
Each shape is a GPU step of its own; run one per command under a time limit of its own, chained so that a failure ends the chain:

    timeout -k 10 300 python tools/time_p010_crop.py --shapes cfg2 --out profiles/p010_crop_time.jsonl && \\
    timeout -k 10 300 python tools/time_p010_crop.py --shapes 4k --out profiles/p010_crop_time.jsonl && \\
    timeout -k 10 300 python tools/time_p010_crop.py --shapes 4k_to_1080p --out profiles/p010_crop_time.jsonl"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from meshflow_amd import ops  # noqa: E402
from time_p010 import CHUNK, bgr_to_p010, noise, p010_to_bgr, stats, timed  # noqa: E402

# name -> (H, W, frames, (out_W, out_H))
SHAPES = {'cfg2': (1080, 1920, 300, (1920, 1080)), '4k': (2160, 3840, 150, (3840, 2160)), '4k_to_1080p': (2160, 3840, 150, (1920, 1080))}


def rectangle(W, H):
    return (W // 20 | 1, H // 20 | 1, W - 1 - W // 20, H - 1 - H // 20)


def recipe(y, uv, rect, size, bgr, cropped, oy, ouv):
    for i in range(0, y.shape[0], CHUNK):
        p010_to_bgr(y[i:i + CHUNK], uv[i:i + CHUNK], bgr[i:i + CHUNK])
    ops.crop_resize(bgr, rect, out=cropped, size=size)
    for i in range(0, y.shape[0], CHUNK):
        bgr_to_p010(cropped[i:i + CHUNK], oy[i:i + CHUNK], ouv[i:i + CHUNK])


def same(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def run(name, reps, warmup, dev):
    H, W, F, (oW, oH) = SHAPES[name]
    size = (oW, oH)
    rect = rectangle(W, H)
    cw, ch = rect[2] - rect[0] + 1, rect[3] - rect[1] + 1
    bounds = torch.tensor(rect, dtype=torch.int32, device=dev)
    y, uv = noise((F, H, W), dev, 1, torch.uint16), noise((F, H // 2, W // 2, 2), dev, 2, torch.uint16)
    oy = torch.empty((F, oH, oW), dtype=torch.uint16, device=dev)
    ouv = torch.empty((F, oH // 2, oW // 2, 2), dtype=torch.uint16, device=dev)
    y8, uv8 = noise((F, H, W), dev, 3, torch.uint8), noise((F, H // 2, W // 2, 2), dev, 4, torch.uint8)
    oy8 = torch.empty((F, oH, oW), dtype=torch.uint8, device=dev)
    ouv8 = torch.empty((F, oH // 2, oW // 2, 2), dtype=torch.uint8, device=dev)
    bgr = torch.empty((F, H, W, 3), dtype=torch.uint16, device=dev)
    cropped = torch.empty((F, oH, oW, 3), dtype=torch.uint16, device=dev)
    ops.crop_resize_p010(y, uv, rect, size=size, out=(oy, ouv))
    dev_y, dev_uv, status = ops.crop_resize_p010(y, uv, bounds, size=size)
    m = min(F, 4)
    for k in range(3):
        bgr[:m, ..., k].copy_(y[:m])
    ops.crop_resize(bgr[:m], rect, out=cropped[:m], size=size)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert np.array_equal(oy[:m].cpu().numpy(), cropped[:m, ..., 0].cpu().numpy()), 'the luma planes and the u16c3 crop-resize disagree'
    assert same(oy, dev_y) and same(ouv, dev_uv), 'the host-rectangle and the device-rectangle call disagree'
    del dev_y, dev_uv
    out_px, crop_px = F * oH * oW, F * cw * ch
    cases = {'p010': (lambda: ops.crop_resize_p010(y, uv, rect, size=size, out=(oy, ouv)), 3 * (out_px + crop_px)),
             'crop_u16c3': (lambda: ops.crop_resize(bgr, rect, out=cropped, size=size), 6 * (out_px + crop_px)),
             'nv12': (lambda: ops.crop_resize_nv12(y8, uv8, rect, size=size, out=(oy8, ouv8)), 3 * (out_px + crop_px) // 2),
             'recipe': (lambda: recipe(y, uv, rect, size, bgr, cropped, oy, ouv), 3 * (out_px + crop_px))}
    for _ in range(warmup):
        for fn, _ in cases.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):                      # alternating: all see the same clocks and the same neighbours on the machine
        for k, (fn, _) in cases.items():
            ms[k].append(timed(fn))
    rec = {'shape': name, 'frames': F, 'H': H, 'W': W, 'rectangle': list(rect), 'out_W': oW, 'out_H': oH, 'reps': reps, 'warmup': warmup,
           'taps': 'direct, no LDS'}
    for k, (_, nbytes) in cases.items():
        rec[k] = stats(ms[k], nbytes)
    rec['p010_over_crop_u16c3'] = round(rec['p010']['median_ms'] / rec['crop_u16c3']['median_ms'], 4)
    rec['p010_over_nv12'] = round(rec['p010']['median_ms'] / rec['nv12']['median_ms'], 4)
    rec['p010_over_recipe'] = round(rec['p010']['median_ms'] / rec['recipe']['median_ms'], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--shapes', default='cfg2,4k,4k_to_1080p')
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
