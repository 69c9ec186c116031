"""The NV16 crop-resize (ops.crop_resize_nv16: the grey crop-resize of the luma planes, then the 4:2:2 chroma launches) against what it is
measured by, in ONE process, alternating, with the same host rectangle (HIP events around the launches only):
  nv16          ops.crop_resize_nv16, all launches (luma tables + luma kernel, chroma x tables + chroma kernel)
  luma          its luma launches alone: ops.crop_resize on the luma planes (the same kernels, the same arguments)
  chroma        its chroma launches: the C ABI has no entry that launches them alone, so this is nv16 - luma of the same repetition -- the
                launches run back to back on one stream and each fills the device
  nv12          ops.crop_resize_nv12 on the same luma and every second chroma row, and nv12_chroma = nv12 - luma of the same repetition
  packed        ops.crop_resize_packed_422 of the same clip as UYVY: unpack, the nv16 call, pack; pack_unpack = packed - nv16 per repetition
  recipe        what a resident NV16 clip pays without the call: NV16 -> BGR with torch ops (BT.601 limited range, chroma repeated along x), the
                u8c3 crop-resize, BGR -> NV16 (chroma averaged along x), in chunks of 30 frames so that the float temporaries stay small
Shapes: 64 frames of 1920x1080 cropped back to size, 64 frames of 4K cropped back to size, and the 4K clip cropped to 1920x1080 (the frame
counts of tools/time_nv16.py).  The rectangle keeps about 5 % off every side and has an odd left and top.  Planes: noise generated on the host
from a seed.  One JSON line per shape: median and spread in ms per case, algorithmic bytes (every output sample written once, every crop sample
read once), the fraction of the 8 TB/s peak, and the ratios chroma / luma, chroma / nv12_chroma, pack_unpack / packed and nv16 / recipe
(medians).  Before timing, the luma output is checked once against ops.crop_resize (equal bytes), both planes against ops.crop_resize_nv16 with
the rectangle on the device, and the packed call against pack_422 of the nv16 call's planes.

    python tools/time_nv16_crop.py [--reps 15] [--shapes 1080p,4k,4k_to_1080p] [--out profiles/nv16_crop_time.jsonl]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

from meshflow_amd import ops  # noqa: E402
from time_nv12 import CHUNK, noise, stats, timed  # noqa: E402

# name -> (H, W, frames, (out_W, out_H))
SHAPES = {'1080p': (1080, 1920, 64, (1920, 1080)), '4k': (2160, 3840, 64, (3840, 2160)), '4k_to_1080p': (2160, 3840, 64, (1920, 1080)),
          'tiny': (97, 128, 4, (96, 65))}
ORDER = 'uyvy'


def rectangle(W, H):
    return (W // 20 | 1, H // 20 | 1, W - 1 - W // 20, H - 1 - H // 20)


def nv16_to_bgr(y, uv, out):
    """BT.601 limited range, chroma repeated along x; out: (m, H, W, 3) uint8."""
    yf = (y.float() - 16.0) * 1.164383
    c = (uv.float() - 128.0).repeat_interleave(2, dim=2)
    u, v = c[..., 0], c[..., 1]
    out[..., 0] = (yf + 2.017232 * u).round_().clamp_(0, 255)
    out[..., 1] = (yf - 0.391762 * u - 0.812968 * v).round_().clamp_(0, 255)
    out[..., 2] = (yf + 1.596027 * v).round_().clamp_(0, 255)


def bgr_to_nv16(bgr, y, uv):
    b, g, r = bgr[..., 0].float(), bgr[..., 1].float(), bgr[..., 2].float()
    y.copy_((16.0 + 0.256788 * r + 0.504129 * g + 0.097906 * b).round_().clamp_(0, 255))
    cu = 128.0 - 0.148223 * r - 0.290993 * g + 0.439216 * b
    cv = 128.0 + 0.439216 * r - 0.367788 * g - 0.071427 * b
    c = torch.stack([cu, cv], dim=-1)
    uv.copy_(((c[:, :, 0::2] + c[:, :, 1::2]) * 0.5).round_().clamp_(0, 255))


def recipe(y, uv, rect, size, bgr, cropped, oy, ouv):
    for i in range(0, y.shape[0], CHUNK):
        nv16_to_bgr(y[i:i + CHUNK], uv[i:i + CHUNK], bgr[i:i + CHUNK])
    ops.crop_resize(bgr, rect, out=cropped, size=size)
    for i in range(0, y.shape[0], CHUNK):
        bgr_to_nv16(cropped[i:i + CHUNK], oy[i:i + CHUNK], ouv[i:i + CHUNK])


def run(name, reps, warmup, dev):
    H, W, F, (oW, oH) = SHAPES[name]
    rect = rectangle(W, H)
    cw, ch = rect[2] - rect[0] + 1, rect[3] - rect[1] + 1
    bounds = torch.tensor(rect, dtype=torch.int32, device=dev)
    y, uv = noise((F, H, W), dev, 1), noise((F, H, W // 2, 2), dev, 2)
    H12, oH12 = H // 2 * 2, oH // 2 * 2                                 # (the NV12 call on the same luma: even sizes)
    y12, uv12 = y[:, :H12].contiguous(), uv[:, 0:H12:2].contiguous()
    rect12 = (rect[0], rect[1], rect[2], min(rect[3], H12 - 1))
    packed = ops.pack_422(y, uv, ORDER)
    oy = torch.empty((F, oH, oW), dtype=torch.uint8, device=dev)
    ouv = torch.empty((F, oH, oW // 2, 2), dtype=torch.uint8, device=dev)
    oy12 = torch.empty((F, oH12, oW), dtype=torch.uint8, device=dev)
    ouv12 = torch.empty((F, oH12 // 2, oW // 2, 2), dtype=torch.uint8, device=dev)
    og = torch.empty_like(oy)
    opacked = torch.empty((F, oH, oW, 2), dtype=torch.uint8, device=dev)
    bgr = torch.empty((F, H, W, 3), dtype=torch.uint8, device=dev)
    cropped = torch.empty((F, oH, oW, 3), dtype=torch.uint8, device=dev)
    ops.crop_resize_nv16(y, uv, rect, size=(oW, oH), out=(oy, ouv))
    ops.crop_resize(y, rect, out=og, size=(oW, oH))
    dev_y, dev_uv, status = ops.crop_resize_nv16(y, uv, bounds, size=(oW, oH))
    ops.crop_resize_packed_422(packed, rect, ORDER, size=(oW, oH), out=opacked)
    torch.cuda.synchronize()
    assert int(status.item()) == 0
    assert torch.equal(oy, og), 'the luma planes and the grey crop-resize disagree'
    assert torch.equal(oy, dev_y) and torch.equal(ouv, dev_uv), 'the host-rectangle and the device-rectangle call disagree'
    assert torch.equal(opacked, ops.pack_422(oy, ouv, ORDER)), 'the packed call is not unpack, crop_resize_nv16, pack'
    del dev_y, dev_uv
    out_px, crop_px = F * oH * oW, F * cw * ch
    out_px12, crop_px12 = F * oH12 * oW, F * cw * (rect12[3] - rect12[1] + 1)
    cases = {'nv16': (lambda: ops.crop_resize_nv16(y, uv, rect, size=(oW, oH), out=(oy, ouv)), 2 * (out_px + crop_px)),
             'luma': (lambda: ops.crop_resize(y, rect, out=og, size=(oW, oH)), out_px + crop_px),
             'nv12': (lambda: ops.crop_resize_nv12(y12, uv12, rect12, size=(oW, oH12), out=(oy12, ouv12)), 3 * (out_px12 + crop_px12) // 2),
             'luma12': (lambda: ops.crop_resize(y12, rect12, out=oy12, size=(oW, oH12)), out_px12 + crop_px12),
             'packed': (lambda: ops.crop_resize_packed_422(packed, rect, ORDER, size=(oW, oH), out=opacked), 2 * (out_px + crop_px)),
             'recipe': (lambda: recipe(y, uv, rect, (oW, oH), bgr, cropped, oy, ouv), 2 * (out_px + crop_px))}
    for _ in range(warmup):
        for fn, _ in cases.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in cases}
    for _ in range(reps):                      # alternating: all see the same clocks and the same neighbours on the machine
        for k, (fn, _) in cases.items():
            ms[k].append(timed(fn))
    rec = {'shape': name, 'frames': F, 'H': H, 'W': W, 'rectangle': list(rect), 'out_W': oW, 'out_H': oH, 'reps': reps, 'warmup': warmup,
           'chroma_taps': 'direct, no LDS', 'order': ORDER}
    for k, (_, nbytes) in cases.items():
        rec[k] = stats(ms[k], nbytes)
    rec['chroma'] = stats([a - b for a, b in zip(ms['nv16'], ms['luma'])], out_px + crop_px)
    rec['chroma']['derived'] = 'nv16 - luma per repetition'
    rec['nv12_chroma'] = stats([a - b for a, b in zip(ms['nv12'], ms['luma12'])], (out_px12 + crop_px12) // 2)
    rec['nv12_chroma']['derived'] = 'nv12 - luma12 per repetition'
    # unpack reads the clip and writes the pair, pack reads the resized pair and writes the packed output: 2 bytes moved per byte, twice
    rec['pack_unpack'] = stats([a - b for a, b in zip(ms['packed'], ms['nv16'])], 4 * F * (H * W + oH * oW))
    rec['pack_unpack']['derived'] = 'packed - nv16 per repetition'
    rec['chroma_over_luma'] = round(rec['chroma']['median_ms'] / rec['luma']['median_ms'], 4)
    rec['chroma_over_nv12_chroma'] = round(rec['chroma']['median_ms'] / rec['nv12_chroma']['median_ms'], 4)
    rec['pack_unpack_share_of_packed'] = round(rec['pack_unpack']['median_ms'] / rec['packed']['median_ms'], 4)
    rec['nv16_over_recipe'] = round(rec['nv16']['median_ms'] / rec['recipe']['median_ms'], 4)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--shapes', default='1080p,4k,4k_to_1080p')
    ap.add_argument('--out', default=None, help='append the JSON lines to this file as well')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('time_nv16_crop.py needs a GPU: nothing is measured without one')
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
