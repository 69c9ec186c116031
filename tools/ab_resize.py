"""Interleaved A/B of builds of libmeshflow_hip.so on one crop + resize call (default: cfg2 frames, the cfg2 crop rectangle, u8c3, same size).

    python tools/ab_resize.py [--format u8c1] [--size 2560x1440] [--shape 64x2160x3840] [--rect 13,11,1909,1068] [--dev] base.so base_copy.so new.so

--size: mf_crop_resize_to_<format> to that output (without it mf_crop_resize_<format>); --dev: mf_crop_resize_dev_<format>, the rectangle read
from device memory.  Every library's output is compared with the first one's, byte for byte.  The same library under two file names gives
the A/A spread of the call."""
import argparse, ctypes, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from meshflow_amd import synthetic
ap = argparse.ArgumentParser()
ap.add_argument('--format', default='u8c3', choices=['u8c3', 'u8c1', 'u16c3', 'u8c4'])
ap.add_argument('--size', default=None, help='output WxH')
ap.add_argument('--shape', default='300x1080x1920', help='frames FxHxW')
ap.add_argument('--rect', default='13,11,1909,1068', help='left,top,right,bottom (inclusive)')
ap.add_argument('--dev', action='store_true')
ap.add_argument('--reps', type=int, default=5)
ap.add_argument('libs', nargs='+')
args = ap.parse_args()
F, H, W = (int(v) for v in args.shape.split('x'))
oW, oH = (int(v) for v in args.size.split('x')) if args.size else (W, H)
rect = tuple(int(v) for v in args.rect.split(','))
dev = torch.device('cuda:0')
frames = synthetic.frames_torch(F, H, W, dev, seed=0)
if args.format == 'u8c1':
    frames = frames[..., 1].contiguous()
elif args.format == 'u8c4':
    frames = torch.cat([frames, frames[..., :1]], dim=-1).contiguous()
elif args.format == 'u16c3':
    frames = (frames.to(torch.int32) * 257).to(torch.uint16)
bounds = torch.tensor(rect, dtype=torch.int32, device=dev)
status = torch.zeros(1, dtype=torch.int32, device=dev)
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
P, I = ctypes.c_void_p, ctypes.c_int
libs = []
for p in args.libs:
    lib = ctypes.CDLL(os.path.abspath(p))
    lib.mf_crop_resize_workspace_bytes.restype = ctypes.c_size_t
    lib.mf_crop_resize_workspace_bytes.argtypes = [I] * 2
    getattr(lib, 'mf_crop_resize_' + args.format).argtypes = [P, P] + [I] * 7 + [P, P]
    getattr(lib, 'mf_crop_resize_to_' + args.format).argtypes = [P, P] + [I] * 9 + [P, P]
    getattr(lib, 'mf_crop_resize_dev_' + args.format).argtypes = [P, P, I, I, I, P, I, I, P, P, P]
    libs.append(dict(name=os.path.basename(p), lib=lib, out=torch.empty((F, oH, oW) + tuple(frames.shape[3:]), dtype=frames.dtype, device=dev),
                     work=torch.empty(lib.mf_crop_resize_workspace_bytes(oW, oH), dtype=torch.uint8, device=dev), t=[]))
def run(v):
    a = (frames.data_ptr(), v['out'].data_ptr(), F, W, H)
    if args.dev:
        rc = getattr(v['lib'], 'mf_crop_resize_dev_' + args.format)(*a, bounds.data_ptr(), oW, oH, v['work'].data_ptr(), status.data_ptr(), st)
    elif args.size:
        rc = getattr(v['lib'], 'mf_crop_resize_to_' + args.format)(*a, *rect, oW, oH, v['work'].data_ptr(), st)
    else:
        rc = getattr(v['lib'], 'mf_crop_resize_' + args.format)(*a, *rect, v['work'].data_ptr(), st)
    assert rc == 0
for v in libs:
    for _ in range(30): run(v)              # (launches 3-20 after a fresh allocation run slow: bench.py's warm-up for this row)
torch.cuda.synchronize()
assert int(status.item()) == 0
print(f'{args.format} {F}x{H}x{W} rect {rect} -> {oW}x{oH}' + (' (device rectangle)' if args.dev else ''))
for v in libs[1:]:
    print(v['name'], 'identical to', libs[0]['name'], ':', torch.equal(v['out'].view(torch.uint8), libs[0]['out'].view(torch.uint8)))
for _ in range(args.reps):
    for v in libs:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10): run(v)
        e1.record(); torch.cuda.synchronize()
        v['t'].append(e0.elapsed_time(e1) / 10)
moved = (F * H * W + F * oH * oW) * frames[0, 0, 0].numel() * frames.element_size()        # bytes of a full-frame crop: read once, written once
for v in libs:
    t = np.array(v['t'])
    print(f'{v["name"]:28s} resize median {np.median(t):.4f} ms min {t.min():.4f} max {t.max():.4f}  (frac of 8 TB/s {moved / (np.median(t) * 1e-3) / 8e12:.4f})')
