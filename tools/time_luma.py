"""What `ops.luma` costs: the kernel for each of its four sources (BGR and BGRA uint8, BGR uint16, a 16-bit luma plane) at cfg2's 300 x 1080p
and at a 150 x 4K shard, by HIP events, interleaved with the same bytes computed by a torch expression on the same tensors (there is no
earlier kernel to compare with); the two results are compared with torch.equal first.  Per source and size: the median and the best of
--repeats after --warmup passes of each, the bytes the conversion has to move (source + destination) over the kernel's median time, and
that rate as a fraction of the 8 TB/s peak.  With --motion, also what share of `estimate_motion(outliers='device', fit='device')` the luma
step is on a synthetic cfg2-sized BGR clip: the wall clock around the synchronised call on the BGR clip and on its luma.  One JSON line per
source and size, one for the share.
    python tools/time_luma.py [--sizes 300x1080x1920,150x2160x3840] [--repeats 20] [--warmup 3] [--motion]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_BYTES_PER_S = 8.0e12
# name -> (channels; 0 = a plane without a channel axis, bytes per sample)
SOURCES = {'u8c3': (3, 1), 'u8c4': (4, 1), 'u16c3': (3, 2), 'u16c1': (0, 2)}


def torch_luma(frames):
    """tests/luma_model.py in torch: int32 holds every sum."""
    import torch
    if frames.dim() == 3:
        return (frames.to(torch.int32) >> 8).to(torch.uint8)
    b, g, r = (frames[..., i].to(torch.int32) for i in range(3))
    if frames.dtype == torch.uint8:
        return ((b * 3735 + g * 19235 + r * 9798 + 16384) >> 15).to(torch.uint8)
    return ((b * 1868 + g * 9617 + r * 4899 + 8192) >> 22).to(torch.uint8)


def random_frames(name, n, h, w, dev):
    import torch
    channels, sample = SOURCES[name]
    shape = (n, h, w) + ((channels,) if channels else ())
    count = n * h * w * max(channels, 1) * sample
    raw = torch.empty(count, dtype=torch.uint8, device=dev)
    step = 1 << 28
    for lo in range(0, count, step):                                    # (randint's int64 intermediate stays small)
        raw[lo:lo + step] = torch.randint(0, 256, (min(step, count - lo),), dtype=torch.uint8, device=dev)
    return (raw.view(torch.uint16) if sample == 2 else raw).view(shape)


def timed(fn, repeats):
    import torch
    out = []
    for _ in range(repeats):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        ev[1].synchronize()
        out.append(ev[0].elapsed_time(ev[1]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='300x1080x1920,150x2160x3840')
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--motion', action='store_true')
    a = ap.parse_args()
    import statistics
    import torch
    from meshflow_amd import ops
    dev = torch.device('cuda:0')
    for size in a.sizes.split(','):
        n, h, w = (int(v) for v in size.split('x'))
        for name, (channels, sample) in SOURCES.items():
            frames = random_frames(name, n, h, w, dev)
            out = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
            ops.luma(frames, out=out)
            equal = bool(torch.equal(out, torch_luma(frames)))
            kernel, composed = [], []
            for k in range(a.warmup + a.repeats):                       # interleaved: one of each per pass
                one = timed(lambda: ops.luma(frames, out=out), 1) + timed(lambda: torch_luma(frames), 1)
                if k >= a.warmup:
                    kernel.append(one[0])
                    composed.append(one[1])
            moved = n * h * w * (max(channels, 1) * sample + 1)
            med = statistics.median(kernel)
            print(json.dumps(dict(source=name, frames=n, height=h, width=w, equals_torch=equal, kernel_ms_median=med, kernel_ms_best=min(kernel),
                                  kernel_ms_worst=max(kernel), torch_ms_median=statistics.median(composed), torch_ms_best=min(composed),
                                  bytes_moved=moved, tb_per_s=moved / (med * 1e-3) / 1e12, of_peak=moved / (med * 1e-3) / PEAK_BYTES_PER_S,
                                  repeats=a.repeats, warmup=a.warmup)), flush=True)
            del frames, out
            torch.cuda.empty_cache()
    if a.motion:
        from meshflow_amd import synthetic
        from meshflow_amd.stabilizer import MeshFlowStabilizer
        n, h, w = 300, 1080, 1920
        bgr = torch.cat([synthetic.frames_torch(min(50, n - lo), h, w, dev, seed=1, kind='pattern', first_frame=lo) for lo in range(0, n, 50)])
        s = MeshFlowStabilizer(device='cuda:0')
        grey = ops.luma(bgr)
        line = dict(what='estimate_motion', frames=n, height=h, width=w)
        try:
            for key, clip in (('bgr_ms', bgr), ('luma_ms', grey)):
                best = None
                for k in range(3):                                      # (the first pass warms up and is dropped)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    s.estimate_motion(clip, outliers='device', fit='device')
                    torch.cuda.synchronize()
                    ms = (time.perf_counter() - t0) * 1e3
                    best = ms if k and (best is None or ms < best) else best
                line[key] = best
            line['luma_kernel_ms'] = statistics.median(timed(lambda: ops.luma(bgr, out=grey), 5))
            line['luma_share_of_bgr'] = line['luma_kernel_ms'] / line['bgr_ms']
        except ValueError as e:                                         # (a synthetic pair the tracker refuses: say so, do not hide it)
            line['error'] = str(e)
        print(json.dumps(line), flush=True)


if __name__ == '__main__':
    main()
