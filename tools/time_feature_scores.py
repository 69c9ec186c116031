"""What the feature scores cost beside the tracker, at tools/time_tracker.py's 61-frame 1080p shape: `track_clip_resident` over the adjacent
pairs of a resident grey clip (the tracker's own pass, F - 1 pairs), against the scored pass -- `track_stacks_resident` over the F pairs
(clip[t], cropped[t]) followed by `ops.feature_scores` and the read of its record and scores, which is what
`MeshFlowStabilizer.cropping_and_distortion_resident` runs.  `cropped` is `ops.crop_resize` of the clip by a rectangle that scales it by
about 1.1 per axis.  Wall clock around a synchronised pass, the better of --repeats; `scores_kernel_ms` is `ops.feature_scores` alone by
HIP events.  One JSON line.
    python tools/time_feature_scores.py [--frames 61] [--height 1080] [--width 1920] [--chunk-pairs 32] [--max-per-subframe 128] [--repeats 3]
                                        [--inset-divisor 22]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=61)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--sub', type=int, default=4)
    ap.add_argument('--chunk-pairs', type=int, default=32)
    ap.add_argument('--max-per-subframe', type=int, default=128)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--kind', default='pattern')
    ap.add_argument('--inset-divisor', type=int, default=22, help='the crop leaves out width / this and height / this on every side (22: 1.1x)')
    a = ap.parse_args()
    import torch
    from meshflow_amd import ops, synthetic, tracker
    dev = torch.device('cuda:0')
    grey = torch.cat([synthetic.frames_torch(min(50, a.frames - lo), a.height, a.width, dev, seed=1, kind=a.kind, first_frame=lo)[..., 1].contiguous()
                      for lo in range(0, a.frames, 50)])
    mx, my = a.width // a.inset_divisor, a.height // a.inset_divisor
    rect = (mx, my, a.width - 1 - mx, a.height - 1 - my)
    cropped = ops.crop_resize(grey, rect)
    t = tracker.DeviceTracker(a.sub, a.sub, 4, dev, a.max_per_subframe, outliers='device', fit='device')
    best = {}

    def keep(key, ms):
        best[key] = min(best.get(key, ms), ms)

    for _ in range(a.repeats + 1):                                      # (the first pass warms up and is dropped)
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        own = t.track_clip_resident(grey, a.chunk_pairs)
        refused = ops.fit_check(own[5])
        torch.cuda.synchronize()
        w1 = time.perf_counter()
        tracked = t.track_stacks_resident(grey, cropped, a.chunk_pairs)
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        scores, per_pair, record = ops.feature_scores(tracked[4], tracked[5])
        ev[1].record()
        unscored = ops.feature_scores_check(record)
        values = scores.cpu().numpy().tolist()
        torch.cuda.synchronize()
        w2 = time.perf_counter()
        if _:
            keep('tracker_ms', (w1 - w0) * 1e3)
            keep('scored_pass_ms', (w2 - w1) * 1e3)
            keep('scores_kernel_ms', ev[0].elapsed_time(ev[1]))
    # where the scored pass spends its time: the tracker's stages on the pairs (clip[t], cropped[t]) by HIP events, as tools/time_tracker.py
    # brackets them on adjacent frames (summed over the chunks, once, after the passes above)
    stages = dict.fromkeys(('scored_fast_ms', 'scored_lk_ms', 'scored_ransac_gather_ms', 'scored_fit_ms'), 0.0)
    iterations = []
    for lo in range(0, a.frames, a.chunk_pairs):
        e, l = grey[lo:lo + a.chunk_pairs], cropped[lo:lo + a.chunk_pairs]
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        ev[0].record()
        points, counts, _ = ops.fast_corners(e, a.sub, a.sub, a.max_per_subframe)
        ev[1].record()
        moved, found = ops.lk_track(e, l, points, counts, a.sub, a.sub)
        ev[2].record()
        inlier, info = ops.ransac_inliers(points, counts, moved, found, 4)
        early, late, offsets, _ = ops.gather_inliers(points, moved, inlier, info, a.width, a.height, a.sub, a.sub, 4)
        ev[3].record()
        ops.fit_homographies(early, late, offsets)
        ev[4].record()
        torch.cuda.synchronize()
        for i, key in enumerate(stages):
            stages[key] += ev[i].elapsed_time(ev[i + 1])
        iterations.append(info.cpu().numpy().reshape(-1, 4)[:, 3])
    import numpy as np
    ran = np.concatenate(iterations)
    best.update(stages, scored_ransac_iterations=dict(median=float(np.median(ran)), p90=float(np.percentile(ran, 90)), max=int(ran.max()),
                                                      total=int(ran.sum())))
    geometric = (rect[2] - rect[0] + 1) * (rect[3] - rect[1] + 1) / (a.width * a.height)
    best.update(tracker_pairs=a.frames - 1, tracker_first_refused=refused, scored_pairs=int(record[0].item()), first_unscored=unscored,
                cropping_ratio=values[0], distortion_score=values[1], rect=rect, geometric_ratio=geometric, frames=a.frames, width=a.width,
                height=a.height, sub=a.sub, chunk_pairs=a.chunk_pairs, max_per_subframe=a.max_per_subframe, kind=a.kind, repeats=a.repeats)
    print(json.dumps(best))


if __name__ == '__main__':
    main()
