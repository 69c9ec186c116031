"""Where the device tracker's time goes at cfg2 (300 x 1080p, 4 x 4 sub-frames): the two device calls (`ops.fast_corners` = fast_detect_kernel +
fast_compact_kernel; `ops.lk_track` = pyr_down_kernel x 3 + lk_level_kernel x 4) by HIP events, the copy of their outputs to the host, and the
host finisher (`tracker.finish_pair`: RANSAC per sub-frame + one DLT per pair) by the wall clock.  With --outliers device the outlier step
runs on the device too (`ops.ransac_inliers` + `ops.gather_inliers` = ransac_subframe_kernel + track_gather_kernel, by HIP events), only the
packed survivors are copied, the host finisher is the DLT per pair alone (`tracker.finish_packed`), and the line also carries the
distribution of the iterations run per sub-frame.  `host_fit_ms` is the DLT per pair by itself (in the host mode: run once more after
`finish_pair`), so `host_ms - host_fit_ms` is the host RANSAC.  With --fit device (needs --outliers device) the fit per pair runs on the
device as well (`ops.fit_homographies` = hfit_sums_kernel + hfit_solve_kernel): `fit_ms` by HIP events, `copy_ms` is the copy of the
matrices and their records alone, `host_ms` and `host_fit_ms` stay 0, and the line carries the fit's statuses and sweeps.  `tracker_fps` is
frames over the sum of all timed stages.  Per-kernel times: run this under
`rocprofv3 --kernel-trace --stats -- python tools/time_tracker.py --repeats 1`.  One JSON line.
    python tools/time_tracker.py [--frames 300] [--height 1080] [--width 1920] [--chunk-pairs 32] [--max-per-subframe 1024] [--repeats 3]
                                 [--outliers {host,device}] [--fit {host,device}]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=300)
    ap.add_argument('--height', type=int, default=1080)
    ap.add_argument('--width', type=int, default=1920)
    ap.add_argument('--sub', type=int, default=4)
    ap.add_argument('--chunk-pairs', type=int, default=32)
    ap.add_argument('--max-per-subframe', type=int, default=1024)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--kind', default='pattern')
    ap.add_argument('--outliers', choices=('host', 'device'), default='host')
    ap.add_argument('--fit', choices=('host', 'device'), default='host')
    a = ap.parse_args()
    if a.fit == 'device' and a.outliers != 'device':
        ap.error('--fit device needs --outliers device')
    import numpy as np
    import torch
    from meshflow_amd import host, ops, synthetic, tracker
    dev = torch.device('cuda:0')
    # the green channel of synthetic.clip's frames, made on the device chunk by chunk (the BGR clip itself is 1.9 GB)
    grey = torch.cat([synthetic.frames_torch(min(50, a.frames - lo), a.height, a.width, dev, seed=1, kind=a.kind, first_frame=lo)[..., 1].contiguous()
                      for lo in range(0, a.frames, 50)])
    grid = ops.track_subframe_grid(a.width, a.height, a.sub, a.sub)
    best = None
    timed = ('fast_ms', 'lk_ms', 'ransac_gather_ms', 'fit_ms', 'copy_ms', 'host_ms')
    for _ in range(a.repeats):
        t = dict.fromkeys(timed + ('host_fit_ms',), 0.0)
        corners = found_total = tracked = survivors = 0
        overflow = 0
        infos, fit_infos = [], []
        for lo in range(0, a.frames - 1, a.chunk_pairs):
            e, l = grey[lo:lo + a.chunk_pairs][:a.frames - 1 - lo], grey[lo + 1:lo + 1 + a.chunk_pairs]
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
            ev[0].record()
            points, counts, status = ops.fast_corners(e, a.sub, a.sub, a.max_per_subframe)
            ev[1].record()
            moved, found = ops.lk_track(e, l, points, counts, a.sub, a.sub)
            ev[2].record()
            if a.outliers == 'device':
                inlier, info = ops.ransac_inliers(points, counts, moved, found, 4)
                early, late, offsets, _ = ops.gather_inliers(points, moved, inlier, info, a.width, a.height, a.sub, a.sub, 4)
            ev[3].record()
            if a.fit == 'device':
                d_hom, d_fit_info, _ = ops.fit_homographies(early, late, offsets)
            ev[4].record()
            torch.cuda.synchronize()
            t['fast_ms'] += ev[0].elapsed_time(ev[1])
            t['lk_ms'] += ev[1].elapsed_time(ev[2])
            t['ransac_gather_ms'] += ev[2].elapsed_time(ev[3])
            t['fit_ms'] += ev[3].elapsed_time(ev[4])
            w0 = time.perf_counter()
            if a.fit == 'device':
                h_hom, h_fit_info = d_hom.cpu().numpy(), d_fit_info.cpu().numpy()
                t['copy_ms'] += (time.perf_counter() - w0) * 1e3
                infos.append(info.cpu().numpy().reshape(-1, 4))
                fit_infos.append(h_fit_info)
                corners += int(counts.sum().item())
                overflow += int((status != 0).sum().item())
                found_total += int(found.sum().item())
                survivors += int(early.shape[0])
                tracked += int((h_fit_info[:, 0] == 0).sum())
                continue
            if a.outliers == 'device':
                early, late, offsets = (x.cpu().numpy() for x in (early, late, offsets))
                w1 = time.perf_counter()
                results = [tracker.finish_packed(early[lo_:hi_], late[lo_:hi_]) for lo_, hi_ in zip(offsets[:-1], offsets[1:])]
                w2 = time.perf_counter()
                t['copy_ms'] += (w1 - w0) * 1e3
                t['host_ms'] += (w2 - w1) * 1e3
                t['host_fit_ms'] += (w2 - w1) * 1e3
                infos.append(info.cpu().numpy().reshape(-1, 4))
                corners += int(counts.sum().item())
                overflow += int((status != 0).sum().item())
                found_total += int(found.sum().item())
                survivors += int(offsets[-1])
                tracked += sum(h is not None for _, _, h in results)
                continue
            points, counts, status, moved, found = (x.cpu().numpy() for x in (points, counts, status, moved, found))
            w1 = time.perf_counter()
            results = [tracker.finish_pair(grid, points[i], counts[i], moved[i], found[i], 4) for i in range(len(points))]
            w2 = time.perf_counter()
            for e_, l_, h_ in results:                 # the DLT of every pair once more, by itself: host_ms - host_fit_ms = the host RANSAC
                if h_ is not None:
                    host.lsq_homography(e_, l_)
            w3 = time.perf_counter()
            t['copy_ms'] += (w1 - w0) * 1e3
            t['host_ms'] += (w2 - w1) * 1e3
            t['host_fit_ms'] += (w3 - w2) * 1e3
            corners += int(counts.sum())
            overflow += int((status != 0).sum())
            found_total += int(found.sum())
            survivors += sum(len(e) for e, _, h in results if h is not None)
            tracked += sum(h is not None for _, _, h in results)
        t.update(corners=corners, found=found_total, survivors=survivors, pairs_with_homography=tracked, subframes_over_the_cap=overflow)
        if infos:
            info = np.concatenate(infos)
            ran = info[:, 3]
            t.update(subframes=len(info), subframes_by_status=np.bincount(info[:, 0], minlength=3).tolist(),
                     iterations_run=dict(min=int(ran.min()), median=float(np.median(ran)), p90=float(np.percentile(ran, 90)),
                                         p99=float(np.percentile(ran, 99)), max=int(ran.max()), total=int(ran.sum())))
        if fit_infos:
            fit_info = np.concatenate(fit_infos)
            t.update(fit_by_status=np.bincount(fit_info[:, 0], minlength=5).tolist(), fit_sweeps_max=int(fit_info[:, 2].max()),
                     fit_points_max=int(fit_info[:, 1].max()))
        t['tracker_fps'] = a.frames / (sum(t[k] for k in timed) * 1e-3)
        if best is None or sum(t[k] for k in timed) < sum(best[k] for k in timed):
            best = t
    best.update(frames=a.frames, width=a.width, height=a.height, sub=a.sub, chunk_pairs=a.chunk_pairs, max_per_subframe=a.max_per_subframe,
                kind=a.kind, repeats=a.repeats, outliers=a.outliers, fit=a.fit)
    print(json.dumps(best))


if __name__ == '__main__':
    main()
