"""The tracker on the device: `frontend_cv2.Tracker`'s interface (mfs.py:455-629) without OpenCV.

FAST corners and pyramidal LK of every sub-frame run as HIP kernels (`ops.fast_corners`, `ops.lk_track`, csrc/track_*.hip; bit for bit
tests/track_model.py).  The outlier step per sub-frame and the homography over the survivors are a few thousand points per pair and run
on the host in NumPy (`host.ransac_inliers`, `host.lsq_homography`) -- deterministic stand-ins for cv2.findHomography, NOT restatements of
it (host.py says why).  With outliers='device' the outlier step and the packing of the survivors run as HIP kernels too
(`ops.ransac_inliers`, `ops.gather_inliers`, csrc/track_ransac.hip; bit for bit tests/ransac_model.py, a specification of its own and not
`host.ransac_inliers`), and only the packed survivors come down for the one homography fit per pair.  With fit='device' (which needs
outliers='device') that fit runs as HIP kernels as well (`ops.fit_homographies`, csrc/track_fit.hip; bit for bit
tests/homography_model.py, again a specification of its own: `host.lsq_homography` stays the specification of fit='host', and the two agree
to rounding, tests/test_homography_model.py) and no feature leaves the device: `DeviceTracker.track_clip_resident`.
Input is one-channel uint8 only: grey frames or the luma plane of an NV12 clip.  A BGR clip needs a luma plane first, e.g.
`(bgr.float() @ torch.tensor([0.114, 0.587, 0.299], device=bgr.device)).round().clamp(0, 255).to(torch.uint8)` (cv2's BGR2GRAY up to
its 14-bit fixed point); the reference itself hands BGR sub-frames to cv2, where FAST sees BGR2GRAY and LK tracks three channels."""
import numpy as np

from . import host


def finish_pair(grid, points, counts, moved, found, min_features):
    """mfs.py:510-528 and 564-629 after the two cv2 calls, for ONE frame pair: `grid` = ops.track_subframe_grid(...), points / moved
    (S, max, 2) float32, counts (S,), found (S, max) as NumPy arrays.  Returns (early, late, homography) -- (K, 1, 2) float64 features in
    frame coordinates -- or (None, None, None)."""
    sub_w, sub_h, _, rows = grid
    early_parts, late_parts = [], []
    for s in range(points.shape[0]):
        k = min(int(counts[s]), points.shape[1])
        if k < min_features:                                             # mfs.py:614
            continue
        keep = found[s, :k].astype(bool)
        early, late = points[s, :k][keep], moved[s, :k][keep]
        if len(early) < min_features:                                    # mfs.py:626
            continue
        try:
            inliers = host.ransac_inliers(early, late)
        except ValueError:                                               # fewer than 4 pairs, collinear points, no consensus: cv2 returns no mask
            continue
        offset = [(s // rows) * sub_w, (s % rows) * sub_h]
        # adding the (int, int) offset promotes the float32 coordinates to float64, as in mfs.py:578
        early_parts.append(early[inliers][:, np.newaxis, :] + offset)
        late_parts.append(late[inliers][:, np.newaxis, :] + offset)
    if not early_parts:        # the reference dies in np.concatenate here; like frontend_cv2.Tracker we report the pair as untrackable
        return None, None, None
    early, late = np.concatenate(early_parts), np.concatenate(late_parts)
    if len(early) < min_features:                                        # mfs.py:521
        return None, None, None
    try:
        homography = host.lsq_homography(early, late)
    except ValueError:
        return None, None, None
    return early, late, homography


OUTLIER_MODES = ('host', 'device')


def check_outliers(outliers):
    if outliers not in OUTLIER_MODES:
        raise ValueError(f"outliers must be 'host' or 'device', got {outliers!r}")
    return outliers


FIT_MODES = ('host', 'device')


def check_fit(fit, outliers):
    if fit not in FIT_MODES:
        raise ValueError(f"fit must be 'host' or 'device', got {fit!r}")
    if fit == 'device' and outliers != 'device':
        raise ValueError(f"fit='device' needs outliers='device' (got outliers={outliers!r}): the device fit reads the survivors the device "
                         f"outlier step packs")
    return fit


def finish_packed(early, late):
    """mfs.py:521-528 for ONE pair's packed survivors of the device outlier step ((K, 2) float64, empty where the pair fell below the
    minimum): (early, late, homography) as `finish_pair` returns them, or (None, None, None)."""
    if len(early) == 0:
        return None, None, None
    early, late = early[:, np.newaxis, :], late[:, np.newaxis, :]
    try:
        homography = host.lsq_homography(early, late)
    except ValueError:
        return None, None, None
    return early, late, homography


class DeviceTracker:
    """FAST + LK on the device and the homography on the host, with the stabilizer's sub-frame grid and minimum feature count; the RANSAC
    outlier step on the host (outliers='host': `host.ransac_inliers`) or on the device (outliers='device': `ops.ransac_inliers`, its own
    specification -- the two modes agree on clean tracks and may differ by points near the threshold).  fit='device' (with
    outliers='device' only): the homography on the device too (`ops.fit_homographies`, its own specification; the two fits agree to
    rounding) -- `track_clip_resident`; the other methods and fit='host' are the host fit's."""

    def __init__(self, subframe_rows, subframe_cols, min_features, device='cuda:0', max_per_subframe=1024, threshold=10, outliers='host',
                 fit='host'):
        self.outliers = check_outliers(outliers)
        self.fit = check_fit(fit, self.outliers)
        self.subframe_rows = int(subframe_rows)
        self.subframe_cols = int(subframe_cols)
        self.min_features = min_features
        self.device = device
        self.max_per_subframe = int(max_per_subframe)
        self.threshold = int(threshold)

    def _device_stack(self, frames, name):
        import torch
        if not isinstance(frames, torch.Tensor):
            frames = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(f) for f in frames])))
        if frames.dtype != torch.uint8 or frames.dim() != 3:
            raise ValueError(f'{name} must be one-channel uint8 frames (n, H, W), got {frames.dtype} {tuple(frames.shape)}: the device tracker '
                             f'takes grey or luma only')
        return frames.to(self.device).contiguous()

    def track_stacks(self, d_early, d_late, chunk_pairs=32):
        """[(early, late, homography) or (None, None, None)] for the pairs (d_early[i], d_late[i]) of two (n, H, W) uint8 device stacks,
        `chunk_pairs` pairs per launch so that outputs and workspace stay bounded."""
        from . import ops
        if self.outliers == 'device':
            return self.track_stacks_packed(d_early, d_late, chunk_pairs)[0]
        if d_early.shape != d_late.shape:
            raise ValueError('early and late stacks must have the same shape')
        n, H, W = d_early.shape
        grid = ops.track_subframe_grid(W, H, self.subframe_rows, self.subframe_cols)
        chunk_pairs = max(1, min(int(chunk_pairs), 65535 // (2 * grid[2] * grid[3])))
        out = []
        for lo in range(0, n, chunk_pairs):
            e, l = d_early[lo:lo + chunk_pairs], d_late[lo:lo + chunk_pairs]
            points, counts, _ = ops.fast_corners(e, self.subframe_rows, self.subframe_cols, self.max_per_subframe, self.threshold)
            moved, found = ops.lk_track(e, l, points, counts, self.subframe_rows, self.subframe_cols)
            points, counts, moved, found = (t.cpu().numpy() for t in (points, counts, moved, found))
            out.extend(finish_pair(grid, points[i], counts[i], moved[i], found[i], self.min_features) for i in range(len(points)))
        return out

    def track_stacks_packed(self, d_early, d_late, chunk_pairs=32):
        """outliers='device': `track_stacks`' list and the same features as they stay on the device -- (early (K_total, 2) float64, late,
        offsets (n + 1,) int32 device tensors, the largest range), what `ops.vertex_motion` takes.  Per chunk FAST -> LK -> RANSAC -> gather on
        the device, then one copy of the chunk's packed survivors and offsets to the host for `host.lsq_homography` per pair.  (A pair whose
        fit fails keeps its range in the packed features; its entry in the list is the None triple.)  Unlike the host mode, which takes any
        `min_features`, this one needs min_features >= 1: the C calls refuse less."""
        import torch
        from . import ops
        if d_early.shape != d_late.shape:
            raise ValueError('early and late stacks must have the same shape')
        n, H, W = d_early.shape
        grid = ops.track_subframe_grid(W, H, self.subframe_rows, self.subframe_cols)
        chunk_pairs = max(1, min(int(chunk_pairs), 65535 // (2 * grid[2] * grid[3])))
        dev = d_early.device
        out, earlies, lates, total = [], [torch.empty((0, 2), dtype=torch.float64, device=dev)], [torch.empty((0, 2), dtype=torch.float64, device=dev)], 0
        ranges = [torch.zeros(1, dtype=torch.int32, device=dev)]
        for lo in range(0, n, chunk_pairs):
            e, l = d_early[lo:lo + chunk_pairs], d_late[lo:lo + chunk_pairs]
            points, counts, _ = ops.fast_corners(e, self.subframe_rows, self.subframe_cols, self.max_per_subframe, self.threshold)
            moved, found = ops.lk_track(e, l, points, counts, self.subframe_rows, self.subframe_cols)
            inlier, info = ops.ransac_inliers(points, counts, moved, found, self.min_features)
            early, late, offsets, _ = ops.gather_inliers(points, moved, inlier, info, W, H, self.subframe_rows, self.subframe_cols,
                                                         self.min_features)
            h_early, h_late, h_offsets = early.cpu().numpy(), late.cpu().numpy(), offsets.cpu().numpy()
            for a, b in zip(h_offsets[:-1], h_offsets[1:]):
                out.append(finish_packed(h_early[a:b], h_late[a:b]))
            earlies.append(early)
            lates.append(late)
            ranges.append(offsets[1:] + total)
            total += int(h_offsets[-1])
        offsets = torch.cat(ranges)
        kmax = int((offsets[1:] - offsets[:-1]).max().item()) if n else 0
        return out, (torch.cat(earlies), torch.cat(lates), offsets, kmax)

    def track_clip_packed(self, d_grey, chunk_pairs=32):
        """`track_stacks_packed` over the adjacent pairs of a resident clip."""
        d_grey = self._device_stack(d_grey, 'd_grey')
        if d_grey.shape[0] < 2:
            raise ValueError('a clip needs at least 2 frames')
        return self.track_stacks_packed(d_grey[:-1], d_grey[1:], chunk_pairs)

    def track_stacks_resident(self, d_early, d_late, chunk_pairs=32):
        """fit='device': per chunk FAST -> LK -> RANSAC -> gather -> fit on the device and nothing else: (early (K_total, 2) float64, late,
        offsets (n + 1,) int32, the largest range, homographies (n, 3, 3) float64, info (n, 4) int32 -- `ops.fit_homographies`' record; a pair
        that is not _lib.HFIT_OK holds the identity --) as device tensors.  No feature visits the host: the only host traffic is the
        survivor total `ops.gather_inliers` reads per chunk, and the largest range at the end.  Nobody has looked at `info` yet:
        `ops.fit_check` does."""
        import torch
        from . import ops
        if self.fit != 'device':
            raise ValueError("track_stacks_resident needs a tracker made with fit='device'")
        if d_early.shape != d_late.shape:
            raise ValueError('early and late stacks must have the same shape')
        n, H, W = d_early.shape
        grid = ops.track_subframe_grid(W, H, self.subframe_rows, self.subframe_cols)
        chunk_pairs = max(1, min(int(chunk_pairs), 65535 // (2 * grid[2] * grid[3])))
        dev = d_early.device
        earlies, lates = [torch.empty((0, 2), dtype=torch.float64, device=dev)], [torch.empty((0, 2), dtype=torch.float64, device=dev)]
        ranges, total = [torch.zeros(1, dtype=torch.int32, device=dev)], 0
        homographies, infos = [torch.empty((0, 3, 3), dtype=torch.float64, device=dev)], [torch.empty((0, 4), dtype=torch.int32, device=dev)]
        for lo in range(0, n, chunk_pairs):
            e, l = d_early[lo:lo + chunk_pairs], d_late[lo:lo + chunk_pairs]
            points, counts, _ = ops.fast_corners(e, self.subframe_rows, self.subframe_cols, self.max_per_subframe, self.threshold)
            moved, found = ops.lk_track(e, l, points, counts, self.subframe_rows, self.subframe_cols)
            inlier, info = ops.ransac_inliers(points, counts, moved, found, self.min_features)
            early, late, offsets, _ = ops.gather_inliers(points, moved, inlier, info, W, H, self.subframe_rows, self.subframe_cols,
                                                         self.min_features)
            h, fit_info, _ = ops.fit_homographies(early, late, offsets)
            earlies.append(early)
            lates.append(late)
            ranges.append(offsets[1:] + total)
            total += early.shape[0]
            homographies.append(h)
            infos.append(fit_info)
        offsets = torch.cat(ranges)
        kmax = int((offsets[1:] - offsets[:-1]).max().item()) if n else 0
        return torch.cat(earlies), torch.cat(lates), offsets, kmax, torch.cat(homographies), torch.cat(infos)

    def track_clip_resident(self, d_grey, chunk_pairs=32):
        """`track_stacks_resident` over the adjacent pairs of a resident clip: (d_early, d_late, d_offsets, kmax, d_homographies, d_info)."""
        d_grey = self._device_stack(d_grey, 'd_grey')
        if d_grey.shape[0] < 2:
            raise ValueError('a clip needs at least 2 frames')
        return self.track_stacks_resident(d_grey[:-1], d_grey[1:], chunk_pairs)

    def track_clip(self, d_grey, chunk_pairs=32):
        """The adjacent pairs (t, t + 1) of a resident (F, H, W) uint8 clip: F - 1 results."""
        d_grey = self._device_stack(d_grey, 'd_grey')
        if d_grey.shape[0] < 2:
            raise ValueError('a clip needs at least 2 frames')
        return self.track_stacks(d_grey[:-1], d_grey[1:], chunk_pairs)

    def track_pair(self, early_frame, late_frame):
        """(early_features, late_features, homography) of one frame pair, or (None, None, None) -- mfs.py:492-528."""
        return self.track_pairs([early_frame], [late_frame])[0]

    def track_pairs(self, first_frames, second_frames, workers=None, chunk_pairs=32):
        """track_pair over many independent pairs, in order (`workers` is accepted for frontend_cv2.Tracker's signature and unused)."""
        return self.track_stacks(self._device_stack(first_frames, 'first_frames'), self._device_stack(second_frames, 'second_frames'),
                                 chunk_pairs)
