"""Online stabilization: frames pushed in as they arrive, every frame out again at once (`MeshFlowStabilizer.online_session`).

The offline path needs a whole clip twice: `ops.jacobi` smooths every vertex path over all its frames, and the crop rectangle is a clip-level
reduction.  A session replaces the first by `ops.online_smooth` -- a sliding window that ends at the newest frame (include/meshflow_hip.h,
mf_online_smooth_f64; tests/online_model.py) -- and the second by a rectangle fixed in advance from `crop_margin`.  Everything else is the
offline path's own: `ops.luma`, the device tracker with the outlier step and the fit on the device, `ops.vertex_motion`, `ops.cell_table`,
the format's warp and crop-resize (`ClipForm`).  What a session carries between pushes is listed once, in `_CARRIED`: the previous push's
last luma frame, an `ops.OnlineState`, -- with on_cut='reset' -- that frame's scene-cut signature (`ops.find_cuts`; tests/cuts_model.py), by
which a push finds the cuts in its frames and restarts the path at each, and -- with on_uncovered='limit' -- the last frame's step of
`ops.path_limit` (tests/path_limit_model.py), which scales a frame's correction back until the warped mesh covers the fixed rectangle again.

lag=k >= 1 trades k frames of latency for a smoother path (profiles/online_lag.md): the smoother is `ops.online_smooth_lag`
(mf_online_smooth_lag_f64; tests/online_lag_model.py), which hands a frame out as it stands in the window that ends k frames after it, so a
push returns the frames that have become final, [emitted, seen - k), and the session also carries the pixels of the at most k frames it still
owes, as clones on the device (`hold_frames`).  `flush()` hands those out when the stream -- or, with on_cut='reset', a shot -- ends.

Many live streams of one size go through an `OnlineGroup` (`MeshFlowStabilizer.online_group`; profiles/online_group.md): one new frame of each
of any subset of them per push, in one set of launches, with the bytes of a session per stream; an `OnlineLagGroup` gives each `lag` frames
of look-ahead (profiles/online_group_lag.md).  What the three are told lives in an `OnlineSettings` each, and the stages they share exist
once, as functions of it: `track_pairs`, `warp_rows`, `empty_result`, `join_reports`."""
import collections
import math

import numpy as np

from . import host

# What `push` reports beside its frames.  first: the session's index of the first frame returned (the push's first frame unless the
# session has a lag); d_unstab, d_stab: (n, R+1, C+1, 2) float64 device tensors, n the frames returned, the unstabilized and the stabilized vertex paths; rectangle: the fixed crop (left, top, right, bottom), inclusive, in
# `ops.crop_resize`'s convention; covered: (n,) bool device tensor, True where the frame's own crop values (`CellTable.crop`, mfs.py:1075-1098)
# contain the rectangle -- False says the margin was too small for that frame and border colour shows --; lost: the session's indices of the
# frames whose pair (frame - 1 -> frame) could not be fitted.
OnlineReport = collections.namedtuple('OnlineReport', 'first d_unstab d_stab rectangle covered lost')


def margin_rectangle(crop_margin, W, H):
    """The fixed rectangle of a W x H frame: left = floor(m (W - 1)), right = (W - 1) - left, the same vertically; inclusive edges, any
    parity (`ops.crop_resize_nv12` and `ops.crop_resize_nv16` take the rectangle in luma pixels of any parity, so a pair needs no other)."""
    left, top = math.floor(crop_margin * (W - 1)), math.floor(crop_margin * (H - 1))
    right, bottom = (W - 1) - left, (H - 1) - top
    if right - left + 1 < 2 or bottom - top + 1 < 2:
        raise ValueError(f'crop_margin={crop_margin} leaves fewer than 2 x 2 pixels of a {W} x {H} frame')
    return left, top, right, bottom


class ClipForm(collections.namedtuple('ClipForm', 'fmt dtype shape')):
    """The form of a clip, whatever its length: fmt, the `ops._FormatYuv` row of a 4:2:0 or 4:2:2 pair (d_y, d_uv) or None for a stack (n, ...);
    the dtype; the shape of a frame -- of a luma plane for a pair.  Two clips of one form compare equal."""
    pair = property(lambda self: self.fmt is not None)

    def planes(self, clip):
        """The clip's plane stacks as a tuple: two for a pair, the stack itself otherwise; `clip(planes)` puts them back."""
        return tuple(clip) if self.pair else (clip,)

    def clip(self, planes):
        return tuple(planes) if self.pair else planes[0]

    def part(self, clip, lo, hi):
        return self.clip([p[lo:hi] for p in self.planes(clip)])

    def cat(self, clips):
        import torch
        return self.clip([torch.cat(planes) for planes in zip(*(self.planes(c) for c in clips))])

    def check_same(self, other, who):
        """ValueError unless `other`, the form of a later push to `who` -- 'session' or 'group' --, is this form, that of its first."""
        if other != self:
            raise ValueError(f'this {who} takes {self.dtype} frames of shape {self.shape}{" as (d_y, d_uv) pairs" if self.pair else ""}; '
                             f'got {other.dtype} frames of shape {other.shape}{" as a pair" if other.pair else ""}')

    def warp_crop(self, clip, table, border_bgr, crop):
        """The format's warp from `table` -- border_bgr for a stack, the format's red for a pair -- and, unless `crop` is None, its
        crop-resize to crop = (rectangle, output size or None)."""
        from . import ops
        if self.pair:
            out = ops._warp_yuv(self.fmt, *clip, table, ops.P010_BORDER_RED if self.fmt.border is ops._p010_border else ops.NV12_BORDER_RED, None, None)
            return out if crop is None else ops._crop_resize_yuv(self.fmt, out[0], out[1], crop[0], crop[1], None, None)
        out = ops.warp(clip, table, border_bgr)
        return out if crop is None else ops.crop_resize(out, crop[0], size=crop[1])

    def empty(self, w, h, device):
        """0 frames of this form at w x h."""
        import torch
        shapes = ((h, w), (h // 2 if self.fmt.half_rows else h, w // 2, 2)) if self.pair else ((h, w) + self.shape[2:],)
        return self.clip([torch.empty((0,) + shape, dtype=self.dtype, device=device) for shape in shapes])


def _is_422_pair(d_y, d_uv, dtype):
    """Whether a pair is a 4:2:2 clip of that dtype -- NV16 (uint8) or P210 (uint16): d_y (n, H, W) and d_uv (n, H, W/2, 2) -- chroma with
    luma's rows.  (A 4:2:0 pair has H/2 of them, and H >= 2, so no clip is both.)"""
    import torch
    if not (isinstance(d_y, torch.Tensor) and isinstance(d_uv, torch.Tensor) and d_y.dtype == d_uv.dtype == dtype):
        return False
    if d_y.dim() != 3 or d_uv.dim() != 4:
        return False
    n, H, W = (int(v) for v in d_y.shape)
    return W % 2 == 0 and H >= 1 and tuple(d_uv.shape) == (n, H, W // 2, 2)


def luma_of(frames, red_first=False):
    """(form, luma (n, H, W) uint8) of a clip in any form `stabilize_scored` takes; form: its `ClipForm`.  A pair's dtype tells NV12 / NV16
    (uint8) from P010 / P210 (uint16), and its d_uv's rows 4:2:2 (as many as luma's) from 4:2:0 (half); a uint16 luma plane goes through
    `ops.luma`."""
    import torch
    from . import ops
    if isinstance(frames, (tuple, list)):
        if len(frames) != 2:
            raise ValueError('an NV12 or P010 clip is the pair (d_y, d_uv)')
        d_y, d_uv = frames
        fmt = {torch.uint16: ops._P010}.get(getattr(d_y, 'dtype', None), ops._NV12)         # (whatever is neither fails NV12's checks)
        if fmt is ops._NV12 and _is_422_pair(d_y, d_uv, torch.uint8):
            fmt = ops._NV16
        elif fmt is ops._P010 and _is_422_pair(d_y, d_uv, torch.uint16):
            fmt = ops._P210
        ops._need_yuv(fmt, d_y, d_uv)
        return ClipForm(fmt, d_y.dtype, tuple(d_y.shape[1:])), (ops.luma(d_y) if fmt.dtype == torch.uint16 else d_y)
    if isinstance(frames, torch.Tensor) and frames.dtype == torch.uint16 and frames.dim() == 3:
        raise ValueError('a (n, H, W) uint16 stack is the luma plane of a P010 clip: pass the pair (d_y, d_uv)')
    ops._frames_format(frames)
    return ClipForm(None, frames.dtype, tuple(frames.shape[1:])), (ops.luma(frames, red_first) if ops.luma_source(frames) is not None else frames)


def hold_frames(held, planes, m):
    """The pixels of a lagged push: of the frames (held, then new) the oldest m are final and the rest are held.  held: a tuple of plane
    stacks or None; planes: the caller's new ones, as many; returns (final planes, new held planes or None: none).  With nothing held,
    `final` is the caller's planes or a view of them, no copy; what is held is a copy -- the caller's buffers are free --; every new frame is copied once,
    into the stack it is held in or the one it is handed out from, and a held frame at most once more; an old held stack is never written
    to.  Any torch tensors; no session is touched."""
    import torch
    n = int(planes[0].shape[0])
    if held is None:
        return (planes if m == n else tuple(f[:m] for f in planes)), (tuple(f[m:].clone() for f in planes) if m < n else None)
    h = int(held[0].shape[0])
    if m <= h:
        return tuple(x[:m] for x in held), tuple(torch.cat([x[m:], f]) if m < h else f.clone() for x, f in zip(held, planes))
    return tuple(torch.cat([x, f[:m - h]]) for x, f in zip(held, planes)), (tuple(f[m - h:].clone() for f in planes) if m - h < n else None)


class OnlineSettings:
    """What a session or a group is told and what its first push finds out; nothing that a stream carries.  The keywords are
    `MeshFlowStabilizer.online_session`'s, checked here for sessions and groups alike; with them come the tracker and the device.  The
    first push (`start`) adds form, the frames' `ClipForm`; rectangle, the fixed crop; crop, `ClipForm.warp_crop`'s (None: the warp goes
    out whole); out_size, the output's (width, height); taps, the smoother's, on the device; lam_newest, the newest frame's weight; dims,
    the (W, H, R, C) that the ops take; grid, a frame's path as a report shapes it, and S, its floats.  The shared stages below take one."""

    def __init__(self, stabilizer, window=40, iters=10, beta=1.0, crop_margin=0.08, output_size=None,
                 adaptive_weights_definition=host.ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, chunk_pairs=32, max_per_subframe=1024, red_first=False,
                 on_lost='hold', on_cut='ignore', cut_threshold=0.30, on_uncovered='report', limit_steps=32, limit_guard=2.0, limit_rise=2,
                 lag=0):
        from . import _lib, ops
        stabilizer._check_definition(adaptive_weights_definition)
        omega = int(stabilizer.temporal_smoothing_radius)
        if not 2 <= int(window) <= _lib.ONLINE_MAX_WINDOW:
            raise ValueError(f'window must be in 2 .. {_lib.ONLINE_MAX_WINDOW} frames (got {window})')
        self.lag = ops.check_online_lag(lag, int(window))
        if not 1 <= omega <= _lib.ONLINE_MAX_OMEGA:
            raise ValueError(f'an online session needs temporal_smoothing_radius in 1 .. {_lib.ONLINE_MAX_OMEGA} (got {omega})')
        if not 1 <= int(iters) <= _lib.ONLINE_MAX_ITERS:
            raise ValueError(f'iters must be in 1 .. {_lib.ONLINE_MAX_ITERS} (got {iters})')
        if not (math.isfinite(beta) and beta >= 0):
            raise ValueError(f'beta must be finite and >= 0 (got {beta})')
        if not (isinstance(crop_margin, (int, float)) and 0 <= crop_margin < 0.5):
            raise ValueError(f'crop_margin must lie in [0, 0.5) (got {crop_margin!r})')
        if on_lost not in ('hold', 'raise'):
            raise ValueError(f"on_lost must be 'hold' or 'raise' (got {on_lost!r})")
        if on_cut not in ('ignore', 'reset'):
            raise ValueError(f"on_cut must be 'ignore' or 'reset' (got {on_cut!r})")
        if on_uncovered not in ('report', 'limit'):
            raise ValueError(f"on_uncovered must be 'report' or 'limit' (got {on_uncovered!r})")
        self.on_uncovered = on_uncovered
        self.limit_steps, self.limit_guard, self.limit_rise = ops.check_path_limit(limit_steps, limit_guard, limit_rise,
                                                                                   ('limit_steps', 'limit_guard', 'limit_rise'))
        self.on_cut, self.cut_threshold = on_cut, ops.check_cut_threshold(cut_threshold, 'cut_threshold')
        self.stabilizer, self.window, self.omega, self.iters, self.beta = stabilizer, int(window), omega, int(iters), float(beta)
        self.crop_margin, self.output_size, self.definition = crop_margin, output_size, adaptive_weights_definition
        self.chunk_pairs, self.red_first, self.on_lost = chunk_pairs, red_first, on_lost
        self.device = stabilizer._torch_device()
        self.tracker = stabilizer.device_tracker(max_per_subframe, 'device', 'device')
        self.form = self.rectangle = self.crop = self.out_size = self.taps = self.lam_newest = self.dims = self.grid = self.S = None   # (`start`)

    def check_limit_fits(self, frames):
        """on_uncovered='limit', before the first push touches the device -- or has a form --: the rectangle widened by the guard must lie
        inside the untouched frame with a pixel to spare, or no candidate could pass and every frame would come back unstabilized."""
        first = frames[0] if isinstance(frames, (tuple, list)) and len(frames) == 2 else frames
        shape = getattr(first, 'shape', ())
        if len(shape) < 3:
            return                                  # (not a clip: `luma_of` says what is wrong with it)
        H, W = int(shape[1]), int(shape[2])
        left, top, _, _ = margin_rectangle(self.crop_margin, W, H)
        if left < self.limit_guard + 1 or top < self.limit_guard + 1:
            raise ValueError(f"on_uncovered='limit': crop_margin={self.crop_margin} leaves {left} x {top} pixels around the rectangle of a "
                             f'{W} x {H} frame, limit_guard={self.limit_guard} needs {self.limit_guard + 1:g} on every side: no correction would '
                             'pass; widen crop_margin')

    def read(self, frames):
        """What every push begins with: (the frames' `ClipForm`, their luma), behind `check_limit_fits` while no push has fixed a form."""
        if self.form is None and self.on_uncovered == 'limit':
            self.check_limit_fits(frames)
        return luma_of(frames, self.red_first)

    def start(self, form, H, W):
        """The first push: frames of `form`, H x W in luma, fix everything listed above."""
        import torch
        from . import ops
        if self.output_size is not None:
            self.output_size = (ops._yuv_output_size(form.fmt, self.output_size, 'output_size') if form.pair else
                                ops.check_output_size(self.output_size, 'output_size'))
        rectangle = margin_rectangle(self.crop_margin, W, H)
        R, C = self.stabilizer.mesh_row_count, self.stabilizer.mesh_col_count
        self.dims, self.grid, self.S = (W, H, R, C), (R + 1, C + 1, 2), (R + 1) * (C + 1) * 2
        self.taps = torch.from_numpy(host.online_taps(self.omega)).to(self.device)
        # the weight of the newest frame: the identity homography's under the chosen definition (mfs.py:273-274, 757)
        self.lam_newest = float(host.adaptive_weights(1, W, H, self.definition, np.identity(3)[None])[0])
        whole = rectangle == (0, 0, W - 1, H - 1) and self.output_size in (None, (W, H))
        self.crop = None if whole else (rectangle, self.output_size)
        self.out_size = (W, H) if whole or self.output_size is None else self.output_size
        self.form, self.rectangle = form, rectangle

    def check_started(self):
        if self.form is None:
            raise ValueError('flush before the first push: the frame size and form are not known yet')


def track_pairs(cfg, early, late, t0=None):
    """A run of pairs early[i] -> late[i], luma stacks (P, H, W), through the tracker and `ops.vertex_motion`: (their velocities (P, S)
    float32 on the device, their weights (P,) float64 from the homographies, the indices of the pairs that could not be fitted).  Such a
    pair has no motion ('hold'), or -- on_lost='raise' -- the first is a ValueError about frames t0 + i and t0 + i + 1, before any further launch."""
    import torch
    from . import _lib, ops
    s, (W, H, _, _) = cfg.stabilizer, cfg.dims
    early, late, offsets, kmax, d_hom, d_info = cfg.tracker.track_stacks_resident(early, late, cfg.chunk_pairs)
    _, d_vel, status = ops.vertex_motion(early, late, offsets, d_hom, kmax, *cfg.dims, s.feature_ellipse_row_count, s.feature_ellipse_col_count)
    homographies, info = d_hom.cpu().numpy(), d_info.cpu().numpy()          # (the one wait of a push beyond the tracker's own)
    ops.vertex_motion_check(status)
    bad = np.nonzero(info[:, 0] != _lib.HFIT_OK)[0]
    if bad.size and cfg.on_lost == 'raise':
        t = t0 + int(bad[0])
        raise ValueError(f'fewer than {s.homography_min_number_corresponding_features} features could be '
                         f'tracked from frame {t} to frame {t + 1}')
    d_vel = d_vel.reshape(-1, cfg.S)
    if bad.size:
        # The fit left the identity there, whose weight is lam_newest's; an empty feature range gives a zero velocity by itself
        # (oracle/motion_oracle.py), a refused fit over a non-empty range does not
        d_vel = d_vel.index_fill(0, torch.from_numpy(bad).to(cfg.device), 0.0)
    return d_vel, host.adaptive_weights(len(homographies), W, H, cfg.definition, homographies), bad


def warp_rows(cfg, frames, c, p):
    """Frames with their paths (n, S) through one cell table, the format's warp and the crop-resize: (frames out, covered (n,) bool)."""
    from . import ops
    table = ops.cell_table(c, p, *cfg.dims)
    out = cfg.form.warp_crop(frames, table, cfg.stabilizer.color_outside_image_area_bgr, cfg.crop)
    table.check()
    crop = table.crop
    left, top, right, bottom = cfg.rectangle
    return out, (crop[:, 0] <= left) & (crop[:, 1] <= top) & (crop[:, 2] >= right) & (crop[:, 3] >= bottom)


def empty_result(cfg, first, lost):
    """What a part that hands out no frame returns: (0 frames of the output's dtype and trailing shape, a report with 0-row tensors, 0
    steps of the limiter or None).  No op is called."""
    import torch
    k = torch.empty(0, dtype=torch.int32, device=cfg.device) if cfg.on_uncovered == 'limit' else None
    path = torch.empty((0,) + cfg.grid, dtype=torch.float64, device=cfg.device)
    return (cfg.form.empty(*cfg.out_size, cfg.device),
            OnlineReport(first, path, path.clone(), cfg.rectangle, torch.empty(0, dtype=torch.bool, device=cfg.device), lost), k)


def join_reports(reports):
    """The reports of consecutive parts of one stream as one: `first` is the first part's, `lost` in each part's own numbering."""
    import torch
    d_unstab, d_stab, covered = (torch.cat([getattr(r, field) for r in reports]) for field in ('d_unstab', 'd_stab', 'covered'))
    return OnlineReport(reports[0].first, d_unstab, d_stab, reports[0].rectangle, covered, [t for r in reports for t in r.lost])


# What a shot carries from push to push beside the `ops.OnlineState` (its tensors and `seen`), and what each starts from: the one list
# that the constructor, `reset()`, `_snapshot()` and `_restore()` go by.
#   _last_luma: the last luma frame pushed, the early frame of the next push's first pair;
#   _last_sig:  on_cut='reset': that frame's scene-cut signature;
#   _k_prev:    on_uncovered='limit': the limiter's k of the last frame handed out, a 1-element int32 device tensor (None: k starts at K);
#   _held:      lag >= 1: the input frames not handed out yet, oldest first, as a tuple of the input's planes (`hold_frames`);
#   emitted:    how many frames of the path begun at the last reset have been handed out.
# Every one is REPLACED, never written to -- and so are the tensors behind them --, which is why a snapshot keeps references, not clones.
_CARRIED = {'_last_luma': None, '_last_sig': None, '_k_prev': None, '_held': None, 'emitted': 0}


class OnlineSession:
    """One stream of frames through `stabilizer`.  Made by `MeshFlowStabilizer.online_session`, which documents the keywords; they live in
    `settings` (`OnlineSettings`) and read as the session's own.  The session itself holds what the stream carries: `state`, an `ops.OnlineState` made by the first
    push, and the members of `_CARRIED`."""

    def __init__(self, stabilizer, *args, **keywords):
        self.settings = OnlineSettings(stabilizer, *args, **keywords)
        self.state = None             # made by the first push (`_start`)
        self.last_limit = None        # on_uncovered='limit': the last push's (n,) int32 k on the device
        # shots: the shots begun so far (the first frame, every frame after a `reset()`, every cut found); last_cuts: the indices, relative to
        # the last push, of its frames that started a shot, and last_cut_distances: that push's (n,) int32 distances -- on_cut='reset' only
        self.shots, self.last_cuts, self.last_cut_distances = 0, [], None
        self.reset()

    def __getattr__(self, name):
        """What the settings hold reads as the session's own, as when the session held it: `form`, `rectangle`, `lag`, `on_uncovered` and the rest."""
        return getattr(object.__getattribute__(self, 'settings'), name)    # (no settings, on a session made without its constructor: AttributeError)

    @property
    def seen(self):
        return self.state.seen if self.state is not None else 0

    @property
    def pending(self):
        """The frames pushed but not handed out yet: seen - emitted, at most `lag`."""
        return self.seen - self.emitted

    def reset(self):
        """Forget every frame pushed so far (a caller that knows of a cut; on_cut='reset' calls it at the cuts it finds): the next push starts
        a path at frame 0, as a fresh session's does, and its first frame is no cut.  The frame size and form stay.  With lag >= 1 the
        pending frames are DISCARDED, pixels and all: `flush()` first hands them out."""
        if self.state is not None:
            self.state.reset()
        vars(self).update(_CARRIED)

    def _snapshot(self):
        st = self.state
        return [getattr(self, name) for name in _CARRIED], self.shots, (st.c.clone(), st.q.clone(), st.lam.clone(), st.seen)

    def _restore(self, saved):
        st = self.state
        carried, self.shots, (c, q, lam, st.seen) = saved
        vars(self).update(zip(_CARRIED, carried))
        st.c.copy_(c), st.q.copy_(q), st.lam.copy_(lam)

    def flush(self):
        """The end of the stream (or of a shot the caller knows of): (the pending frames stabilized and cropped, `OnlineReport`), with the
        paths of `ops.online_pending` -- the last window's solution, beyond which there is nothing to wait for -- through the same limiter,
        warp and crop as a push's; then the session is left as `reset()` leaves it.  With lag=0, or nothing pending, the empty result: 0
        frames of the output's dtype and trailing shape and a report with 0-row tensors.  Before the first push, whose frames fix that
        shape, it is a ValueError."""
        self.settings.check_started()
        parts = [self._flush_part()]
        self.reset()
        return self._result(parts)

    _check_limit_fits = OnlineSettings.check_limit_fits                  # (it reads `crop_margin` and `limit_guard`, which a session has as above)

    def _start(self, form, H, W):
        from . import ops
        self.settings.start(form, H, W)
        self.state = ops.OnlineState(self.settings.S, self.settings.window, self.settings.device)

    def push(self, frames):
        """One or more new frames -- a stack (n, ...) in any form `stabilize_scored` takes, on the session's device -- in; returns
        (the same n frames stabilized and cropped, in the input's form, `OnlineReport`).  on_cut='reset': the frames are scored first
        (`ops.find_cuts` against the signature of the last frame pushed: two small launches and one wait for n integers), the block is
        split at every cut and each part pushed as a plain session would, with `reset()` before each part that begins at a cut -- the pair
        across a cut is never tracked --; the parts' frames and reports come back joined (`join`): `first` is the first part's, d_unstab,
        d_stab and covered are concatenated, `lost` is concatenated in each part's own numbering.
        lag=k >= 1: what comes back is the frames that have become final with this push, session indices [emitted, seen - k): `first` is
        the first of them (`emitted` where none came out -- the frames are then a 0-frame tensor, a pair for 4:2:0 and 4:2:2, of the output's dtype
        and trailing shape, and the report's tensors have 0 rows), d_unstab, d_stab and covered are theirs, `lost` stays that of the frames
        PUSHED.  The session keeps its own copies of the frames it still owes: the caller's buffers are free when push returns.  With
        on_cut='reset' the old shot is flushed before the `reset()` at each cut: its tail comes out of this push, in front of the new
        shot's frames."""
        from . import ops
        cfg = self.settings
        form, luma = cfg.read(frames)
        n, H, W = (int(v) for v in luma.shape)
        if n < 1:
            raise ValueError('push needs at least one frame')
        if cfg.form is None:
            self._start(form, H, W)
        else:
            cfg.form.check_same(form, 'session')
        # (what on_cut='ignore' puts in their place is what the three members hold from the start: nothing is looked for)
        cuts, distances, sig = ops.find_cuts(luma, cfg.cut_threshold, self._last_sig) if cfg.on_cut == 'reset' else ([], None, None)
        if not cuts:
            parts = [self._push_part(frames, luma)]
        else:
            starts = sorted({0, *cuts}) + [n]
            # on_lost='raise' promises the session as it was: a part may fail after an earlier one, or a reset, has changed it
            saved = self._snapshot() if cfg.on_lost == 'raise' else None
            try:
                parts = []
                for lo, hi in zip(starts[:-1], starts[1:]):
                    if lo in cuts:
                        if self.pending:
                            parts.append(self._flush_part())              # the old shot's tail, ahead of the new shot's frames
                        self.reset()
                    parts.append(self._push_part(form.part(frames, lo, hi), luma[lo:hi]))
            except ValueError:
                if saved is not None:
                    self._restore(saved)
                raise
        self._last_sig, self.last_cuts, self.last_cut_distances = sig, cuts, distances
        return self._result(parts)

    def _result(self, parts):
        """What a push or a flush returns from its parts (frames, report, k), in order; on_uncovered='limit': their k is `last_limit`."""
        import torch
        if self.settings.on_uncovered == 'limit':
            self.last_limit = parts[0][2] if len(parts) == 1 else torch.cat([k for _, _, k in parts])
        return parts[0][:2] if len(parts) == 1 else self.join([p[:2] for p in parts])

    def join(self, parts):
        """Several (frames, report) of this session's stream in order as one: the frames concatenated, the reports as `join_reports` joins them."""
        return self.form.cat([out for out, _ in parts]), join_reports([r for _, r in parts])

    def _push_part(self, frames, luma):
        """A run of frames of one shot through the session: (frames out, `OnlineReport`, the limiter's k or None)."""
        import torch
        from . import ops
        cfg = self.settings
        n, first = int(luma.shape[0]), self.state.seen
        # pairs: (the frame kept from the previous push -> new frame 0), then the adjacent new frames
        stack, k0 = (luma, 1) if self._last_luma is None else (torch.cat([self._last_luma[None], luma]), 0)
        vel = torch.zeros((n, cfg.S), dtype=torch.float32, device=cfg.device)
        lam_known = np.full(n, cfg.lam_newest)
        lost = []
        if stack.shape[0] >= 2:
            vel[k0:], lam_known[k0:], bad = track_pairs(cfg, stack[:-1], stack[1:], first + k0 - 1)
            lost = [first + k0 + int(b) for b in bad]
        block = (vel, torch.from_numpy(lam_known).to(cfg.device), self.state, cfg.taps, cfg.omega, cfg.iters, cfg.beta, cfg.lam_newest)
        c, p = ops.online_smooth_lag(*block, cfg.lag) if cfg.lag else ops.online_smooth(*block)
        self._last_luma = luma[-1].clone()
        self.shots += int(first == 0)
        # the frames that became final are the oldest of (held, new); without a lag that is the caller's frames, and nothing is held
        final, self._held = hold_frames(self._held, cfg.form.planes(frames), int(c.shape[0]))
        return self._hand_out(cfg.form.clip(final), c, p, lost) if c.shape[0] else empty_result(cfg, self.emitted, lost)

    def _flush_part(self):
        """The pending frames of the shot under way with `ops.online_pending`'s paths: (frames out, `OnlineReport`, k or None).  Leaves
        the reset to the caller."""
        from . import ops
        cfg = self.settings
        if not self.pending:
            return empty_result(cfg, self.emitted, [])
        c, p = ops.online_pending(self.state, cfg.lag)
        held, self._held = self._held, None
        return self._hand_out(cfg.form.clip(held), c, p, [])

    def _hand_out(self, frames, c, p, lost):
        """Frames of one shot whose paths are final, session indices from `emitted` on, through the limiter and `warp_rows`: a part, as `_push_part`'s."""
        from . import ops
        cfg = self.settings
        first, k = self.emitted, None
        self.emitted += int(c.shape[0])
        if cfg.on_uncovered == 'limit':
            # (behind the smoother, whose state keeps the unlimited path: blocks of any sizes give the bytes of one push)
            p, k = ops.path_limit(c, p, *cfg.dims, cfg.rectangle, cfg.limit_steps, cfg.limit_guard, cfg.limit_rise, self._k_prev)
            self._k_prev = k[-1:]
        out, covered = warp_rows(cfg, frames, c, p)
        return out, OnlineReport(first, c.view(-1, *cfg.grid), p.view(-1, *cfg.grid), cfg.rectangle, covered, lost), k


def _check_stream_count(streams):
    if isinstance(streams, bool) or not isinstance(streams, (int, np.integer)) or int(streams) < 1:
        raise ValueError(f'streams must be an int >= 1 (got {streams!r})')


class OnlineGroup:
    """`streams` live streams of one size and form through `stabilizer`, a frame of each of any subset per `push`, in ONE set of launches
    whatever the subset's size.  Made by `MeshFlowStabilizer.online_group`, which documents the keywords.  What a stream gets is what an
    `OnlineSession` of its own with the same keywords, pushed its frames one at a time, returns, byte for byte: the stages shared between
    the streams work per pair or per frame and are the functions a session calls (`track_pairs`, `warp_rows`), and the three that carry a
    stream's memory have a batched form that restates the single one per row -- `ops.online_smooth_group`, `ops.path_limit_group`,
    `ops.cut_distance_pairs`.  The keywords, and what the first push fixes, are in `settings`, an `OnlineSettings` as a session has one.
    Per stream the group carries, on the device: its slices of an `ops.OnlineGroupState`, its last luma frame (B, H, W), that frame's
    signature (B, 256) and the limiter's last step (B,), -1 where nothing is carried; on the host: `seen` and `shots`."""

    def __init__(self, stabilizer, streams, **keywords):
        _check_stream_count(streams)
        if keywords.get('lag', 0) != 0 or isinstance(keywords.get('lag', 0), bool):
            raise ValueError(f"a group takes lag=0 only (got {keywords['lag']!r}): online_lag_group(streams, lag) is the group with "
                             'look-ahead, the bytes of an online_session(lag=lag) per stream')
        self._setup(stabilizer, streams, keywords)

    def _setup(self, stabilizer, streams, keywords):
        """What every group is made of, behind the checks of `streams` and `lag`."""
        if keywords.get('on_lost', 'hold') == 'raise':
            raise ValueError(f"a group takes on_lost='hold' only (got {keywords['on_lost']!r}): one stream's lost pair must not stop the "
                             "others; it is reported in that stream's report.lost")
        self.streams = int(streams)
        self.settings = OnlineSettings(stabilizer, **keywords)
        self.state = self._last_luma = self._last_sig = self._k_prev = None       # made by the first push, which fixes the frame size
        self.shots = [0] * self.streams
        # of the last push, per pushed row: the limiter's (K,) int32 k on the device (on_uncovered='limit'); the rows at which a cut was
        # found and the (K,) int32 distances, 0 for a stream with no frame before (on_cut='reset')
        self.last_limit, self.last_cuts, self.last_cut_distances = None, [], None

    form = property(lambda self: self.settings.form)
    rectangle = property(lambda self: self.settings.rectangle)

    @property
    def seen(self):
        """The frames of each stream's path since its last reset: a list of `streams` ints."""
        return list(self.state.seen) if self.state is not None else [0] * self.streams

    def _named(self, stream):
        """The streams that `reset(stream)` or `flush(stream)` means: that one, or all of them for None."""
        from . import ops
        return list(range(self.streams)) if stream is None else ops.check_streams([stream], self.streams, 'stream')

    def reset(self, stream=None):
        """Forget every frame of `stream` (None: of every stream), as `OnlineSession.reset` does for its one: the stream's next frame
        starts a path at frame 0 and is no cut.  No byte of the state is cleared: a stream at seen = 0 reads none of it."""
        ids = self._named(stream)
        if self.state is not None:
            for b in ids:
                self.state.reset(b)
            self._k_prev[ids] = -1

    def push(self, frames, streams=None):
        """One new frame of each stream of `streams` (K distinct indices, any order; None: all of them, in order): a stack (K, ...) in any
        form a session takes, row r the frame of streams[r].  Returns (the K frames stabilized and cropped, in the input's form, a list of
        K `OnlineReport`): row r and report r belong to streams[r] and hold what that stream's own session would have returned for the
        frame.  A stream at its first frame, after `reset(stream)` or at a cut found is not tracked: it pushes a zero velocity at seen = 0."""
        from . import ops
        cfg = self.settings
        ids, d_ids, form, luma, first, vel, lam_known, lost, _ = self._front(frames, streams)
        K = len(ids)
        c, p = ops.online_smooth_group(vel, lam_known, self.state, ids, cfg.taps, cfg.omega, cfg.iters, cfg.beta, cfg.lam_newest)
        c, p = c.view(K, cfg.S), p.view(K, cfg.S)
        self._carry(ids, d_ids, luma, first)
        k = None
        if cfg.on_uncovered == 'limit':
            p, k = ops.path_limit_group(c, p, *cfg.dims, cfg.rectangle, cfg.limit_steps, cfg.limit_guard, cfg.limit_rise, self._k_prev[d_ids])
            self._k_prev[d_ids] = k
        self.last_limit = k
        out, covered = warp_rows(cfg, frames, c, p)
        c, p = c.view(K, *cfg.grid), p.view(K, *cfg.grid)
        return out, [OnlineReport(first[r], c[r:r + 1], p[r:r + 1], cfg.rectangle, covered[r:r + 1], lost[r]) for r in range(K)]

    def _carry(self, ids, d_ids, luma, first):
        """Behind the smoother: every pushed stream's last luma frame, and the shots begun."""
        self._last_luma[d_ids] = luma
        for r, b in enumerate(ids):
            self.shots[b] += int(first[r] == 0)

    def _begin(self, form, H, W, frames):
        """The first push: the frame size and form fix the settings and the per-stream state."""
        import torch
        from . import _lib, ops
        cfg = self.settings
        cfg.start(form, H, W)
        self.state = ops.OnlineGroupState(self.streams, cfg.S, cfg.window, cfg.device)
        self._last_luma = torch.empty((self.streams, H, W), dtype=torch.uint8, device=cfg.device)
        self._last_sig = torch.zeros((self.streams, _lib.CUT_COUNTERS), dtype=torch.int32, device=cfg.device)
        self._k_prev = torch.full((self.streams,), -1, dtype=torch.int32, device=cfg.device)

    def _front(self, frames, streams, tail=None):
        """A push up to the smoother, shared by the groups: the checks, luma, the cut decisions, the tracked pairs (`track_pairs`).
        Returns (ids, d_ids, form, luma, first -- each row's stream's `seen` --, vel (K, 1, S), lam_known (K, 1) on the device, lost per
        row, tails: per row at which a cut was found, what `tail(stream)` returned for the old shot before the stream's reset, or None)."""
        import torch
        from . import ops
        cfg = self.settings
        ids = ops.check_streams(range(self.streams) if streams is None else streams, self.streams)
        K = len(ids)
        form, luma = cfg.read(frames)
        n, H, W = (int(v) for v in luma.shape)
        if n != K:
            raise ValueError(f'push takes one frame per pushed stream: {K} streams, {n} frames')
        if cfg.form is None:
            self._begin(form, H, W, frames)
        else:
            cfg.form.check_same(form, 'group')
        seen = self.state.seen
        d_ids = torch.tensor(ids, dtype=torch.int64, device=cfg.device)

        # cuts: every row against its own stream's last signature, one wait for the K distances
        cuts, distances, tails = [], None, {}
        if cfg.on_cut == 'reset':
            sig = ops.frame_signatures(luma)
            distances = ops.cut_distance_pairs(self._last_sig[d_ids], sig).cpu().numpy()
            distances[np.array([seen[b] == 0 for b in ids])] = 0           # no frame before: nothing to be far from, never a cut
            cuts = [int(r) for r in np.nonzero(distances.astype(np.int64) > ops.cut_bound(cfg.cut_threshold, W, H))[0]]
            self._last_sig[d_ids] = sig
            for r in cuts:                                                  # (the pair across a cut is never tracked)
                tails[r] = tail(ids[r]) if tail else None
                self.reset(ids[r])
        self.last_cuts, self.last_cut_distances = cuts, distances

        # the pairs (a stream's last luma -> its new frame) of the streams that have a frame before, through the tracker together
        first = [seen[b] for b in ids]
        rows = [r for r in range(K) if first[r] > 0]
        vel = torch.zeros((K, 1, cfg.S), dtype=torch.float32, device=cfg.device)
        lam_known = np.full((K, 1), cfg.lam_newest)
        lost = [[] for _ in ids]
        if rows:
            everyone = len(rows) == K
            d_rows = None if everyone else torch.tensor(rows, dtype=torch.int64, device=cfg.device)
            early = self._last_luma[d_ids if everyone else d_ids[d_rows]]
            d_vel, lam_known[rows, 0], bad = track_pairs(cfg, early, luma if everyone else luma[d_rows])
            for b in bad:
                lost[rows[int(b)]] = [first[rows[int(b)]]]
            if everyone:
                vel = d_vel[:, None].contiguous()
            else:
                vel[d_rows] = d_vel[:, None]
        return ids, d_ids, form, luma, first, vel, torch.from_numpy(lam_known).to(cfg.device), lost, tails


class OnlineLagGroup(OnlineGroup):
    """An `OnlineGroup` whose streams each have `lag` frames of look-ahead.  Made by `MeshFlowStabilizer.online_lag_group`, which documents
    the contract: a stream gets the bytes of an `OnlineSession` of its own with lag=lag.  Everything up to the smoother is `OnlineGroup`'s
    (`_front`); behind it the smoother is `ops.online_smooth_group_lag`, and the pixels a stream still owes live in a ring per plane of the
    clip form, (streams, lag, ...) on the device -- frame t of a stream in slot t mod lag --, which one `ops.ring_exchange` per plane and
    tick both fills and hands out from.  Memory: streams * lag frames per plane, allocated at the first push.  Beside `OnlineGroup`'s state
    the group carries, on the host, `emitted` per stream (the frames handed out since its last reset) and whether the limiter carries a
    step for it."""

    def __init__(self, stabilizer, streams, lag, **keywords):
        _check_stream_count(streams)
        if not isinstance(lag, bool) and isinstance(lag, (int, np.integer)) and int(lag) == 0:
            raise ValueError('a lagged group takes lag in 1 .. window - 1 (got 0): online_group(streams) is the group without look-ahead')
        self._setup(stabilizer, streams, dict(keywords, lag=lag))         # (the settings' own checks of window and lag)
        self.lag = self.settings.lag
        self.emitted, self._limited = [0] * self.streams, [False] * self.streams
        self._rings = None                                                  # per plane (streams, lag, ...), made by the first push
        self.last_counts = []                                               # of the last push or flush: the frames of `out` per row

    @property
    def pending(self):
        """The frames of each stream pushed but not handed out yet, at most `lag`: a list of `streams` ints."""
        return [a - b for a, b in zip(self.seen, self.emitted)]

    def reset(self, stream=None):
        """`OnlineGroup.reset`; the pending frames of those streams are DISCARDED -- `flush(stream)` first hands them out.  No ring byte is
        cleared: a stream at seen = 0 reads none of its slots."""
        super().reset(stream)
        for b in self._named(stream):
            self.emitted[b], self._limited[b] = 0, False

    def _begin(self, form, H, W, frames):
        import torch
        planes = form.planes(frames)
        size = sum(self.streams * self.lag * int(p[0].numel()) * p.element_size() for p in planes)
        try:
            rings = tuple(torch.empty((self.streams, self.lag) + tuple(p.shape[1:]), dtype=p.dtype, device=self.settings.device) for p in planes)
        except RuntimeError as e:                                           # (torch's out-of-memory error is one)
            raise ValueError(f'a lagged group of {self.streams} streams at lag={self.lag} holds streams * lag frames on the device: '
                             f'{size} bytes could not be allocated ({str(e).splitlines()[0]})') from None
        super()._begin(form, H, W, frames)
        self._rings = rings

    def _tail(self, stream):
        """The pending frames of `stream` with `ops.online_pending_group`'s paths through the single-stream limiter and `warp_rows` --
        `OnlineSession._flush_part` on the stream's slices, launches of its own --: (frames out, `OnlineReport`, k or None), or None where
        nothing is pending.  Leaves the reset to the caller."""
        import torch
        from . import ops
        cfg = self.settings
        n, seen, first, k = self.pending[stream], self.state.seen[stream], self.emitted[stream], None
        if not n:
            return None
        (c, p), = ops.online_pending_group(self.state, [stream], self.lag)
        # oldest first: slots (seen - n) mod lag onwards, in one run or two around the ring's end (slices: torch indexes no uint16 tensor);
        # the warp below reads them on this stream before the tick's exchange writes a slot
        lo = (seen - n) % self.lag
        wrap = max(0, lo + n - self.lag)
        frames = cfg.form.clip([torch.cat([ring[stream, lo:], ring[stream, :wrap]]) if wrap else ring[stream, lo:lo + n] for ring in self._rings])
        if cfg.on_uncovered == 'limit':
            p, k = ops.path_limit(c, p, *cfg.dims, cfg.rectangle, cfg.limit_steps, cfg.limit_guard, cfg.limit_rise,
                                  self._k_prev[stream:stream + 1].clone() if self._limited[stream] else None)
        out, covered = warp_rows(cfg, frames, c, p)
        self.emitted[stream] += n
        return out, OnlineReport(first, c.view(n, *cfg.grid), p.view(n, *cfg.grid), cfg.rectangle, covered, []), k

    def _result(self, parts):
        """What a push or a flush returns from its rows' parts -- per row a list of (frames, report, k) in order, as a session's parts
        are --: (the frames joined in order, a report per row).  Sets `last_counts` and, with on_uncovered='limit', `last_limit`: the k of
        every frame of `out`."""
        import torch
        cfg = self.settings
        flat = [part for row in parts for part in row]
        self.last_counts = [sum(int(r.d_stab.shape[0]) for _, r, _ in row) for row in parts]
        if cfg.on_uncovered == 'limit':
            self.last_limit = flat[0][2] if len(flat) == 1 else torch.cat([k for _, _, k in flat])
        clips = [out for out, r, _ in flat if r.d_stab.shape[0]] or [flat[0][0]]           # (no frame at all: 0 frames are the answer)
        out = clips[0] if len(clips) == 1 else cfg.form.cat(clips)
        return out, [row[0][1] if len(row) == 1 else join_reports([r for _, r, _ in row]) for row in parts]

    def flush(self, stream=None):
        """The end of `stream` (None: of every stream): (its pending frames stabilized and cropped -- of all the named streams, in order --,
        a list of an `OnlineReport` per named stream), with the last window's solution as their paths, as `OnlineSession.flush` does for
        its one; then `reset(stream)`.  A stream with nothing pending gives a 0-row report.  Before the first push it is a ValueError."""
        self.settings.check_started()
        parts = []
        for b in self._named(stream):
            parts.append([self._tail(b) or empty_result(self.settings, self.emitted[b], [])])
            self.reset(b)
        return self._result(parts)

    def push(self, frames, streams=None):
        """One new frame of each stream of `streams`, as `OnlineGroup.push` takes them.  Returns (the frames handed out this tick, in row
        order, a list of K `OnlineReport`): row r hands out its stream's frame seen - lag once the stream has more than `lag` frames -- a
        report of one row --, nothing before -- a report of 0 rows --, and at a cut found its old shot's tail; `last_counts[r]` is how many
        frames of the output are row r's, `first` the stream's index of the first of them, `lost` that of the frame PUSHED."""
        import torch
        from . import ops
        cfg = self.settings
        ids, d_ids, form, luma, first, vel, lam_known, lost, tails = self._front(frames, streams, self._tail)
        K = len(ids)
        c, p, final = ops.online_smooth_group_lag(vel, lam_known, self.state, ids, cfg.taps, cfg.omega, cfg.iters, cfg.beta, cfg.lam_newest, self.lag)
        c, p = c.view(K, cfg.S), p.view(K, cfg.S)
        self._carry(ids, d_ids, luma, first)

        # the new frames into their slots, the owed ones out of them: row r's frame `first[r]` takes the slot of frame first[r] - lag
        emit = [r for r in range(K) if final[r] == 1]
        M = len(emit)
        out_row = {r: j for j, r in enumerate(emit)}
        rows = np.array([(b, first[r] % self.lag, out_row.get(r, -1)) for r, b in enumerate(ids)], dtype=np.int32)
        owed = [ops.ring_exchange(ring, plane, rows, M) for ring, plane in zip(self._rings, form.planes(frames))]

        parts = [[tails[r]] if tails.get(r) else [] for r in range(K)]         # the old shot's tail, ahead of the new shot's frames
        if M:
            k = None
            if M < K:
                d_emit = torch.tensor(emit, dtype=torch.int64, device=cfg.device)
                c, p, d_ids = c[d_emit], p[d_emit], d_ids[d_emit]
            if cfg.on_uncovered == 'limit':
                p, k = ops.path_limit_group(c, p, *cfg.dims, cfg.rectangle, cfg.limit_steps, cfg.limit_guard, cfg.limit_rise, self._k_prev[d_ids])
                self._k_prev[d_ids] = k
            out, covered = warp_rows(cfg, form.clip(owed), c, p)
            c, p = c.view(M, *cfg.grid), p.view(M, *cfg.grid)
            for j, r in enumerate(emit):
                b = ids[r]
                report = OnlineReport(self.emitted[b], c[j:j + 1], p[j:j + 1], cfg.rectangle, covered[j:j + 1], lost[r])
                parts[r].append((out if M == 1 else form.part(out, j, j + 1), report, None if k is None else k if M == 1 else k[j:j + 1]))
                self.emitted[b] += 1
                self._limited[b] = k is not None
        for r, b in enumerate(ids):
            if r not in out_row:
                parts[r].append(empty_result(cfg, self.emitted[b], lost[r]))
        if M == K:                                                          # the steady tick: the warp's output and the limiter's k as they are
            self.last_counts, self.last_limit = [1] * K, k
            return out, [row[0][1] for row in parts]
        return self._result(parts)
