"""`MeshFlowStabilizer`: the reference's class surface with its two hot methods on an MI355X.

Mirrors /root/reference/meshflowstabilizer.py (`mfs.py`): constructor keywords and defaults
(mfs.py:43-49), the four enum values and two constants (mfs.py:32-40), `stabilize(input_path,
output_path, adaptive_weights_definition)` and its `(cropping_ratio, distortion_score,
stability_score)` return (mfs.py:102-169), and the two private methods that form the drop-in boundary:

    _get_stabilized_vertex_displacements          mfs.py:632-710    Jacobi sweep      -> HIP kernel 1
    _get_stabilized_frames_and_crop_boundaries    mfs.py:909-1108   mesh warp + crop  -> HIP kernels 2a/2b

Both take and return NumPy arrays exactly like the reference (host buffers in, host buffers out); the
`*_device` variants keep everything in HBM and are what `stabilize_clip` and bench.py use.  Video
decode/encode, the FAST/LK/RANSAC front-end and the two feature-based metrics are outside this path
(they need OpenCV); `stabilize()` needs `cv2` for them and says so when it is missing.
"""
import numpy as np

from . import host

try:  # progress bars are optional
    import tqdm as _tqdm  # noqa: F401
except Exception:  # pragma: no cover
    _tqdm = None


def _torch_device_of(self):
    """The torch device of a stabilizer(-like) object: its `device` attribute, None / absent / 'cuda' = the CURRENT HIP device."""
    import torch
    if not torch.cuda.is_available():
        raise RuntimeError('no MI355X visible: the meshflow_amd hot path has no CPU fallback')
    name = getattr(self, 'device', None)
    dev = torch.device(name if name is not None else 'cuda')
    if dev.index is None:                 # 'cuda' without an index means the caller's CURRENT device, not device 0
        dev = torch.device(dev.type, torch.cuda.current_device())
    return dev


# The host-frame C calls (csrc/hostpipe.hip) by HostClip.channels: warp, warp + _crop_frames, _crop_frames alone, and the last two to a
# caller-chosen output size
_HOST_CALLS = {3: ('mf_warp_u8c3_host_frames', 'mf_warp_crop_u8c3_host_frames', 'mf_crop_resize_u8c3_host_frames',
                   'mf_warp_crop_to_u8c3_host_frames', 'mf_crop_resize_to_u8c3_host_frames'),
               1: ('mf_warp_u8c1_host_frames', 'mf_warp_crop_u8c1_host_frames', 'mf_crop_resize_u8c1_host_frames',
                   'mf_warp_crop_to_u8c1_host_frames', 'mf_crop_resize_to_u8c1_host_frames')}


def _warp_host_c(self, clip, unstab, stab, crop=False, keep_uncropped=True, output_size=None):
    """Host frames in -> host frames out through the C ABI's own chunked pipeline (csrc/hostpipe.hip:
    `mf_warp_u8c3_host_frames`, upload / kernel / download threads below Python, GIL released for the whole call).
    Grey clips (HostClip.channels == 1) take the u8c1 twins of these calls and come back as (F, H, W) arrays.
    Returns (stabilized frames (F, H, W, 3) uint8 array, clip-level crop bounds as np.int64 (left, top, right,
    bottom), mfs.py:1103-1106).  crop=True: `mf_warp_crop_u8c3_host_frames` -- the same pipeline followed by `_crop_frames`
    (mfs.py:159, 1111-1157) on the device; returns (stabilized frames or None when keep_uncropped is False, bounds,
    cropped + resized frames (F, H, W, 3)); output_size=(width, height) resizes the crop to that size instead
    (`mf_warp_crop_to_u8c3_host_frames`: (F, height, width, 3))."""
    import ctypes
    import torch
    from . import _lib, ops, pipeline
    dev = self._torch_device()
    n, H, W = clip.num_frames, clip.height, clip.width
    frames = [clip.array[i] for i in range(n)] if clip.array is not None else clip.frames      # (validated by HostClip, every one of them)
    warp_fn, warp_crop_fn, _, warp_crop_to_fn, _ = (getattr(_lib.lib, name) for name in _HOST_CALLS[clip.channels])
    fb = H * W * clip.channels
    want_out = keep_uncropped or not crop
    out = np.empty((n,) + clip.frame_shape, dtype=np.uint8) if want_out else None
    pin = (ctypes.c_void_p * n)(*[f.ctypes.data for f in frames])
    pout = (ctypes.c_void_p * n)(*[out.ctypes.data + i * fb for i in range(n)]) if want_out else None
    per_frame = np.empty((n, 4), dtype=np.int32)
    border = ops.pixel_format(torch.uint8, (n,) + clip.frame_shape).border(self.color_outside_image_area_bgr)   # (grey: the first component)
    args = (unstab.ctypes.data_as(ctypes.c_void_p), stab.ctypes.data_as(ctypes.c_void_p), n, W, H,
            self.mesh_row_count, self.mesh_col_count, border, per_frame.ctypes.data_as(ctypes.c_void_p))
    # the library works on the calling thread's current HIP device: scope it like every other path here does (and leave the
    # caller's current device as it was)
    with torch.cuda.device(dev):
        if not crop:
            _lib.check(warp_fn(pin, pout, *args, None))
            bounds = (np.int64(per_frame[:, 0].max()), np.int64(per_frame[:, 1].max()),
                      np.int64(per_frame[:, 2].min()), np.int64(per_frame[:, 3].min()))
            return out, bounds
        oW, oH = output_size if output_size is not None else (W, H)
        cropped = np.empty((n, oH, oW) + clip.frame_shape[2:], dtype=np.uint8)
        fbc = oH * oW * clip.channels
        pcrop = (ctypes.c_void_p * n)(*[cropped.ctypes.data + i * fbc for i in range(n)])
        rect = (ctypes.c_int32 * 4)()
        if output_size is None:
            _lib.check(warp_crop_fn(pin, pout, pcrop, *args, rect, None))
        else:
            _lib.check(warp_crop_to_fn(pin, pout, pcrop, *args[:-1], oW, oH, args[-1], rect, None))
    return out, tuple(np.int64(v) for v in rect), cropped


class DegenerateMeshError(ValueError):
    """A resident clip had mesh cells without a homography (cv2.findHomography would return None and the reference dies inside cv2,
    mfs.py:1041-1042); its frames are undefined.  `clip_serial`: the clip's serial number -- `MeshFlowStabilizer.resident_serial` right
    after the `stabilize_resident` call that issued it; `cells`: how many cells.  A ValueError, as before."""

    def __init__(self, cells, clip_serial):
        where = f' in resident clip #{clip_serial}' if clip_serial is not None else ''       # (None: `stabilization_maps`, no resident clip)
        super().__init__(f'{cells} degenerate mesh cell(s){where}: no homography exists '
                         '(cv2.findHomography would return None); its frames are undefined')
        self.cells, self.clip_serial = cells, clip_serial


class UnusableCropError(ValueError):
    """The clip-level crop rectangle of a resident clip issued with crop=True cannot be used: it is empty (right < left or bottom < top:
    the stabilised frames share no fully covered area) or leaves the frame -- where the reference's cv2.resize fails on an empty source
    (mfs.py:1150-1155) and `ops.crop_resize` raises.  The clip's cropped frames are whatever the buffer held before; its uncropped frames,
    rectangle and displacements are valid.  `clip_serial`: as for `DegenerateMeshError`."""

    def __init__(self, clip_serial):
        super().__init__(f'the crop rectangle of resident clip #{clip_serial} is empty or outside the frame (cv2.resize would fail on an '
                         'empty source); its cropped frames are undefined')
        self.clip_serial = clip_serial


class MeshFlowStabilizer:
    ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL = 0
    ADAPTIVE_WEIGHTS_DEFINITION_FLIPPED = 1
    ADAPTIVE_WEIGHTS_DEFINITION_CONSTANT_HIGH = 2
    ADAPTIVE_WEIGHTS_DEFINITION_CONSTANT_LOW = 3

    ADAPTIVE_WEIGHTS_DEFINITION_CONSTANT_HIGH_VALUE = 100
    ADAPTIVE_WEIGHTS_DEFINITION_CONSTANT_LOW_VALUE = 1

    def __init__(self, mesh_row_count=16, mesh_col_count=16,
                 mesh_outlier_subframe_row_count=4, mesh_outlier_subframe_col_count=4,
                 feature_ellipse_row_count=10, feature_ellipse_col_count=10,
                 homography_min_number_corresponding_features=4,
                 temporal_smoothing_radius=10, optimization_num_iterations=100,
                 color_outside_image_area_bgr=(0, 0, 255),
                 visualize=False, device=None):
        self.mesh_col_count = mesh_col_count
        self.mesh_row_count = mesh_row_count
        self.mesh_outlier_subframe_row_count = mesh_outlier_subframe_row_count
        self.mesh_outlier_subframe_col_count = mesh_outlier_subframe_col_count
        self.feature_ellipse_row_count = feature_ellipse_row_count
        self.feature_ellipse_col_count = feature_ellipse_col_count
        self.homography_min_number_corresponding_features = homography_min_number_corresponding_features
        self.temporal_smoothing_radius = temporal_smoothing_radius
        self.optimization_num_iterations = optimization_num_iterations
        self.color_outside_image_area_bgr = color_outside_image_area_bgr
        self.visualize = visualize
        self.device = device          # extra keyword: torch device string; None = current HIP device

    # ------------------------------------------------------------------------------------------
    # public API
    # ------------------------------------------------------------------------------------------

    @staticmethod
    def _check_definition(adaptive_weights_definition):
        if adaptive_weights_definition not in host.VALID_DEFINITIONS:          # mfs.py:136-146
            raise ValueError(
                'Invalid value for `adaptive_weights_definition`. Expecting value of '
                '`MeshFlowStabilizer.ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL`, '
                '`MeshFlowStabilizer.ADAPTIVE_WEIGHTS_DEFINITION_FLIPPED`, '
                '`MeshFlowStabilizer.ADAPTIVE_WEIGHTS_DEFINITION_CONSTANT_HIGH`, or'
                '`MeshFlowStabilizer.ADAPTIVE_WEIGHTS_DEFINITION_CONSTANT_LOW`.')

    def stabilize(self, input_path, output_path, adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL):
        """Same contract as mfs.py:102-169: reads `input_path`, writes the stabilized video to `output_path`, returns
        (cropping_ratio, distortion_score, stability_score).  Video I/O, the FAST/LK/RANSAC tracker and the two
        feature-based scores are OpenCV calls in the reference and stay OpenCV calls here (`frontend_cv2.py`, needs
        `cv2`); everything between the tracker and the encoder runs on the MI355X."""
        self._check_definition(adaptive_weights_definition)
        from . import frontend_cv2
        cv2 = frontend_cv2.require_cv2()
        if self.overlap_video_io and not self._boundary_overridden(self._BOUNDARY_METHODS + self._OPENCV_METHODS):
            # nothing replaced: decode || track || upload, then the device path, then download || encode || scores
            from . import streaming
            return streaming.stabilize_streamed(self, cv2, input_path, output_path, adaptive_weights_definition)
        unstabilized_frames, num_frames, frames_per_second, codec = self._get_unstabilized_frames_and_video_features(input_path)
        disp, homographies = self._get_unstabilized_vertex_displacements_and_homographies(num_frames, unstabilized_frames)
        if self._boundary_overridden():
            # A subclass (or an instance attribute) replaces one of the reference's boundary methods: keep the reference's
            # own call sequence (mfs.py:150-162) so that the replacement is honoured, at the price of one PCIe round trip
            # per method instead of one for the whole path.
            stab = self._get_stabilized_vertex_displacements(
                num_frames, unstabilized_frames, adaptive_weights_definition, disp, homographies)               # mfs.py:150
            stabilized_frames, crop_boundaries = self._get_stabilized_frames_and_crop_boundaries(
                num_frames, unstabilized_frames, disp, stab)                                                     # mfs.py:154
            cropped_frames = self._crop_frames(stabilized_frames, crop_boundaries)                               # mfs.py:159
            stability_score = self._compute_stability_score(num_frames, stab)                                    # mfs.py:162
        else:
            _, _, stab, stability_score, cropped_frames = self.stabilize_clip(
                unstabilized_frames, disp, homographies, adaptive_weights_definition, crop=True, keep_uncropped=False)
        cropping_ratio, distortion_score = self._compute_cropping_ratio_and_distortion_score(
            num_frames, unstabilized_frames, cropped_frames)
        self._write_stabilized_video(output_path, num_frames, frames_per_second, codec, cropped_frames)
        if self.visualize:
            frontend_cv2.show_loop(cv2, frames_per_second, unstabilized_frames, cropped_frames)
        return (cropping_ratio, distortion_score, stability_score)

    _BOUNDARY_METHODS = ('_get_stabilized_vertex_displacements', '_get_stabilized_frames_and_crop_boundaries',
                         '_crop_frames', '_compute_stability_score')

    _OPENCV_METHODS = ('_get_unstabilized_frames_and_video_features', '_get_unstabilized_vertex_displacements_and_homographies',
                       '_get_matched_features_and_homography', '_compute_cropping_ratio_and_distortion_score',
                       '_write_stabilized_video')
    overlap_video_io = True      # False: `stabilize` runs its stages one after the other, like the reference

    def _boundary_overridden(self, names=None):
        """True when one of the reference's boundary methods (called at mfs.py:150-162) is not this class's
        own implementation: overridden in a subclass or patched on the instance."""
        for name in names or self._BOUNDARY_METHODS:
            if name in vars(self) or getattr(type(self), name) is not getattr(MeshFlowStabilizer, name):
                return True
        return False

    # ---- the reference's OpenCV-side helpers, same names, delegating to cv2 (frontend_cv2.py) ----

    def _tracker(self):
        from . import frontend_cv2
        return frontend_cv2.Tracker(frontend_cv2.require_cv2(), self.mesh_outlier_subframe_row_count,
                                    self.mesh_outlier_subframe_col_count,
                                    self.homography_min_number_corresponding_features)

    def _get_unstabilized_frames_and_video_features(self, input_path):
        """mfs.py:172-213."""
        from . import frontend_cv2
        return frontend_cv2.read_video(frontend_cv2.require_cv2(), input_path)

    def _get_matched_features_and_homography(self, early_frame, late_frame):
        """mfs.py:455-528."""
        return self._tracker().track_pair(early_frame, late_frame)

    def _get_unstabilized_vertex_displacements_and_homographies(self, num_frames, unstabilized_frames):
        """mfs.py:236-284: the tracker on every adjacent frame pair (cv2, host threads), then the accumulation of
        their features into vertex displacements on the device."""
        tracked = self._tracker().track_pairs(unstabilized_frames[:-1], unstabilized_frames[1:])
        homographies = np.empty((num_frames, 3, 3))
        homographies[-1] = np.identity(3)                                                   # mfs.py:274
        for t, (_, _, h) in enumerate(tracked):
            if h is None:      # the reference hands None to cv2.perspectiveTransform (mfs.py:325) and dies in cv2
                raise ValueError(f'fewer than {self.homography_min_number_corresponding_features} features could be '
                                 f'tracked from frame {t} to frame {t + 1}')
            homographies[t] = h
        frame_height, frame_width = unstabilized_frames[0].shape[:2]
        return self._get_unstabilized_vertex_displacements_from_features(
            num_frames, frame_width, frame_height, [(e, l) for e, l, _ in tracked], homographies)

    def device_tracker(self, max_per_subframe=1024, outliers='host', fit='host'):
        """The tracker that needs no OpenCV (tracker.py): FAST + LK as HIP kernels, the outlier step in NumPy (outliers='host') or as a HIP
        kernel (outliers='device'), the homography in NumPy (fit='host') or as HIP kernels (fit='device', with outliers='device' only)."""
        from . import tracker
        tracker.check_fit(fit, tracker.check_outliers(outliers))
        return tracker.DeviceTracker(self.mesh_outlier_subframe_row_count, self.mesh_outlier_subframe_col_count,
                                     self.homography_min_number_corresponding_features, self._torch_device(), max_per_subframe,
                                     outliers=outliers, fit=fit)

    def estimate_motion(self, d_grey, chunk_pairs=32, max_per_subframe=1024, outliers='host', fit='host', red_first=False):
        """mfs.py:236-284 for a clip that is already on the device: `d_grey` (F, H, W) uint8 -- grey frames or the luma plane of an NV12
        clip -- through `device_tracker()` and `_get_unstabilized_vertex_displacements_from_features`.  Returns (d_disp (F, R+1, C+1, 2)
        float64 device tensor, homographies (F, 3, 3) float64 with the identity last, mfs.py:273-274): what `stabilize_resident`,
        `stabilized_nv12`, `stabilized_p010` and `stabilized_planes` take.  ValueError where a pair cannot be tracked, as in
        `_get_unstabilized_vertex_displacements_and_homographies`.  outliers='device': the outlier step runs on the device as well
        (`ops.ransac_inliers`, tests/ransac_model.py), the packed features go straight to `ops.vertex_motion` and d_disp never visits the
        host; only the survivors come down, for the one homography fit per pair.  fit='device' (with outliers='device'): that fit runs on the
        device too (`ops.fit_homographies`, tests/homography_model.py -- within rounding of the host fit), its homographies go to
        `ops.vertex_motion` as they are, and all that comes down is the (F - 1, 9) matrices and their (F - 1, 4) records.
        A clip that is not luma yet -- (F, H, W, 3) uint8 or uint16 BGR, (F, H, W, 4) uint8 BGRA, or the (F, H, W) uint16 luma plane of a P010
        clip -- goes through `ops.luma` first (tests/luma_model.py; red_first: channel 0 is red) and is tracked as that uint8
        stack; a uint8 (F, H, W) stack takes the same launches as ever."""
        import torch
        from . import ops, tracker
        if ops.luma_source(d_grey) is not None:
            d_grey = ops.luma(d_grey, red_first)
        if tracker.check_fit(fit, tracker.check_outliers(outliers)) == 'device':
            d_early, d_late, d_offsets, kmax, d_hom, d_info = self.device_tracker(max_per_subframe, outliers, fit).track_clip_resident(d_grey, chunk_pairs)
            num_frames, frame_height, frame_width = d_grey.shape
            d_disp, _, status = ops.vertex_motion(d_early, d_late, d_offsets, d_hom, kmax, frame_width, frame_height, self.mesh_row_count,
                                                  self.mesh_col_count, self.feature_ellipse_row_count, self.feature_ellipse_col_count)
            t = ops.fit_check(d_info)
            if t is not None:
                raise ValueError(f'fewer than {self.homography_min_number_corresponding_features} features could be '
                                 f'tracked from frame {t} to frame {t + 1}')
            ops.vertex_motion_check(status)
            homographies = np.empty((num_frames, 3, 3))
            homographies[:-1] = d_hom.cpu().numpy()
            homographies[-1] = np.identity(3)                                               # mfs.py:274
            return d_disp, homographies
        if outliers == 'device':
            tracked, (d_early, d_late, d_offsets, kmax) = self.device_tracker(max_per_subframe, outliers).track_clip_packed(d_grey, chunk_pairs)
        else:
            tracked = self.device_tracker(max_per_subframe).track_clip(d_grey, chunk_pairs)
        num_frames, frame_height, frame_width = d_grey.shape
        homographies = np.empty((num_frames, 3, 3))
        homographies[-1] = np.identity(3)                                                   # mfs.py:274
        for t, (_, _, h) in enumerate(tracked):
            if h is None:
                raise ValueError(f'fewer than {self.homography_min_number_corresponding_features} features could be '
                                 f'tracked from frame {t} to frame {t + 1}')
            homographies[t] = h
        if outliers == 'device':
            d_disp, _, status = ops.vertex_motion(
                d_early, d_late, d_offsets, torch.from_numpy(np.ascontiguousarray(homographies[:num_frames - 1])).to(self._torch_device()), kmax,
                frame_width, frame_height, self.mesh_row_count, self.mesh_col_count, self.feature_ellipse_row_count,
                self.feature_ellipse_col_count)
            ops.vertex_motion_check(status)
            return d_disp, homographies
        disp, homographies = self._get_unstabilized_vertex_displacements_from_features(
            num_frames, frame_width, frame_height, [(e, l) for e, l, _ in tracked], homographies)
        return torch.from_numpy(disp).to(self._torch_device()), homographies

    def _compute_cropping_ratio_and_distortion_score(self, num_frames, unstabilized_frames, cropped_frames):
        """mfs.py:1160-1212."""
        from . import frontend_cv2
        return frontend_cv2.cropping_and_distortion(self._tracker(), unstabilized_frames[:num_frames],
                                                    cropped_frames[:num_frames])

    def cropping_and_distortion_resident(self, d_unstabilized, d_cropped, chunk_pairs=32, max_per_subframe=1024):
        """mfs.py:1160-1212 for two resident (F, H, W) uint8 stacks of equal shape -- grey frames or luma planes, the unstabilized clip and
        its stabilized, cropped version scaled back to the clip's own size -- without OpenCV: `device_tracker(max_per_subframe, 'device',
        'device').track_stacks_resident` on the pairs (unstabilized[t], cropped[t]), then `ops.feature_scores` with the fit's record
        (tests/scores_model.py: within one float32 ulp per frame of the reference's np.linalg.eigvals formulation).  Returns
        (cropping_ratio, distortion_score) as np.float32 -- the float32 mean and the float32 MINIMUM, the reference's choices.  Where the
        tracker fits no homography for a frame the reference dies with a TypeError on None; this raises a ValueError that names the frame.
        Everything runs on torch's current stream; the call waits for it once, for the 8-byte record and the two scores."""
        import torch
        from . import ops
        for t, name in ((d_unstabilized, 'd_unstabilized'), (d_cropped, 'd_cropped')):
            if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() != 3:
                raise ValueError(f'{name} must be a one-channel uint8 tensor (F, H, W): the device tracker takes grey or luma only')
        if d_unstabilized.shape != d_cropped.shape:
            raise ValueError(f"the feature scores need the crop at the clip's own size: the unstabilized stack is "
                             f'{tuple(d_unstabilized.shape)}, the cropped one {tuple(d_cropped.shape)} (crop without output_size)')
        tracker = self.device_tracker(max_per_subframe, 'device', 'device')
        tracked = tracker.track_stacks_resident(tracker._device_stack(d_unstabilized, 'd_unstabilized'),
                                                tracker._device_stack(d_cropped, 'd_cropped'), chunk_pairs)
        scores, _, record = ops.feature_scores(tracked[4], tracked[5])
        t = ops.feature_scores_check(record)
        if t is not None:
            raise ValueError(f'fewer than {self.homography_min_number_corresponding_features} features could be tracked from unstabilized '
                             f'frame {t} to cropped frame {t}')
        cropping_ratio, distortion_score = scores.cpu().numpy()
        return cropping_ratio, distortion_score

    def stabilize_scored(self, clip, adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, chunk_pairs=32, max_per_subframe=1024,
                         red_first=False):
        """The reference's stabilize() between decoder and encoder (mfs.py:140-169) for a resident clip, without OpenCV: `clip` is an
        (F, H, W) uint8 grey tensor, (F, H, W, 3) uint8 or uint16 BGR frames, (F, H, W, 4) uint8 BGRA frames (red_first: RGB / RGBA), an NV12
        pair (d_y (F, H, W), d_uv (F, H/2, W/2, 2)) of uint8 or a P010 pair of the same shapes of uint16 -- the pair's dtype tells the two
        apart --, or an NV16 pair (d_y (F, H, W), d_uv (F, H, W/2, 2)) of uint8 or a P210 pair of the same shapes of uint16, which their d_uv's rows
        tell from NV12 and P010 (a packed 4:2:2 clip is unpacked by the caller: `ops.unpack_422`, `ops.unpack_y210`).  In order: the clip's form and luma (`online.luma_of`: itself for grey, NV12 and NV16,
        `ops.luma` otherwise);
        `estimate_motion(luma, outliers='device', fit='device')`; `stabilize_resident(crop=True)` on the frames, `stabilized_nv12(crop=True)`,
        `stabilized_p010_cropped`, `stabilized_nv16_cropped` or `stabilized_p210_cropped` on the pair; the luma of the cropped clip in the same way; `cropping_and_distortion_resident(luma, cropped luma)`;
        `_compute_stability_score_device` on the stabilized vertex paths.  Returns (the cropped clip in the input's form,
        (cropping_ratio, distortion_score, stability_score)) -- the reference's order, mfs.py:169; the first two np.float32, the third a
        float.  Every ValueError of those calls is this one's."""
        import torch
        from . import online, ops
        form, luma = online.luma_of(clip, red_first)
        d_disp, homographies = self.estimate_motion(luma, chunk_pairs, max_per_subframe, outliers='device', fit='device')
        if form.pair:
            d_y, d_uv = clip
            deep = form.dtype == torch.uint16                  # (P010, P210: the tracker's luma is `ops.luma` of the plane)
            if form.fmt is ops._P010:
                out_y, out_uv, _ = self.stabilized_p010_cropped(d_y, d_uv, d_disp, homographies,
                                                                adaptive_weights_definition=adaptive_weights_definition)
            elif form.fmt is ops._P210:
                out_y, out_uv, _ = self.stabilized_p210_cropped(d_y, d_uv, d_disp, homographies,
                                                                adaptive_weights_definition=adaptive_weights_definition)
            elif form.fmt is ops._NV16:
                out_y, out_uv, _ = self.stabilized_nv16_cropped(d_y, d_uv, d_disp, homographies,
                                                                adaptive_weights_definition=adaptive_weights_definition)
            else:
                out_y, out_uv, _ = self.stabilized_nv12(d_y, d_uv, d_disp, homographies,
                                                        adaptive_weights_definition=adaptive_weights_definition, crop=True)
            # neither call hands out its paths; the sweep is deterministic, so a second one yields the same bytes
            d_stab = self._stabilized_vertex_displacements_device(d_disp, int(d_y.shape[2]), int(d_y.shape[1]), adaptive_weights_definition,
                                                                  homographies)
            cropped, cropped_luma = (out_y, out_uv), ops.luma(out_y) if deep else out_y
        else:
            _, _, d_stab, cropped = self.stabilize_resident(clip, d_disp, homographies, adaptive_weights_definition, crop=True)
            cropped_luma = cropped if luma is clip else ops.luma(cropped, red_first)
        cropping_ratio, distortion_score = self.cropping_and_distortion_resident(luma, cropped_luma, chunk_pairs, max_per_subframe)
        return cropped, (cropping_ratio, distortion_score, self._compute_stability_score_device(d_stab))

    def online_session(self, window=40, iters=10, beta=1.0, crop_margin=0.08, output_size=None,
                       adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, chunk_pairs=32, max_per_subframe=1024, red_first=False,
                       on_lost='hold', on_cut='ignore', cut_threshold=0.30, on_uncovered='report', limit_steps=32, limit_guard=2.0,
                       limit_rise=2, lag=0):
        """Stabilization of a stream whose end nobody has seen -- a capture card, a decoder's ring, a clip longer than HBM: an
        `online.OnlineSession` whose `push(frames)` takes one or more new frames in any form `stabilize_scored` takes and returns
        (those frames stabilized and cropped, in the input's form, `online.OnlineReport`) at once, with zero latency.  The reference has no
        such path; the arithmetic is the library's own (include/meshflow_hip.h, mf_online_smooth_f64; tests/online_model.py).
        Per push: `ops.luma` where the frames are not luma yet; the pairs (the previous push's last frame -> the first new one, then the
        adjacent new ones) through `device_tracker(max_per_subframe, 'device', 'device').track_stacks_resident(early, late, chunk_pairs)`;
        their velocities from `ops.vertex_motion` (its running sum is ignored: the smoother keeps its own across pushes); their weights from
        `host.adaptive_weights` on the homographies, which come down with the fit's record -- the one wait of a push beyond the tracker's
        own --; `ops.online_smooth` over a window of `window` frames (2 .. 64) that ends at each new frame, radius
        `temporal_smoothing_radius` (1 .. 64), `iters` sweeps, `beta` the pull towards the previous window's solution;
        `ops.cell_table(c, p, ...)`; the format's warp; the format's crop-resize to a FIXED rectangle: left = floor(crop_margin (W - 1)),
        right = (W - 1) - left, the same vertically (crop_margin in [0, 0.5), at least 2 x 2 pixels left, else ValueError; 0 returns the warp
        uncropped), scaled back to the frame size or to output_size = (width, height).  The report says per frame whether the rectangle
        was `covered`.  on_lost: a pair the tracker cannot fit is zero motion and listed in the report's `lost` ('hold'), or today's
        ValueError with the session unchanged ('raise').  `reset()` empties the session's memory at a cut.  on_cut: 'ignore' leaves cuts
        to the caller -- no launch, wait or byte differs from a session without the keyword --; 'reset' scores every push's frames first
        (`ops.find_cuts`: the tile-histogram distance of tests/cuts_model.py to the frame before, a cut where it exceeds
        floor(cut_threshold * 2 H W); cut_threshold a finite number in [0, 1], 0.30 by design, not tuned on footage), splits the block at
        every cut and calls `reset()` before each part that begins at one, so the pair across a cut is never tracked; the session's
        `last_cuts`, `last_cut_distances` and `shots` say what it found.  on_uncovered: 'report' leaves a frame whose warp does not cover
        the rectangle as it is, border colour and all, and says so in `covered` -- no launch, wait or byte differs from a session without
        the keyword --; 'limit' puts `ops.path_limit` (tests/path_limit_model.py) between the smoother and the cell table: the frame's
        correction p - c is scaled by k / limit_steps, k the largest step (of limit_steps, 1 .. 64) at which the mesh's perimeter encloses
        the rectangle widened by limit_guard pixels (finite, >= 0; 2 by CPU trials, profiles/path_limit.md), falling at once and rising by
        at most limit_rise (1 .. limit_steps) per frame.  The limited path is what is warped and what the report's `d_stab` holds; the
        smoother's own state keeps the unlimited one, so blocks still equal one push.  The session's `last_limit` is the last push's (n,)
        int32 k on the device; `reset()` and every cut found start k at limit_steps again.  With 'limit' a rectangle that leaves less
        than limit_guard + 1 pixels on its left or top is a ValueError at the first push: no correction would pass.  Frame size and form
        are fixed by the first push; a later mismatch is a ValueError.
        lag: frames of look-ahead, an int (no bool) in 0 .. window - 1, else ValueError.  0 is the zero-latency session above -- no launch,
        wait or byte differs from a session without the keyword.  With lag = k >= 1 a frame is handed out k frames after it was pushed,
        with the path value it has in the window that ends k frames after it (`ops.online_smooth_lag`, mf_online_smooth_lag_f64;
        tests/online_lag_model.py): on the model's 60-frame random walk five frames of latency halve the residual shake and shrink the
        correction by a quarter, and the gain saturates at about lag = temporal_smoothing_radius (profiles/online_lag.md; synthetic paths
        only, nobody has looked at footage).  `push` then returns the frames that have become final, session indices [emitted, seen - k) --
        possibly none: a 0-frame tensor (a pair for 4:2:0 and 4:2:2) of the output's dtype and trailing shape, and a report with 0-row tensors --;
        the report's `first`, d_unstab, d_stab and covered are those frames', `lost` stays that of the frames pushed, and the number of
        frames out is d_stab.shape[0].  The session keeps the at most k frames it still owes on the device as clones, both planes of a
        4:2:0 pair, so the caller's buffers are free when push returns; `pending` says how many.  `flush()` ends the stream: it returns
        (the pending frames, report) with the last window's solution as their path (`ops.online_pending`), through the same limiter, warp
        and crop, and leaves the session as `reset()` does; over push ... push, flush every pushed frame comes out exactly once, in
        order, and the joined bytes do not depend on the block sizes.  `reset()` DISCARDS pending frames.  on_cut='reset' flushes the old
        shot before the reset at each cut: its tail comes out of the same push, in front of the new shot's frames.  on_lost='raise'
        leaves held frames, `emitted` and the limiter's carry as they were.  The path limit runs on the frames handed out, carrying its
        step across them in order."""
        from . import online
        return online.OnlineSession(self, window, iters, beta, crop_margin, output_size, adaptive_weights_definition, chunk_pairs,
                                    max_per_subframe, red_first, on_lost, on_cut, cut_threshold, on_uncovered, limit_steps, limit_guard,
                                    limit_rise, lag)

    def online_group(self, streams, **keywords):
        """`streams` live streams of one frame size and form -- the cameras of one server -- stabilized together: an `online.OnlineGroup`
        whose `push(frames, streams=None)` takes ONE new frame of each of K distinct streams (a stack (K, ...) in any form a session
        takes, a (d_y, d_uv) pair of (K, ...) stacks for 4:2:0, NV16 and P210 (a packed 4:2:2 clip is no session form: callers unpack once per push); `streams` lists the K indices in any order and defaults to all) and
        returns (the K frames stabilized and cropped, [an `online.OnlineReport` per pushed stream]); row r and report r belong to
        streams[r].  The keywords are `online_session`'s and mean the same, except lag, which must be 0 (`online_lag_group` is the
        group with look-ahead), and on_lost, which must be 'hold' (one camera's lost pair must not stop the others; it is listed in that
        stream's `report.lost`): both are a ValueError otherwise.
        The contract: a stream gets the bytes that an `online_session` of its own with the same keywords returns when pushed the same
        frames one at a time -- frames, d_unstab, d_stab, covered, first, lost, the limiter's k, the cut decisions and distances, shots --
        in whatever grouping of ticks the frames arrive.  One push issues one set of launches whatever K is: `ops.luma` and the cut
        signatures once, the K distances in one wait (`ops.cut_distance_pairs`), the pairs (a stream's last luma -> its new frame) of
        every stream that has a frame before and no cut through the tracker, `ops.vertex_motion`, the one download and
        `host.adaptive_weights` together, then `ops.online_smooth_group`, `ops.path_limit_group`, one cell table, one warp, one
        crop-resize (profiles/online_group.md).  A stream at its first frame, after `reset(stream)` or at a cut found is not tracked and
        starts its path at frame 0.  The group's `seen` and `shots` are lists per stream; `last_limit`, `last_cuts` and
        `last_cut_distances` are per pushed row of the last push; `reset(stream=None)` forgets one stream or all."""
        from . import online
        return online.OnlineGroup(self, streams, **keywords)

    def online_lag_group(self, streams, lag, **keywords):
        """`online_group` with `lag` frames of look-ahead per stream: an `online.OnlineLagGroup`.  lag: an int (no bool) in
        1 .. window - 1 (0 is `online_group`); the keywords are `online_group`'s, on_lost='hold' only -- on_lost='raise' remains a keyword
        of sessions: one camera's lost pair must not stop the others.
        The contract is `online_group`'s against `online_session(lag=lag, **keywords)`: stream b gets, byte for byte, what a lagged session
        of its own returns when pushed the same frames one at a time -- frames, d_unstab, d_stab, covered, first, lost, the limiter's k,
        the cut decisions and distances, shots, and `pending`.  `push(frames, streams=None)` takes one new frame of each of K distinct
        streams and returns (the frames handed out this tick, concatenated in row order, [an `online.OnlineReport` per pushed row]): a row
        hands out the frame its stream was pushed `lag` frames of its own earlier, none while the stream has no more than `lag` frames,
        and `last_counts[r]` says how many frames of the output are row r's.  `lost` is reported at the tick of the push.  With
        on_cut='reset' a stream found at a cut hands out its old shot's tail in that tick, in front, and starts again.
        `flush(stream=None)` ends one stream or all: (the pending frames with the last window's solution as their path, a report per
        named stream), then `reset(stream)`; `reset` DISCARDS pending frames.  `pending` is a list per stream.
        A steady tick issues `online_group`'s launches with `ops.online_smooth_group_lag` as the smoother, plus one `ops.ring_exchange`
        per plane, which stores the K new frames in a ring on the device and hands out the owed ones (profiles/online_group_lag.md);
        the limiter, the cell table, the warp and the crop-resize run on the rows that hand a frame out.
        Memory: the ring holds streams * lag frames per plane of the clip form on the device, allocated at the first push (16 streams of
        1080p BGR at lag 5: 498 MB); a ValueError names the size if it cannot be had."""
        from . import online
        return online.OnlineLagGroup(self, streams, lag, **keywords)

    def find_cuts(self, clip, threshold=0.30, red_first=False):
        """Where the shots of a resident clip begin: the list of frame indices t in 1 .. F-1 whose tile-histogram distance to frame t - 1
        (`ops.find_cuts`, tests/cuts_model.py) exceeds floor(threshold * 2 H W).  `clip` in any form `stabilize_scored` takes; its luma comes
        the way a session's does (`online.luma_of`; red_first: RGB / RGBA).  threshold: a finite number in [0, 1], 0.30 by design, not
        tuned on footage; at 1.0 nothing is a cut.  For splitting a clip before `estimate_motion` / `stabilize_scored`, which track across
        a cut like across any pair."""
        from . import online, ops
        threshold = ops.check_cut_threshold(threshold)
        if red_first not in (False, True):
            raise ValueError(f'red_first must be False or True (got {red_first!r})')
        _, luma = online.luma_of(clip, red_first)
        return ops.find_cuts(luma, threshold)[0]

    def stabilize_online(self, clip, **session):
        """One `online_session(**session)` and one push of the whole clip: (stabilized and cropped clip, `online.OnlineReport`).  With
        lag >= 1 the push and the `flush()` behind it, joined: still the whole clip."""
        session = self.online_session(**session)
        result = session.push(clip)
        if session.lag:
            result = session.join([result, session.flush()])
        return result

    def _write_stabilized_video(self, output_path, num_frames, frames_per_second, codec, stabilized_frames):
        """mfs.py:1290-1322."""
        from . import frontend_cv2
        frontend_cv2.write_video(frontend_cv2.require_cv2(), output_path, frames_per_second, codec,
                                 stabilized_frames[:num_frames])

    def stabilize_clip(self, unstabilized_frames, vertex_unstabilized_displacements_by_frame_index, homographies,
                       adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, crop=False,
                       keep_uncropped=True, chunk_frames=16, io_threads=3, output_size=None):
        """The hot path of `stabilize` (mfs.py:150-159, 162) on in-memory inputs, with ONE host->device and ONE
        device->host pass over the frames (the two private methods below each pay their own, like any drop-in
        for NumPy-in / NumPy-out methods must).  The passes are chunked and overlapped with each other and with
        the kernels below Python (csrc/hostpipe.hip): each 16-frame chunk is warped as soon as it has landed and
        comes back while later chunks are still going up.  (`chunk_frames` / `io_threads` are kept for callers of
        earlier versions; the C pipeline has its own, MF_PIPE_* in the environment.)

        Returns (stabilized_frames list, crop_boundaries, vertex_stabilized_displacements, stability_score)
        and, with crop=True, a fifth item: the cropped + resized frames (`_crop_frames`, mfs.py:159), produced
        on the device from the stabilized frames in the same pipeline once the clip-level rectangle is known
        (`mf_warp_crop_u8c3_host_frames`); keep_uncropped=False then never brings the uncropped stabilized frames back
        (the reference only uses the cropped ones afterwards) and returns None for them.  output_size=(width, height) (cv2.resize's
        dsize order; needs crop=True) makes the fifth item the crop resized to that size instead of (W, H)
        (`mf_warp_crop_to_u8c3_host_frames`); bounds, vertex paths and stability score do not change."""
        import torch
        from . import ops, pipeline
        self._check_definition(adaptive_weights_definition)
        if output_size is not None:
            if not crop:
                raise ValueError('output_size needs crop=True: it is the size of the cropped frames')
            output_size = ops.check_output_size(output_size, 'output_size')
        if chunk_frames != 16 or io_threads != 3:
            import warnings
            warnings.warn('stabilize_clip: chunk_frames / io_threads are ignored since the frames travel through the C pipeline '
                          '(csrc/hostpipe.hip); tune it with MF_PIPE_CHUNK / MF_PIPE_UP / MF_PIPE_DOWN in the environment', DeprecationWarning, stacklevel=2)
        num_frames = len(unstabilized_frames)
        dev = self._torch_device()
        unstab = np.ascontiguousarray(vertex_unstabilized_displacements_by_frame_index, dtype=np.float64)
        self._check_mesh_shape(unstab, num_frames)
        clip = pipeline.HostClip(unstabilized_frames, num_frames)
        H, W = clip.height, clip.width
        # the frames travel through the C ABI's own pipeline (no Python threads, GIL released): up in chunks, warped as they land,
        # and -- crop=True -- cropped + resized on the device once the clip-level rectangle is known, only then back
        d_stab = self._stabilized_vertex_displacements_device(torch.from_numpy(unstab).to(dev), W, H,
                                                              adaptive_weights_definition, homographies)
        stab = d_stab.cpu().numpy()
        # the stability score (mfs.py:162: np.fft over every vertex path, 20 ms at config 3) on a host thread BESIDE the frames' trip over
        # PCIe (the C call releases the GIL): same function, same bits, off the critical path
        import threading
        score = {}

        def scoring():
            try:
                score['value'] = self._compute_stability_score(num_frames, stab)
            except BaseException as e:          # re-raised on the calling thread
                score['error'] = e
        scorer = threading.Thread(target=scoring, name='mf-score')
        scorer.start()
        try:
            res = _warp_host_c(self, clip, unstab, stab, crop=crop, keep_uncropped=keep_uncropped, output_size=output_size)
        finally:
            scorer.join()
        if 'error' in score:
            raise score['error']
        if not crop:
            out_host, bounds = res
            return list(out_host), bounds, stab, score['value']
        out_host, bounds, cropped_host = res
        return (list(out_host) if out_host is not None else None), bounds, stab, score['value'], list(cropped_host)

    # ------------------------------------------------------------------------------------------
    # drop-in boundary, host buffers (same signatures as the reference)
    # ------------------------------------------------------------------------------------------

    def _torch_device(self):
        return _torch_device_of(self)

    def _get_stabilized_vertex_displacements(self, num_frames, unstabilized_frames, adaptive_weights_definition,
                                             vertex_unstabilized_displacements_by_frame_index, homographies):
        """mfs.py:632-710.  float64 (F, R+1, C+1, 2) in, float64 (F, R+1, C+1, 2) out."""
        import torch
        disp = np.ascontiguousarray(vertex_unstabilized_displacements_by_frame_index, dtype=np.float64)
        self._check_mesh_shape(disp, num_frames)
        frame_height, frame_width = unstabilized_frames[0].shape[:2]                       # mfs.py:679
        dev = self._torch_device()
        d_disp = torch.from_numpy(disp).to(dev)
        d_stab = self._stabilized_vertex_displacements_device(d_disp, frame_width, frame_height,
                                                              adaptive_weights_definition, homographies)
        return d_stab.cpu().numpy()

    def _get_stabilized_frames_and_crop_boundaries(self, num_frames, unstabilized_frames,
                                                   vertex_unstabilized_displacements_by_frame_index,
                                                   vertex_stabilized_displacements_by_frame_index,
                                                   chunk_frames=16, io_threads=3):
        """mfs.py:909-1108.  Returns (list of F uint8 (H, W, 3) arrays, (left, top, right, bottom)).
        (`chunk_frames` / `io_threads` are kept for callers of earlier versions; the C pipeline has its own.)"""
        from . import pipeline
        unstab = np.ascontiguousarray(vertex_unstabilized_displacements_by_frame_index, dtype=np.float64)
        stab = np.ascontiguousarray(vertex_stabilized_displacements_by_frame_index, dtype=np.float64)
        self._check_mesh_shape(unstab, num_frames)
        self._check_mesh_shape(stab, num_frames)
        clip = pipeline.HostClip(unstabilized_frames, num_frames)
        out_host, bounds = _warp_host_c(self, clip, unstab, stab)
        return list(out_host), bounds

    def _get_unstabilized_vertex_displacements_from_features(self, num_frames, frame_width, frame_height,
                                                             features_by_pair, homographies):
        """mfs.py:236-284 with the tracker's outputs injected: `features_by_pair[t]` = (early_features,
        late_features) of frames t, t+1 as `_get_matched_features_and_homography` returns them (mfs.py:455-528),
        `homographies` (F, 3, 3) with the identity last (mfs.py:274).  Returns the reference's tuple
        (vertex_unstabilized_displacements_by_frame_index float64 (F, R+1, C+1, 2), homographies)."""
        disp, _ = self._vertex_motion_from_features(num_frames, frame_width, frame_height, features_by_pair, homographies)
        return disp, np.asarray(homographies, dtype=np.float64)

    def _get_unstabilized_vertex_velocities_from_features(self, frame_width, frame_height, early_features,
                                                          late_features, early_to_late_homography):
        """mfs.py:287-362 after the tracker call at :316: float32 (R+1, C+1, 2) velocities of one frame pair."""
        hom = np.asarray(early_to_late_homography, dtype=np.float64).reshape(1, 3, 3)
        _, vel = self._vertex_motion_from_features(2, frame_width, frame_height, [(early_features, late_features)], hom)
        return vel[0]

    def _vertex_motion_from_features(self, num_frames, frame_width, frame_height, features_by_pair, homographies):
        import torch
        from . import ops
        if len(features_by_pair) != num_frames - 1:
            raise ValueError('features_by_pair must hold num_frames - 1 (early, late) pairs')
        hom = np.ascontiguousarray(np.asarray(homographies, dtype=np.float64)[:num_frames - 1]).reshape(-1, 3, 3)
        if hom.shape[0] != num_frames - 1:
            raise ValueError('homographies must hold at least num_frames - 1 matrices')
        early, late, offsets, kmax = host.pack_features(features_by_pair)
        dev = self._torch_device()
        d_disp, d_vel, status = ops.vertex_motion(
            torch.from_numpy(early).to(dev), torch.from_numpy(late).to(dev), torch.from_numpy(offsets).to(dev),
            torch.from_numpy(hom).to(dev), kmax, frame_width, frame_height, self.mesh_row_count, self.mesh_col_count,
            self.feature_ellipse_row_count, self.feature_ellipse_col_count)
        ops.vertex_motion_check(status)
        return d_disp.cpu().numpy(), d_vel.cpu().numpy()

    def _crop_frames(self, uncropped_frames, crop_boundaries, chunk_frames=16, io_threads=3, output_size=None):
        """mfs.py:1111-1157: crop to the inclusive bounds and resize back to (W, H) (cv2.resize, INTER_LINEAR).
        Host frames in, host frames out through the C ABI's ring of chunk buffers (`mf_crop_resize_u8c3_host_frames`,
        csrc/hostpipe.hip): upload, resize and download of the chunks all overlap, below Python.
        output_size=(width, height) (cv2.resize's dsize order) resizes to that size instead: cv2.resize(crop, output_size)
        (`mf_crop_resize_to_u8c3_host_frames`).
        (`chunk_frames` / `io_threads` are kept for callers of earlier versions; the C pipeline has its own, MF_PIPE_*.)"""
        import ctypes
        import torch
        from . import _lib, ops, pipeline
        if output_size is not None:
            output_size = ops.check_output_size(output_size, 'output_size')
        dev = _torch_device_of(self)
        n = len(uncropped_frames)
        clip = pipeline.HostClip(uncropped_frames, n)
        H, W = clip.height, clip.width
        frames = [clip.array[i] for i in range(n)] if clip.array is not None else clip.frames       # (every frame validated by HostClip)
        left, top, right, bottom = (int(v) for v in crop_boundaries)
        oW, oH = output_size if output_size is not None else (W, H)
        out = np.empty((n, oH, oW) + clip.frame_shape[2:], dtype=np.uint8)
        fb = oH * oW * clip.channels
        pin = (ctypes.c_void_p * n)(*[f.ctypes.data for f in frames])
        pout = (ctypes.c_void_p * n)(*[out.ctypes.data + i * fb for i in range(n)])
        with torch.cuda.device(dev):
            if output_size is None:
                _lib.check(getattr(_lib.lib, _HOST_CALLS[clip.channels][2])(pin, pout, n, W, H, left, top, right, bottom, None))
            else:
                _lib.check(getattr(_lib.lib, _HOST_CALLS[clip.channels][4])(pin, pout, n, W, H, left, top, right, bottom, oW, oH, None))
        return list(out)

    def compute_scores(self, frame_width, frame_height, vertex_unstabilized_displacements_by_frame_index,
                       vertex_stabilized_displacements_by_frame_index, crop_boundaries):
        """(cropping_ratio, distortion_score, stability_score) in the order `stabilize` returns them (mfs.py:169).
        stability_score is the reference's own formula (mfs.py:1216-1259); the other two are computed from the
        mesh correspondences instead of tracked features -- see host.mesh_cropping_ratio_and_distortion."""
        ratio, distortion = host.mesh_cropping_ratio_and_distortion(
            frame_width, frame_height, self.mesh_row_count, self.mesh_col_count,
            vertex_unstabilized_displacements_by_frame_index, vertex_stabilized_displacements_by_frame_index,
            crop_boundaries)
        stab = np.asarray(vertex_stabilized_displacements_by_frame_index)
        return ratio, distortion, self._compute_stability_score(stab.shape[0], stab)

    def _compute_stability_score(self, num_frames, vertex_stabilized_displacements_by_frame_index):
        """mfs.py:1216-1259."""
        return host.stability_score(np.asarray(vertex_stabilized_displacements_by_frame_index))

    def _compute_stability_score_device(self, d_stab):
        """mfs.py:1216-1259 on device-resident paths (five direct DFT bins + Parseval; float64 rounding apart from
        `_compute_stability_score`, which stays the bit-for-bit restatement of the reference's np.fft formulation)."""
        from . import ops
        score, _ = ops.stability_score(d_stab)
        return float(score.item())

    def _get_vertex_x_y(self, frame_width, frame_height):
        """mfs.py:881-906."""
        return host.vertex_x_y(frame_width, frame_height, self.mesh_row_count, self.mesh_col_count)

    # ------------------------------------------------------------------------------------------
    # device-resident variants (torch tensors in HBM)
    # ------------------------------------------------------------------------------------------

    def _check_mesh_shape(self, disp, num_frames):
        want = (num_frames, self.mesh_row_count + 1, self.mesh_col_count + 1, 2)
        if tuple(disp.shape) != want:
            raise ValueError(f'vertex displacements must have shape {want}, got {tuple(disp.shape)}')

    def _jacobi_coefficients_device(self, num_frames, frame_width, frame_height, adaptive_weights_definition,
                                    homographies, device):
        """Band coefficients (host, O(F): mfs.py:713-841 restated in host.py) -> device.  The upload goes through a
        small ring of pinned buffers with a non-blocking copy: a pageable copy would wait for everything already
        queued on the stream, i.e. serialise this host work with the previous clip's kernels."""
        import torch
        taps, lam, inv_on = host.jacobi_band_coefficients(
            num_frames, frame_width, frame_height, adaptive_weights_definition,
            np.asarray(homographies, dtype=np.float64), self.temporal_smoothing_radius)
        nt = taps.size
        total = nt + 2 * num_frames
        ring = getattr(self, '_coef_ring', None)
        if ring is None or ring['size'] != total or ring['device'] != device:
            ring = {'size': total, 'device': device, 'next': 0,
                    'slots': [(torch.empty(total, dtype=torch.float64).pin_memory(), torch.cuda.Event()) for _ in range(4)]}
            self._coef_ring = ring
        staging, done = ring['slots'][ring['next']]
        ring['next'] = (ring['next'] + 1) % len(ring['slots'])
        done.synchronize()                                   # the copy that last used this slot (long finished)
        view = staging.numpy()
        view[:nt] = taps
        view[nt:nt + num_frames] = lam
        view[nt + num_frames:] = inv_on
        packed = torch.empty(total, dtype=torch.float64, device=device)
        packed.copy_(staging, non_blocking=True)
        done.record(torch.cuda.current_stream(device))
        return packed[:nt], packed[nt:nt + num_frames], packed[nt + num_frames:]

    def _stabilized_vertex_displacements_device(self, d_disp, frame_width, frame_height,
                                                adaptive_weights_definition, homographies):
        """d_disp: (F, R+1, C+1, 2) float64 device tensor -> same shape, stabilized."""
        from . import ops
        F = d_disp.shape[0]
        taps, lam, inv_on = self._jacobi_coefficients_device(F, frame_width, frame_height,
                                                             adaptive_weights_definition, homographies, d_disp.device)
        x = ops.jacobi(d_disp.reshape(F, -1), taps, lam, inv_on, self.temporal_smoothing_radius,
                       self.optimization_num_iterations)
        return x.view(d_disp.shape)

    # ---- the device-resident pipeline ----

    # How a resident clip is issued (measured on MI355X):
    #   0  (default) IN ORDER: cell table + plan, then the warp ALONE, on the caller's stream; only the Jacobi sweep goes to the prep
    #      stream, gated so that the NEXT clip's sweep runs beside THIS clip's table + plan (both leave most of the chip idle) and has
    #      ended when the warp starts.  Kernels that run beside the warp kernel cost it more than they take by themselves.
    #   k >= 1: the clip cut into k frame ranges, tables + crop scan + rectangle on the prep stream BESIDE the warp (warp(j) waits for
    #      table(j) only): the rectangle is known earliest; at the round-6 kernels a config-2 clip takes 1.88 ms this way against 1.19 (the
    #      side kernels are the YOUNGER wavefronts beside the warp -- cell table 273 us instead of 16, plan 468 instead of 70 -- and the
    #      stand-alone crop scan repeats the coordinate arithmetic; it was 2-8 % in round 4, before the in-order path lost a third of its time).
    resident_chunks = 0
    resident_rectangle = 'fused'     # 'early': rectangle from the table on the prep stream (a sharded run's all-reduce hides behind the warp)
    # What the NEXT clip's sweep (prep stream) waits for.  'table': this clip has reached its cell table -- a short sweep (config 2: 48 us)
    # then runs beside cell table + plan (~100 us, both leave most of the chip idle) and nothing runs beside the warp.  'plan': this clip's
    # plan has ended -- a LONG sweep (config 3: 0.65 ms of float64 FMAs on every SIMD) beside cell table + plan makes those take 0.7 + 0.4 ms
    # instead of 0.05 + 0.2; beside the first part of the warp it costs the warp what it takes itself, and the step is 7.5 % shorter
    # (3.73 -> 3.45 ms; config 2: 1.277 -> 1.269).  'auto': 'plan' from 4 GFLOP of sweep on.
    resident_gate = 'auto'
    resident_table_shapes = 4        # cell tables are kept for this many (W, H, mesh) geometries (two tables each, grow-only in the clip length)

    def _resident_state(self, dev):
        """Per-device plumbing of `stabilize_resident`: the PREP stream beside the caller's, a stream for the 4-byte status read-backs,
        two cell tables per clip geometry taking turns, the event after which a table is free again, and the gate of the next sweep."""
        import collections
        import torch
        st = getattr(self, '_resident', None)
        if st is None or st['device'] != dev:
            if st is not None:                               # another device: nothing of the old one's is kept
                self.finish()
            st = {'device': dev, 'prep': torch.cuda.Stream(device=dev), 'status': torch.cuda.Stream(device=dev),
                  'tables': collections.OrderedDict(), 'turn': 0, 'ends': [], 'serial': 0}
            self._resident = st
        return st

    @staticmethod
    def _settle(slot):
        """The degenerate-mesh verdict of the clip that last used this table slot: waits for its 4-byte status read-back (issued behind
        that clip's warp on a stream of its own -- long finished when the slot comes up again two clips later) and raises if the clip had
        cells without a homography.  The counter is cumulative per table; a slot remembers what it has seen.  A clip issued with crop=True
        brings its crop's status word along in the same read-back (the slot's second word): an unusable rectangle raises
        UnusableCropError -- after the mesh verdict, which explains it more often than not."""
        pending, slot['pending'] = slot['pending'], None
        if pending is None:
            return
        pending['copied'].synchronize()
        total, crops = int(slot['host'][0]), int(slot['host'][1])
        bad, slot['seen'] = total - slot['seen'], total
        empty, slot['crop_seen'] = crops - slot['crop_seen'], crops
        if bad and not pending['ignore']:
            raise DegenerateMeshError(bad, pending['serial'])
        if empty and not pending['ignore']:
            raise UnusableCropError(pending['serial'])

    def finish(self):
        """Waits for the verdict of every clip `stabilize_resident` has issued and not yet checked (it checks clip i when clip i + 2 is
        issued) and raises ValueError for the first one that had a degenerate mesh.  Later clips are unaffected either way."""
        st = getattr(self, '_resident', None)
        first = None
        if st is not None:
            for pair in st['tables'].values():
                for slot in pair:
                    try:
                        self._settle(slot)
                    except ValueError as e:
                        first = first or e
        if first is not None:
            raise first

    @property
    def resident_serial(self):
        """Serial number of the clip the last `stabilize_resident` call issued (what `DegenerateMeshError.clip_serial` names)."""
        st = getattr(self, '_resident', None)
        return 0 if st is None else st['serial']

    def _settle_upcoming(self, st, W, H):
        """The verdict of the clip whose table slot the NEXT clip of this geometry takes -- looked at before ANYTHING of the new clip is
        queued (its sweep included), so that a deferred DegenerateMeshError leaves no half-issued clip behind."""
        pair = st['tables'].get((W, H, self.mesh_row_count, self.mesh_col_count))
        if pair is not None:
            self._settle(pair[st['turn'] & 1])

    def _resident_slot(self, st, n, W, H):
        """The table slot of the next clip (two per geometry take turns), settled and sized for n frames."""
        import torch
        from . import ops
        dev = st['device']
        key = (W, H, self.mesh_row_count, self.mesh_col_count)
        pair = st['tables'].get(key)
        if pair is None:
            while len(st['tables']) >= max(1, self.resident_table_shapes):           # least recently used geometry out (its verdicts first)
                _, old = next(iter(st['tables'].items()))
                for slot in old:
                    self._settle(slot)
                torch.cuda.synchronize(dev)
                st['tables'].popitem(last=False)
            pair = st['tables'][key] = [{'table': ops.CellTable(n, W, H, self.mesh_row_count, self.mesh_col_count, dev), 'free': None,
                                         'pending': None, 'seen': 0, 'host': torch.zeros(2, dtype=torch.int32).pin_memory(),
                                         # (crop=True: the slot's count of unusable crop rectangles, cumulative like the table's status;
                                         # made by the first clip that crops, so that crop=False launches what it always did)
                                         'crop_status': None, 'crop_seen': 0} for _ in range(2)]
        st['tables'].move_to_end(key)
        slot = pair[st['turn'] & 1]
        self._settle(slot)                                   # (raises BEFORE anything of the new clip is issued or any state changes)
        if n > slot['table'].capacity:
            torch.cuda.synchronize(dev)                      # a longer clip than this slot has seen: its buffers are replaced (rare)
        slot['table'].resize(n)
        st['turn'] += 1
        return slot

    def _sweep_gate(self, d_disp):
        if self.resident_gate != 'auto':
            return self.resident_gate
        flops = float(self.optimization_num_iterations) * d_disp.shape[0] * (d_disp.numel() // d_disp.shape[0]) * (4 * self.temporal_smoothing_radius + 5)
        return 'plan' if flops >= 4e9 else 'table'

    def _resident_jacobi(self, d_disp, frame_width, frame_height, adaptive_weights_definition, homographies, inputs_ready=None):
        """Stage 1 of the resident pipeline, on the prep stream: mfs.py:632-710.  `inputs_ready`: a torch.cuda.Event after which
        d_disp (and the frames) are valid, or None = whatever is queued on the current stream right now (safe, but then this clip's
        sweep cannot start before the previous clip's warp has ended).  In-order mode gates the sweep on the previous clip having
        reached its cell table (= the warp before it has ended): it then runs beside that table + plan, not beside a warp."""
        import torch
        dev = d_disp.device
        st = self._resident_state(dev)
        prep = st['prep']
        if inputs_ready is None:
            inputs_ready = torch.cuda.Event()
            inputs_ready.record(torch.cuda.current_stream(dev))
        prep.wait_event(inputs_ready)
        # The gate is for sweeps of one wavefront per series (clips of up to 64 K frames: config 2's 47 us fit under cell table + plan,
        # config 3's 0.8 ms start there).  A longer clip spreads each series over 2-8 wavefronts with up to 40 KB of LDS per workgroup
        # (the replicated sweep of an N-GPU job): gated, it runs on into the warp and crowds it out of the CUs (rehearsal of a rank of 8:
        # 1.68 ms per step against 1.54 in order); left ungated, the queued sweeps of several clips fill the chip together (1.48).
        radius = self.temporal_smoothing_radius
        one_wave = d_disp.shape[0] <= 64 * (5 if radius <= 12 else 8 if radius <= 20 else 10)
        gate = self._sweep_gate(d_disp)
        st['gate'] = gate
        if self.resident_chunks <= 0 and one_wave and gate == 'plan' and st.get('planned') is not None:
            prep.wait_event(st['planned'])        # the previous clip's cell table + plan have ended: a LONG sweep runs beside its warp
        elif self.resident_chunks <= 0 and one_wave and len(st['ends']) >= 2:
            prep.wait_event(st['ends'][-2])       # the warp two clips back has ended = the previous clip has reached its cell table
        with torch.cuda.stream(prep):
            d_stab = self._stabilized_vertex_displacements_device(d_disp, frame_width, frame_height, adaptive_weights_definition, homographies)
            st['swept'] = torch.cuda.Event()
            st['swept'].record(prep)
        d_stab.record_stream(torch.cuda.current_stream(dev))      # allocated on the prep stream, handed to the caller's
        return d_stab

    def _resident_warp(self, d_frames, d_unstab, d_stab, out=None, chunks=None, warp_events=None, check='deferred', verdict=True):
        """Stages 2-4, mfs.py:909-1108, for the d_stab `_resident_jacobi` just produced.  Returns (stabilized frames, bounds, table):
        bounds = the clip-level rectangle in a 16-byte tensor of this clip's own (the kernels fold it together there), table.crop per
        frame (valid until the table's next turn, two clips on).
        verdict=False leaves the status read-back to the caller, who issues it behind the crop (`_resident_verdict` with the returned
        st['open'] = (slot, end event)).
        warp_events: two torch events recorded on the current stream in front of and behind the warp kernel(s) (bench.py's roofline)."""
        import torch
        from . import ops
        dev = d_frames.device
        st = self._resident_state(dev)
        main = torch.cuda.current_stream(dev)
        chunks = self.resident_chunks if chunks is None else chunks
        n, H, W = d_frames.shape[:3]
        if n == 0:
            # an EMPTY shard (a clip of fewer frames than ranks, or the tail of an uneven split): nothing to warp; the rectangle's
            # neutral element (mfs.py:992-995), so that the rank still takes part in the all-reduce, and d_stab in stream order
            if st.get('swept') is not None:
                main.wait_event(st['swept'])
            bounds = torch.tensor([0, 0, W - 1, H - 1], dtype=torch.int32, device=dev)
            if self.resident_rectangle == 'early':
                st['scanned'] = torch.cuda.Event()
                st['scanned'].record(main)
            return (out if out is not None else d_frames.new_empty(tuple(d_frames.shape))), bounds, None
        slot = self._resident_slot(st, n, W, H)
        table = slot['table']
        bounds = torch.empty(4, dtype=torch.int32, device=dev)           # this clip's own: never rewritten by a later one
        if chunks <= 0:
            if st.get('swept') is not None:
                main.wait_event(st['swept'])                      # the sweep that produced d_stab
            # (every marker on a stream costs the step ~5 us -- DESIGN.md section 5 -- so ONE event per clip, recorded behind its warp,
            # serves as the end of a timed interval, as "this table is free again", as the start of the status read-back and, two clips
            # on, as the gate of a sweep)
            # (the same launches as mf_warp_clip_u8c3 with chunks = 0, issued from here so that the warp kernel can be bracketed)
            ops.cell_table(d_unstab, d_stab, W, H, self.mesh_row_count, self.mesh_col_count, table=table, reset_status=False, bounds=bounds)
            if st.get('gate') == 'plan':
                st['planned'] = torch.cuda.Event()
                st['planned'].record(main)
            early = self.resident_rectangle == 'early'
            if early:                                             # rectangle from the table, on the prep stream, beside the start of the warp
                tabled = torch.cuda.Event()
                tabled.record(main)
                st['prep'].wait_event(tabled)
                with torch.cuda.stream(st['prep']):
                    ops.crop_scan(table, bounds=bounds)           # (the scan folds the clip-level rectangle together as well)
                    scanned = torch.cuda.Event()
                    scanned.record(st['prep'])
                st['scanned'] = scanned
            if warp_events:
                warp_events[0].record(main)
            out = ops.warp(d_frames, table, self.color_outside_image_area_bgr, out=out, bounds=bounds)
            end = warp_events[1] if warp_events else torch.cuda.Event()
            end.record(main)
            st['ends'].append(end)
            del st['ends'][:-2]
        else:
            if slot['free'] is not None:
                st['prep'].wait_event(slot['free'])               # the warps that last read this table (two clips ago) have ended
            if warp_events:
                warp_events[0].record(main)
            out, _ = ops.warp_clip(d_frames, d_unstab, d_stab, table, self.color_outside_image_area_bgr, out=out,
                                   chunks=chunks, prep_stream=st['prep'], bounds=bounds)
            end = warp_events[1] if warp_events else torch.cuda.Event()
            end.record(main)
        slot['free'] = end
        st['open'] = (slot, end)
        if verdict:
            self._resident_verdict(st, check)
        return out, bounds, table

    def _resident_verdict(self, st, check, cropped=False):
        """Issues the status read-back of the clip `_resident_warp` has just queued (behind its warp; cropped=True: behind whatever is on
        the current stream now, i.e. the clip's crop, whose status word then rides along) and, under check=True, waits for it."""
        import torch
        slot, end = st.pop('open')
        table = slot['table']
        if cropped:
            end = torch.cuda.Event()
            end.record(torch.cuda.current_stream(st['device']))
        # the degenerate-cell counter of this clip, 4 bytes into pinned memory on a stream of their own behind the warp: no marker on
        # the caller's stream, nobody waits -- `_settle` looks at it when this slot comes up again (or `finish()` does); check='never'
        # only keeps the slot's running total in step
        ss = st['status']
        ss.wait_event(end)
        with torch.cuda.stream(ss):
            slot['host'][:1].copy_(table.status, non_blocking=True)
            if cropped:
                slot['host'][1:].copy_(slot['crop_status'], non_blocking=True)
            copied = torch.cuda.Event()
            copied.record(ss)
        st['serial'] += 1
        slot['pending'] = {'copied': copied, 'serial': st['serial'], 'ignore': check == 'never' or check is False}
        if check is True or check == 'now':
            self._settle(slot)

    def stabilize_resident(self, d_frames, d_disp, homographies, adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL,
                           out=None, frame_range=None, inputs_ready=None, check=True, collective=False, warp_events=None,
                           jacobi_events=None, crop=False, output_size=None, cropped_out=None):
        """mfs.py:150-158 (crop=True: mfs.py:150-162, `_crop_frames` included) for a clip whose frames (n, H, W, 3) uint8 or uint16 -- or (n, H, W) uint8 grey, or (n, H, W, 4) uint8 BGRA / RGBA
        -- and vertex displacements (F, R+1, C+1, 2) float64 are RESIDENT in HBM (uint16, grey and 4-channel frames: `ops.warp`; the sweep,
        tables and rectangle are the uint8 call's; 4-channel frames get alpha 0 where the warp uncovers the frame, the 3-component
        color_outside_image_area_bgr padded as cv::Scalar pads it): Jacobi sweep -> cell tables -> warp + crop rectangle, nothing leaves the device, one call per clip, NO synchronisation:
        calls issued back to back pipeline by themselves (the sweep runs on this object's prep stream, the next clip's beside this
        clip's cell table + plan; see `resident_chunks` for the other arrangement).
        frame_range = (lo, hi): d_frames holds frames lo..hi-1 of the clip (a frame-range shard; the sweep still covers all F);
        collective=True then all-reduces the rectangle over the process group (16 bytes, `dist.allreduce_crop`).
        Returns (stabilized frames, clip-level crop bounds as a device int32 tensor {left, top, right, bottom} -- 16 bytes of this
        clip's own, never rewritten by a later call --, stabilized vertex displacements (F, R+1, C+1, 2)), all valid in current-stream
        order.
        A degenerate mesh (a cell without homography: the reference dies inside cv2) raises `DegenerateMeshError` (a ValueError) that
        carries the clip's serial number (`resident_serial` right after the call that issued it).  check=True (the default, like the
        reference: the error belongs to THIS call) waits for the clip's 4-byte verdict before returning -- one blocking device-to-host
        read per clip, so the calls no longer overlap.  A pipelined caller (bench.py's timed step) passes check='deferred': the verdict
        of clip i is then looked at when clip i + 2 is issued (its table slot comes up again; BEFORE anything of the new clip is queued,
        which is then not issued) or by `finish()`, whichever comes first -- such a caller MUST end with `finish()`.  check='never'
        skips it.  Clips after a degenerate one are unaffected.
        crop=True adds the reference's last step, `_crop_frames` (mfs.py:159, 1111-1157), on the device: the frames cropped to the
        clip-level rectangle and scaled back to (W, H) -- or to output_size=(width, height), cv2.resize's dsize order, which needs
        crop=True -- by kernels that read the rectangle from `bounds` themselves (`ops.crop_resize_resident`): the host never learns it and
        never waits for it.  The call then returns (frames, bounds, d_stab, cropped); `cropped` (cropped_out if given: (n, height, width
        [, channels]) of the frames' dtype) is valid in current-stream order.  With frame_range and collective=True the crop uses the
        all-reduced rectangle.  A rectangle that cannot be used (empty: the stabilised frames share no covered area; cv2.resize would
        fail on an empty source) leaves `cropped` unwritten and is reported like a degenerate mesh, by the same read-back: `UnusableCropError`
        (a ValueError with the clip's serial number) from this call under check=True, two clips later or from `finish()` under
        check='deferred', never under check='never'.  crop=False (the default) is the call as it always was: the same 3-tuple, the same
        launches.
        warp_events / jacobi_events: pairs of torch events recorded around the warp kernel (caller's stream) and the sweep stage (prep
        stream) -- bench.py's roofline brackets.
        One host thread per stabilizer object here: the calls of a pipeline are ordered by construction (table slots take turns, the
        deferred verdicts are kept per slot); threads that want their own pipelines take their own objects (the host-memory methods,
        `stabilize_clip` and the drop-in pair, may be called from several threads on one object: tests/test_gpu_stabilize_api.py)."""
        import torch
        from . import dist as mfdist, ops
        self._check_definition(adaptive_weights_definition)
        if output_size is not None:
            if not crop:
                raise ValueError('output_size needs crop=True: it is the size of the cropped frames')
            output_size = ops.check_output_size(output_size, 'output_size')
        if cropped_out is not None and not crop:
            raise ValueError('cropped_out needs crop=True')
        if check is False:
            check = 'never'
        F = d_disp.shape[0]
        lo, hi = frame_range if frame_range is not None else (0, F)
        ops.pixel_format(d_frames.dtype, d_frames.shape)
        n, H, W = d_frames.shape[:3]
        if hi - lo != n:
            raise ValueError(f'frame_range {lo, hi} does not match {n} frames')
        dev = d_frames.device
        st = self._resident_state(dev)
        if n > 0:
            self._settle_upcoming(st, W, H)              # (a deferred verdict is raised here: nothing of this clip has been queued yet)

        def jacobi_fn():
            if jacobi_events:
                jacobi_events[0].record(st['prep'])
            d_stab = self._resident_jacobi(d_disp, W, H, adaptive_weights_definition, homographies, inputs_ready)
            if jacobi_events:
                jacobi_events[1].record(st['prep'])
            return d_stab

        def warp_fn(lo_, hi_, d_stab):
            frames, bounds, _ = self._resident_warp(d_frames, d_disp[lo_:hi_], d_stab[lo_:hi_], out=out, warp_events=warp_events, check=check,
                                                    verdict=not crop)
            return frames, bounds

        on_prep = self.resident_chunks > 0 or self.resident_rectangle == 'early'       # the rectangle is final on the prep stream, early

        def exchange_ctx():
            # the 16-byte all-reduce of a sharded clip goes to the prep stream too: beside the warp, off the critical path
            return torch.cuda.stream(st['prep'])

        frames, bounds, d_stab, _ = mfdist.stabilize_sharded(F, jacobi_fn, warp_fn, lambda b: b, frame_range=(lo, hi), collective=collective,
                                                             exchange_ctx=exchange_ctx if (on_prep and collective) else None)
        if on_prep:
            main = torch.cuda.current_stream(dev)
            if collective and mfdist.active():
                done = torch.cuda.Event()
                done.record(st['prep'])
                main.wait_event(done)                        # the exchanged rectangle, back in current-stream order
                bounds.record_stream(main)
            elif self.resident_chunks <= 0:
                main.wait_event(st['scanned'])               # (the chunked arrangement joins the streams inside mf_warp_clip_u8c3)
        if not crop:
            return frames, bounds, d_stab
        # _crop_frames (mfs.py:159): behind the warp on the caller's stream, where the (all-reduced) rectangle is final by now; the kernels
        # read it from `bounds`, so nothing here waits.  The clip's status read-back goes behind the crop and takes its status word along.
        if n == 0:                                           # an empty shard: nothing to crop, no table slot, no verdict
            oW, oH = output_size if output_size is not None else (W, H)
            shape = (0, oH, oW) + tuple(d_frames.shape[3:])
            if cropped_out is not None and tuple(cropped_out.shape) != shape:
                raise ValueError(f'cropped_out must have shape {shape}, got {tuple(cropped_out.shape)}')
            return frames, bounds, d_stab, (cropped_out if cropped_out is not None else d_frames.new_empty(shape))
        slot = st['open'][0]
        if slot['crop_status'] is None:
            slot['crop_status'] = torch.zeros(1, dtype=torch.int32, device=dev)
        try:
            cropped, _ = ops.crop_resize_resident(frames, bounds, out=cropped_out, size=output_size, status=slot['crop_status'])
        finally:
            self._resident_verdict(st, check, cropped=True)
        return frames, bounds, d_stab, cropped

    def _checked_table(self, d_disp, W, H, adaptive_weights_definition, homographies):
        """What the frameless calls below start with, on torch's current stream: the Jacobi sweep on d_disp, then the cell table + plan of all
        its frames with a fresh clip rectangle.  Returns (table, bounds); waits for the table's status and raises `DegenerateMeshError`
        (clip_serial None) before anything has been warped."""
        import torch
        from . import ops
        d_stab = self._stabilized_vertex_displacements_device(d_disp, W, H, adaptive_weights_definition, homographies)
        bounds = torch.empty(4, dtype=torch.int32, device=d_disp.device)
        table = ops.cell_table(d_disp, d_stab, W, H, self.mesh_row_count, self.mesh_col_count, bounds=bounds)
        bad = int(table.status.item())
        if bad:
            raise DegenerateMeshError(bad, None)
        return table, bounds

    def stabilization_maps(self, d_disp, homographies, frame_width, frame_height,
                           adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, first=0, count=None, out=None):
        """The stabilisation's float32 coordinate maps without any frame: the Jacobi sweep (mfs.py:695-704) on d_disp -- (F, R+1, C+1, 2)
        float64 unstabilized vertex displacements in HBM --, the cell table + plan of all F frames, then `ops.warp_maps` for the frames
        first .. first + count - 1 (count=None: up to the last; `out`: a (count, H, W, 2) float32 tensor to fill).  Everything on torch's
        current stream.  Returns (maps, bounds): maps[f, y, x] = the source position (u, v) `stabilize_resident` samples for output pixel
        (x, y) of frame first + f, (W + 1, H + 1) where no cell owns the pixel; bounds = int32[4] device tensor {left, top, right, bottom},
        the crop rectangle of the frames of the range (mfs.py:1075-1106).  A degenerate mesh raises `DegenerateMeshError` (clip_serial None)
        here, synchronously, before the maps are written."""
        from . import ops
        self._check_definition(adaptive_weights_definition)
        self._check_mesh_shape(d_disp, d_disp.shape[0])
        W, H = int(frame_width), int(frame_height)
        table, bounds = self._checked_table(d_disp, W, H, adaptive_weights_definition, homographies)
        return ops.warp_maps(table, first=first, count=count, out=out, bounds=bounds), bounds

    def stabilized_planes(self, d_planes, d_disp, homographies, interpolation='linear', fill=0, crop=False, output_size=None, out=None,
                          adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL):
        """Side planes of a clip -- depth, flow, confidence (float32, 'linear') or labels and masks ('nearest', any dtype of 1, 2, 4 or 8
        bytes) -- moved exactly as `stabilize_resident` moves its colour frames, without any frame: the Jacobi sweep (mfs.py:695-704) on
        d_disp, the cell table + plan of all F frames, then `ops.warp_planes` on d_planes (F, H, W); like `stabilization_maps`, everything
        on torch's current stream.  crop=True: `ops.crop_resize_planes` from the clip rectangle as the warp left it on the device (it never
        visits the host), scaled to output_size = (width, height), by default back to (W, H) (mfs.py:1111-1157).  `out`: the tensor to fill
        (the cropped planes with crop=True).  Returns (planes, bounds): bounds = int32[4] device tensor {left, top, right, bottom}, the
        rectangle `stabilization_maps` returns for the same inputs.  A degenerate mesh raises `DegenerateMeshError` (clip_serial None) here,
        synchronously, before a plane is written.  (A caller that moves frames AND planes keeps one table: `_stabilized_frames_device`.)"""
        from . import ops
        self._check_definition(adaptive_weights_definition)
        self._check_mesh_shape(d_disp, d_disp.shape[0])
        if output_size is not None and not crop:
            raise ValueError('output_size belongs to crop=True')
        ops._need_planes(d_planes, interpolation, 'd_planes')
        H, W = int(d_planes.shape[1]), int(d_planes.shape[2])
        table, bounds = self._checked_table(d_disp, W, H, adaptive_weights_definition, homographies)
        if not crop:
            return ops.warp_planes(d_planes, table, interpolation, fill, out=out, bounds=bounds), bounds
        warped = ops.warp_planes(d_planes, table, interpolation, fill, bounds=bounds)
        cropped, _ = ops.crop_resize_planes(warped, bounds, interpolation, size=output_size, out=out)
        return cropped, bounds

    def _stabilized_yuv(self, fmt, d_y, d_uv, d_disp, homographies, border_yuv, out, adaptive_weights_definition, crop, output_size):
        """`stabilized_nv12`, `stabilized_p010`, `stabilized_p010_cropped`, `stabilized_nv16`, `stabilized_nv16_cropped`, `stabilized_p210` and
        `stabilized_p210_cropped` for the semi-planar
        format `fmt` (a row of ops.py): the argument checks -- the (d_y, d_uv) pair among them, so that a bad d_uv is a ValueError whatever the mesh is --,
        `_checked_table`, the warp and, with crop=True, the crop-resize of the warped temporaries from the rectangle on the device."""
        from . import ops
        if output_size is not None:
            if not crop:
                raise ValueError('output_size belongs to crop=True')
            ops._yuv_output_size(fmt, output_size, 'output_size')
        self._check_definition(adaptive_weights_definition)
        self._check_mesh_shape(d_disp, d_disp.shape[0])
        _, H, W = ops._need_yuv(fmt, d_y, d_uv, 'd_y', 'F')
        table, bounds = self._checked_table(d_disp, W, H, adaptive_weights_definition, homographies)
        if not crop:
            out_y, out_uv = ops._warp_yuv(fmt, d_y, d_uv, table, border_yuv, out, bounds)
            return out_y, out_uv, bounds
        warped_y, warped_uv = ops._warp_yuv(fmt, d_y, d_uv, table, border_yuv, None, bounds)
        out_y, out_uv, _ = ops._crop_resize_yuv(fmt, warped_y, warped_uv, bounds, output_size, out, None)
        return out_y, out_uv, bounds

    def stabilized_nv12(self, d_y, d_uv, d_disp, homographies, border_yuv=(81, 90, 240), out=None,
                        adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, crop=False, output_size=None):
        """An NV12 clip that a decoder left in device memory -- d_y (F, H, W) uint8 luma, d_uv (F, H/2, W/2, 2) uint8 interleaved chroma, U
        first -- stabilized without ever becoming BGR: the Jacobi sweep (mfs.py:695-704) on d_disp, the cell table + plan of all F frames, then
        `ops.warp_nv12`; like `stabilized_planes`, everything on torch's current stream.  Luma moves exactly as a grey clip does, chroma is
        sampled at half the luma coordinates of the even luma pixels (`ops.warp_nv12` has the definition).  border_yuv: (Y, U, V) of the
        uncovered area, by default BT.601 limited-range red (81, 90, 240) -- the reference's default BGR (0, 0, 255).  crop=True: the warp
        goes into temporaries and `ops.crop_resize_nv12` crops them from the clip rectangle as the warp left it on the device (the host never
        reads it), scaled to output_size = (width, height), even, by default back to (W, H) (mfs.py:1111-1157).  out: an (out_y, out_uv)
        pair to fill (the cropped pair with crop=True).  Returns (out_y, out_uv, bounds): bounds = int32[4] device tensor {left, top, right,
        bottom}, the rectangle `stabilization_maps` returns for the same inputs.  A degenerate mesh raises `DegenerateMeshError`
        (clip_serial None) here, synchronously, before a plane is written."""
        from . import ops
        return self._stabilized_yuv(ops._NV12, d_y, d_uv, d_disp, homographies, border_yuv, out, adaptive_weights_definition, crop, output_size)

    def stabilized_p010(self, d_y, d_uv, d_disp, homographies, border_yuv=(81 << 8, 90 << 8, 240 << 8), out=None,
                        adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, crop=False, output_size=None):
        """`stabilized_nv12` for a P010 clip -- d_y (F, H, W) uint16 luma, d_uv (F, H/2, W/2, 2) uint16 interleaved chroma, U first, what a
        decoder writes for 10-bit and HDR video (P012 and P016 alike) -- stabilized without ever becoming 3-channel uint16: the Jacobi sweep
        (mfs.py:695-704) on d_disp, the cell table + plan of all F frames, then `ops.warp_p010` (which has the definition), everything on
        torch's current stream.  border_yuv: (Y, U, V) of the uncovered area, by default BT.601 limited-range red at 10 bits in P010's high
        bits, (20736, 23040, 61440).  This call does not crop: crop=True or an output_size raises ValueError, and `stabilized_p010_cropped` is the
        call that crops and scales.  out: an (out_y, out_uv) pair
        to fill.  Returns (out_y, out_uv, bounds): bounds = int32[4] device tensor {left, top, right, bottom}, the rectangle
        `stabilization_maps` returns for the same inputs.  A degenerate mesh raises `DegenerateMeshError` (clip_serial None) here,
        synchronously, before a plane is written."""
        from . import ops
        if crop or output_size is not None:
            raise ValueError('crop-resize of 16-bit 4:2:0 clips is not built yet into stabilized_p010, which takes neither crop=True nor '
                             'output_size: call stabilized_p010_cropped')
        return self._stabilized_yuv(ops._P010, d_y, d_uv, d_disp, homographies, border_yuv, out, adaptive_weights_definition, False, None)

    def stabilized_p010_cropped(self, d_y, d_uv, d_disp, homographies, border_yuv=(81 << 8, 90 << 8, 240 << 8), out=None,
                                adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, output_size=None):
        """`stabilized_p010` followed by the reference's last step, _crop_frames (mfs.py:1111-1157), without the clip ever becoming 3-channel
        uint16: the cell table + plan of all F frames, `ops.warp_p010` into temporaries, then `ops.crop_resize_p010` from the clip rectangle
        as the warp left it on the device (the host never reads it), scaled to output_size = (width, height), even, by default back to
        (W, H); everything on torch's current stream.  d_y, d_uv, d_disp, homographies and border_yuv as in `stabilized_p010`.  out: an
        (out_y, out_uv) pair of the OUTPUT's size to fill.  Returns (out_y, out_uv, bounds): the cropped pair and the int32[4] device
        tensor {left, top, right, bottom} `stabilized_p010` returns for the same inputs.  A degenerate mesh raises `DegenerateMeshError`
        (clip_serial None) here, synchronously, before a plane is written."""
        from . import ops
        return self._stabilized_yuv(ops._P010, d_y, d_uv, d_disp, homographies, border_yuv, out, adaptive_weights_definition, True, output_size)

    def stabilized_nv16(self, d_y, d_uv, d_disp, homographies, border_yuv=(81, 90, 240), out=None,
                        adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL):
        """`stabilized_nv12` for an NV16 clip -- 4:2:2 as capture cards and grabbers deliver it: d_y (F, H, W) uint8 luma, d_uv (F, H, W/2, 2)
        uint8 interleaved chroma, U first, W even, H of either parity -- stabilized without ever becoming BGR and without dropping chroma rows:
        the Jacobi sweep (mfs.py:695-704) on d_disp, the cell table + plan of all F frames, then `ops.warp_nv16` (which has the definition),
        everything on torch's current stream.  d_disp and homographies come from `estimate_motion(d_y)`: the tracker takes the luma plane as it
        is.  This call does not crop or scale and takes no `crop` or `output_size`: `stabilized_nv16_cropped` is the call that does.  out: an
        (out_y, out_uv) pair to fill.  Returns (out_y, out_uv, bounds): bounds = int32[4] device tensor {left, top, right, bottom}, the
        rectangle `stabilization_maps` returns for the same inputs.  A degenerate mesh raises `DegenerateMeshError` (clip_serial None) here,
        synchronously, before a plane is written."""
        from . import ops
        return self._stabilized_yuv(ops._NV16, d_y, d_uv, d_disp, homographies, border_yuv, out, adaptive_weights_definition, False, None)

    def stabilized_packed_422(self, d_packed, d_disp, homographies, order='yuyv', border_yuv=(81, 90, 240), out=None,
                              adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL):
        """`stabilized_nv16` for a packed 4:2:2 clip -- d_packed (F, H, W, 2) uint8, order 'yuyv' (YUY2: bytes Y0 U Y1 V) or 'uyvy' (2vuy: U Y0
        V Y1), W even -- through `ops.warp_packed_422`: unpack, the NV16 warp, pack, with temporaries of twice the clip's size.  d_disp and
        homographies come from `estimate_motion` on the clip's luma plane, which for a packed clip is `ops.unpack_422(d_packed, order)[0]`.
        No `crop` or `output_size`, as for `stabilized_nv16`: `stabilized_packed_422_cropped` is the call that crops and scales.  out: the packed
        tensor to fill.  Returns (out_packed, bounds)."""
        from . import ops
        self._check_definition(adaptive_weights_definition)
        self._check_mesh_shape(d_disp, d_disp.shape[0])
        _, H, W = ops._need_packed_422(d_packed, 'd_packed')
        ops._order_422(order)
        table, bounds = self._checked_table(d_disp, W, H, adaptive_weights_definition, homographies)
        return ops.warp_packed_422(d_packed, table, order, border_yuv, out, bounds), bounds

    def stabilized_nv16_cropped(self, d_y, d_uv, d_disp, homographies, border_yuv=(81, 90, 240), out=None,
                                adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, output_size=None):
        """`stabilized_nv16` followed by the reference's last step, _crop_frames (mfs.py:1111-1157), without the clip ever becoming BGR: the
        cell table + plan of all F frames, `ops.warp_nv16` into temporaries, then `ops.crop_resize_nv16` from the clip rectangle as the warp
        left it on the device (the host never reads it), scaled to output_size = (width, height) -- the width even, the height of either
        parity --, by default back to (W, H); everything on torch's current stream.  d_y, d_uv, d_disp, homographies and border_yuv as in
        `stabilized_nv16`.  out: an (out_y, out_uv) pair of the OUTPUT's size to fill.  Returns (out_y, out_uv, bounds): the cropped pair and
        the int32[4] device tensor {left, top, right, bottom} `stabilized_nv16` returns for the same inputs.  A degenerate mesh raises
        `DegenerateMeshError` (clip_serial None) here, synchronously, before a plane is written."""
        from . import ops
        return self._stabilized_yuv(ops._NV16, d_y, d_uv, d_disp, homographies, border_yuv, out, adaptive_weights_definition, True, output_size)

    def stabilized_packed_422_cropped(self, d_packed, d_disp, homographies, order='yuyv', border_yuv=(81, 90, 240), out=None,
                                      adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, output_size=None):
        """`stabilized_nv16_cropped` for a packed 4:2:2 clip (d_packed and order as in `stabilized_packed_422`): unpack, the NV16 warp, the
        NV16 crop-resize from the rectangle on the device, pack -- the pair stays unpacked between the warp and the crop.  out: the packed
        (F, height, width, 2) tensor of the OUTPUT's size to fill.  Returns (out_packed, bounds)."""
        import torch
        from . import ops
        n, H, W = ops._need_packed_422(d_packed, 'd_packed')
        ops._order_422(order)
        oW, oH = (W, H) if output_size is None else ops._yuv_output_size(ops._NV16, output_size, 'output_size')
        if out is not None:
            ops._plane_yuv(out, 'out', (n, oH, oW, 2), d_packed.device, torch.uint8)
        d_y, d_uv = ops.unpack_422(d_packed, order)
        out_y, out_uv, bounds = self._stabilized_yuv(ops._NV16, d_y, d_uv, d_disp, homographies, border_yuv, None, adaptive_weights_definition, True,
                                                     (oW, oH))
        return ops.pack_422(out_y, out_uv, order, out), bounds

    def stabilized_p210(self, d_y, d_uv, d_disp, homographies, border_yuv=(81 << 8, 90 << 8, 240 << 8), out=None,
                        adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL):
        """`stabilized_nv16` for a P210 clip -- 10-bit 4:2:2 as SDI / HDMI capture and ProRes / XAVC decoders deliver it: d_y (F, H, W) uint16
        luma, d_uv (F, H, W/2, 2) uint16 interleaved chroma, U first, W even, H of either parity, plain 16-bit samples (P212 and P216 alike) --
        stabilized without truncating to 8 bits: the Jacobi sweep (mfs.py:695-704) on d_disp, the cell table + plan of all F frames, then
        `ops.warp_p210` (which has the definition), everything on torch's current stream.  d_disp and homographies come from
        `estimate_motion(ops.luma(d_y))`.  border_yuv: as in `stabilized_p010`.  This call does not crop or scale: `stabilized_p210_cropped`
        does.  out: an (out_y, out_uv) pair to fill.  Returns (out_y, out_uv, bounds), as `stabilized_nv16`.  (Not provided: v210, kernels
        on the packed words, the host and clip pipelines.)"""
        from . import ops
        return self._stabilized_yuv(ops._P210, d_y, d_uv, d_disp, homographies, border_yuv, out, adaptive_weights_definition, False, None)

    def stabilized_p210_cropped(self, d_y, d_uv, d_disp, homographies, border_yuv=(81 << 8, 90 << 8, 240 << 8), out=None,
                                adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, output_size=None):
        """`stabilized_p210` followed by the reference's last step, _crop_frames (mfs.py:1111-1157): `ops.warp_p210` into temporaries, then
        `ops.crop_resize_p210` from the clip rectangle as the warp left it on the device, scaled to output_size = (width, height) -- the width
        even, the height of either parity --, by default back to (W, H).  out: an (out_y, out_uv) pair of the OUTPUT's size to fill.  Returns
        (out_y, out_uv, bounds), as `stabilized_nv16_cropped`."""
        from . import ops
        return self._stabilized_yuv(ops._P210, d_y, d_uv, d_disp, homographies, border_yuv, out, adaptive_weights_definition, True, output_size)

    def stabilized_y210(self, d_packed, d_disp, homographies, border_yuv=(81 << 8, 90 << 8, 240 << 8), out=None,
                        adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL):
        """`stabilized_p210` for a packed Y210 / Y216 clip -- d_packed (F, H, W, 2) uint16, words Y0 U Y1 V, W even -- through `ops.warp_y210`:
        unpack, the P210 warp, pack.  d_disp and homographies come from `estimate_motion` on `ops.luma(ops.unpack_y210(d_packed)[0])`.  out: the
        packed tensor to fill.  Returns (out_packed, bounds)."""
        from . import ops
        self._check_definition(adaptive_weights_definition)
        self._check_mesh_shape(d_disp, d_disp.shape[0])
        _, H, W = ops._need_y210(d_packed, 'd_packed')
        table, bounds = self._checked_table(d_disp, W, H, adaptive_weights_definition, homographies)
        return ops.warp_y210(d_packed, table, border_yuv, out, bounds), bounds

    def stabilized_y210_cropped(self, d_packed, d_disp, homographies, border_yuv=(81 << 8, 90 << 8, 240 << 8), out=None,
                                adaptive_weights_definition=ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, output_size=None):
        """`stabilized_p210_cropped` for a packed Y210 / Y216 clip (d_packed as in `stabilized_y210`): unpack, the P210 warp, the P210
        crop-resize from the rectangle on the device, pack -- the pair stays unpacked between the warp and the crop.  out: the packed
        (F, height, width, 2) tensor of the OUTPUT's size to fill.  Returns (out_packed, bounds)."""
        import torch
        from . import ops
        n, H, W = ops._need_y210(d_packed, 'd_packed')
        oW, oH = (W, H) if output_size is None else ops._yuv_output_size(ops._P210, output_size, 'output_size')
        if out is not None:
            ops._plane_yuv(out, 'out', (n, oH, oW, 2), d_packed.device, torch.uint16)
        d_y, d_uv = ops.unpack_y210(d_packed)
        out_y, out_uv, bounds = self._stabilized_yuv(ops._P210, d_y, d_uv, d_disp, homographies, border_yuv, None, adaptive_weights_definition, True,
                                                     (oW, oH))
        return ops.pack_y210(out_y, out_uv, out), bounds

    def _stabilized_frames_device(self, d_frames, d_unstab, d_stab, out=None, table=None):
        """d_frames: (n, H, W, 3) uint8; d_unstab/d_stab: (n, R+1, C+1, 2) float64, all in HBM.
        Returns (stabilized frames (n, H, W, 3) uint8, per-frame crop values (n, 4) int32), in HBM.
        table: a `CellTable` to (re)build for this clip instead of a new one -- the caller keeps it, and `ops.warp_planes(planes, table)`
        then moves the clip's side planes through the very table its frames went through, without a second cell table or plan."""
        from . import ops
        n, H, W, _ = d_frames.shape
        table = ops.cell_table(d_unstab, d_stab, W, H, self.mesh_row_count, self.mesh_col_count, table=table)
        out = ops.warp(d_frames, table, self.color_outside_image_area_bgr, out=out)
        table.check()
        return out, table.crop
