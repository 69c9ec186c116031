"""A clip in host memory, as the reference hands it to the hot path: a Python list of F NumPy frames (mfs.py:150-159, 213,
997-1100) or one (F, H, W, 3) array.  The staging itself -- chunked, overlapped PCIe copies around the kernels -- lives below
Python, in csrc/hostpipe.hip (ONE implementation: `mf_warp_u8c3_host_frames`, `mf_warp_crop_u8c3_host_frames`,
`mf_crop_resize_u8c3_host_frames`, and their u8c1 twins for single-channel frames); this module only validates the frames and hands out
their addresses."""
import numpy as np


def _need_u8(a):
    """cv2.remap runs its 8-bit fixed-point path on uint8 frames only (mfs.py:1063-1069: what a VideoCapture delivers); float or 16-bit
    frames would take other OpenCV code with other arithmetic -- refused instead of silently cast."""
    if a.dtype != np.uint8:
        raise TypeError(f'frames must be uint8 (got {a.dtype}): the warp reproduces cv2.remap\'s 8-bit fixed-point interpolation')


def _as_frame(frame, shape):
    a = np.asarray(frame)
    _need_u8(a)
    a = np.ascontiguousarray(a)
    if a.shape != shape:
        raise ValueError(f'every frame must have shape {shape}, got {a.shape}')
    return a


class HostClip:
    """A clip in host memory: either one (F, H, W, 3) uint8 array or a sequence of F (H, W, 3) arrays -- or, single-channel (grey), one
    (F, H, W) uint8 array or a sequence of F (H, W) arrays (mfs.py:942, 1129 read shape[:2] only; cv2.remap and cv2.resize take 2-D
    frames).  `channels` is 3 or 1; a clip is one or the other throughout."""

    def __init__(self, frames, num_frames):
        if isinstance(frames, np.ndarray):
            if frames.ndim not in (3, 4) or frames.shape[0] != num_frames or (frames.ndim == 4 and frames.shape[3] != 3):
                raise ValueError('frames must be num_frames arrays of shape (H, W, 3) or (H, W)')
            _need_u8(frames)
            self.array = np.ascontiguousarray(frames)
            self.frames = None
            self.height, self.width = self.array.shape[1:3]
            self.channels = 3 if frames.ndim == 4 else 1
        else:
            if len(frames) != num_frames or num_frames == 0:
                raise ValueError('frames must be num_frames arrays of shape (H, W, 3) or (H, W)')
            first = np.asarray(frames[0])
            if not (first.ndim == 2 or (first.ndim == 3 and first.shape[2] == 3)):
                raise ValueError('frames must be num_frames arrays of shape (H, W, 3) or (H, W)')
            self.height, self.width = first.shape[:2]
            self.channels = 3 if first.ndim == 3 else 1
            # EVERY frame is checked here, before anything is issued (dtype uint8, the first frame's shape; C-contiguous -- a frame that
            # is not gets a contiguous copy, the others are taken as they are): a bad frame k fails in the constructor, not mid-clip
            self.array = None
            self.frames = [_as_frame(f, first.shape) for f in frames]
        self.num_frames = num_frames

    @property
    def frame_shape(self):
        """(H, W, 3) or, single-channel, (H, W)."""
        return (self.height, self.width, 3) if self.channels == 3 else (self.height, self.width)

    def upload(self, d_frames, i0, i1):
        """Blocking copy of frames i0..i1-1 into d_frames[i0:i1] on the calling thread's current stream (streaming.py's decode-side
        staging; the clip methods of the stabilizer go through csrc/hostpipe.hip instead)."""
        import torch
        if self.array is not None:
            d_frames[i0:i1].copy_(torch.from_numpy(self.array[i0:i1]))
        else:
            for i in range(i0, i1):
                d_frames[i].copy_(torch.from_numpy(self.frames[i]))
