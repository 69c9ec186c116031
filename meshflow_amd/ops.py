"""Device-level operators: torch tensors in, torch tensors out, HIP kernels underneath.

torch is used only for device memory, streams and (in `dist.py`) torch.distributed; every operator
hands raw device pointers to libmeshflow_hip.so through the C ABI (`_lib.py`) on torch's current
stream, so torch.cuda events and synchronisation see the kernels."""
import collections
import ctypes
import math

import numpy as np
import torch

from . import _lib

_lib_ = _lib.lib


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _need(t, dtype, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f'{name} must be a CUDA/HIP torch tensor')
    if t.dtype != dtype:
        raise ValueError(f'{name} must have dtype {dtype}, got {t.dtype}')
    if not t.is_contiguous():
        raise ValueError(f'{name} must be contiguous')


def _border_samples(ctype, top, count):
    """Border colour -> what a C call takes: clamp(round(v), 0, top) of the first `count` components -- the value itself, not scaled to 16
    bits (cv2.remap's saturate_cast of borderValue; a 1-channel image uses borderValue[0]) -- as an array, or one value for count 1.  Missing
    components are 0, as cv::Scalar pads them: a 3-component border gives a 4-channel frame alpha 0."""
    def convert(border_bgr):
        v = [int(np.clip(round(float(c)), 0, top)) for c in border_bgr[:count]]
        v += [0] * (count - len(v))
        return (ctype * count)(*v) if count > 1 else ctype(v[0])
    return convert


# One row per pixel format of the device path: the frames it takes and the C calls that serve them (include/meshflow_hip.h).
PixelFormat = collections.namedtuple('PixelFormat', 'dtype channels border warp warp_bounds warp_clip crop_resize crop_resize_to crop_resize_dev')


def _row(name, dtype, channels, ctype, top):
    calls = (getattr(_lib_, f'mf_{op}_{name}') for op in ('warp', 'warp_bounds', 'warp_clip', 'crop_resize', 'crop_resize_to', 'crop_resize_dev'))
    return PixelFormat(dtype, channels, _border_samples(ctype, top, channels), *calls)


_FORMATS = (_row('u8c3', torch.uint8, 3, ctypes.c_uint8, 255),
            _row('u16c3', torch.uint16, 3, ctypes.c_uint16, 65535),   # cv2.remap's / cv2.resize's 16U arithmetic
            _row('u8c1', torch.uint8, 1, ctypes.c_uint8, 255),        # channel 0 of the BGR result of the frames repeated
            _row('u8c4', torch.uint8, 4, ctypes.c_uint8, 255))        # the BGR result on channels 0-2, the u8c1 result on channel 3
_FRAME_DTYPES = {f.dtype for f in _FORMATS}


def pixel_format(dtype, shape):
    """The format of frames of this dtype and shape: (n, H, W, 3) uint8 or uint16 BGR, (n, H, W) uint8 single-channel, or (n, H, W, 4)
    uint8 BGRA / RGBA.  Grey and 4-channel frames of another dtype are refused naming it; other shapes and dtypes raise ValueError."""
    if len(shape) == 3:
        channels = 1
    elif len(shape) == 4 and shape[3] in (3, 4):
        channels = shape[3]
    else:
        raise ValueError('frames must be (n, H, W, 3), or (n, H, W) or (n, H, W, 4) uint8')
    for f in _FORMATS:
        if (f.dtype, f.channels) == (dtype, channels):
            return f
    if channels == 1:
        raise ValueError(f'single-channel frames must be uint8 (got {dtype}): (n, H, W) {dtype} frames are not supported')
    if channels == 4:
        raise ValueError(f'4-channel frames must be uint8 (got {dtype}): (n, H, W, 4) {dtype} frames are not supported')
    raise ValueError(f'frames must have dtype {torch.uint8}, got {dtype}')


def _frames_format(frames):
    """Check a device frame stack and return its format."""
    _need(frames, frames.dtype if isinstance(frames, torch.Tensor) and frames.dtype in _FRAME_DTYPES else torch.uint8, 'frames')
    return pixel_format(frames.dtype, frames.shape)


def _out_for(frames, fmt, out):
    """`out` (None: a new tensor) checked for `frames`; a single-channel or 4-channel one must have their shape."""
    if out is None:
        return torch.empty_like(frames)
    _need(out, fmt.dtype, 'out')
    if fmt.channels in (1, 4) and out.shape != frames.shape:
        raise ValueError('out must have the shape of frames')
    return out


def jacobi(b, taps, lam, inv_on, omega, iters, out=None):
    """`iters` Jacobi sweeps for all S series at once (mfs.py:844-878 x every vertex).
    b: (F, S) float64 device tensor, frame-major.  Returns x (F, S)."""
    _need(b, torch.float64, 'b')
    for name, t in (('taps', taps), ('lam', lam), ('inv_on', inv_on)):
        _need(t, torch.float64, name)
    F, S = b.shape
    if taps.numel() != 2 * omega + 1 or lam.numel() != F or inv_on.numel() != F:
        raise ValueError('coefficient sizes do not match (F, omega)')
    x = out if out is not None else torch.empty_like(b)
    _need(x, torch.float64, 'out')
    _lib.check(_lib_.mf_jacobi_f64(_ptr(b), _ptr(x), _ptr(taps), _ptr(lam), _ptr(inv_on), F, S, int(omega),
                                   int(iters), _stream()))
    return x


class CellTable:
    """Per-cell records + compact boxes of n frames (layout: include/meshflow_hip.h).  One object serves clips of any length of
    its geometry: `resize(n)` re-views the (grow-only) buffers for n frames."""

    def __init__(self, n, W, H, R, C, device):
        self.W, self.H, self.R, self.C = W, H, R, C
        self.device = device
        self.capacity = 0
        self.status = torch.zeros(1, dtype=torch.int32, device=device)
        self.bounds = None            # clip-level rectangle, filled by warp_clip
        self.resize(n)

    def resize(self, n):
        """View the table for n frames (allocates when n exceeds every earlier n; the contents do not survive a resize)."""
        if n > self.capacity:
            self.buf = torch.empty(_lib_.mf_cell_table_bytes(n, self.W, self.H, self.R, self.C), dtype=torch.uint8, device=self.device)
            self._crop = torch.empty((n, 4), dtype=torch.int32, device=self.device)
            self.capacity = n
        if n != getattr(self, 'n', None):
            self.n = n
            self.crop = self._crop[:n]
            off = _lib_.mf_cell_table_bounds_offset(n, self.W, self.H, self.R, self.C)
            # the rectangle as the kernels fold it together inside the table blob when no caller-owned tensor is given (valid after the
            # warp / crop scan of all n frames; overwritten by the next cell_table on this object)
            self.clip_bounds = self.buf[off:off + 16].view(torch.int32)
        return self

    def records(self):
        """(n, R*C, 32) float64 view of the records (for tests)."""
        nrec = self.n * self.R * self.C
        return self.buf[:nrec * _lib.CELL_DOUBLES * 8].view(torch.float64).view(self.n, self.R * self.C, _lib.CELL_DOUBLES)

    def check(self):
        """Raise if a cell had no homography (the reference would fail inside cv2.warpPerspective)."""
        bad = int(self.status.item())
        if bad:
            raise ValueError(f'{bad} degenerate mesh cell(s): no homography exists '
                             '(cv2.findHomography would return None)')


def _need_bounds(bounds):
    _need(bounds, torch.int32, 'bounds')
    if bounds.numel() != 4:
        raise ValueError('bounds must hold 4 int32 {left, top, right, bottom}')


def cell_table(unstab, stab, W, H, R, C, table=None, reset_status=True, bounds=None):
    """Per-cell homographies of n frames (mfs.py:1039-1048).  unstab/stab: (n, R+1, C+1, 2) or (n, V*2)
    float64 device tensors.  Also resets the per-frame crop values to their defaults (mfs.py:992-995).
    bounds: a caller-owned int32[4] device tensor that receives the clip-level rectangle (defaults here; `warp` / `crop_scan` called
    with the same tensor fold their frames into it) instead of the four words inside the table (`table.clip_bounds`)."""
    _need(unstab, torch.float64, 'unstab')
    _need(stab, torch.float64, 'stab')
    n = unstab.shape[0]
    V2 = (R + 1) * (C + 1) * 2
    if unstab.numel() != n * V2 or stab.numel() != n * V2:
        raise ValueError('displacement tensors do not match (n, R+1, C+1, 2)')
    if table is None:
        table = CellTable(n, W, H, R, C, unstab.device)
    else:
        if (table.W, table.H, table.R, table.C) != (W, H, R, C):
            raise ValueError('the cell table was made for another frame size / mesh')
        table.resize(n)
        if reset_status:
            table.status.zero_()          # reset_status=False: keep accumulating; the caller checks once later
    if bounds is None:
        _lib.check(_lib_.mf_cell_table_f64(_ptr(unstab), _ptr(stab), n, W, H, R, C, _ptr(table.buf), _ptr(table.crop),
                                           _ptr(table.status), _stream()))
    else:
        _need_bounds(bounds)
        _lib.check(_lib_.mf_cell_table_bounds_f64(_ptr(unstab), _ptr(stab), n, W, H, R, C, _ptr(table.buf), _ptr(table.crop),
                                                  _ptr(table.status), _ptr(bounds), _stream()))
    return table


def warp(frames, table, border_bgr=(0, 0, 255), out=None, bounds=None):
    """Mesh warp + crop scan of n frames (mfs.py:1000-1100).  frames: (n, H, W, 3) uint8 or uint16 device tensor (uint16: cv2.remap's
    16U arithmetic, include/meshflow_hip.h mf_warp_u16c3; the crop values are those of the uint8 warp of the same table), or (n, H, W)
    uint8 single-channel frames (mf_warp_u8c1: channel 0 of the BGR warp of the frames repeated, border byte = border_bgr[0]), or
    (n, H, W, 4) uint8 BGRA / RGBA frames (mf_warp_u8c4: channels 0-2 as the BGR warp, channel 3 as the single-channel warp of the alpha
    plane; border_bgr may have 4 components, a 3-component one gets alpha 0 -- the uncovered area comes out transparent).
    Returns the stabilized frames (the input's dtype); per-frame crop values accumulate in table.crop, the clip-level rectangle in
    `bounds` (the tensor `cell_table` was given) or, without one, in table.clip_bounds."""
    fmt = _frames_format(frames)
    n, H, W = frames.shape[:3]
    if (n, W, H) != (table.n, table.W, table.H):
        raise ValueError('frames do not match the cell table (n, H, W, 3) or (n, H, W)')
    out = _out_for(frames, fmt, out)
    border = fmt.border(border_bgr)
    if bounds is None:
        _lib.check(fmt.warp(_ptr(frames), _ptr(out), _ptr(table.buf), n, W, H, table.R, table.C, border, _ptr(table.crop), _stream()))
    else:
        _need_bounds(bounds)
        _lib.check(fmt.warp_bounds(_ptr(frames), _ptr(out), _ptr(table.buf), n, W, H, table.R, table.C, border, _ptr(table.crop),
                                   _ptr(bounds), _stream()))
    return out


def warp_clip(frames, unstab, stab, table, border_bgr=(0, 0, 255), out=None, chunks=4, prep_stream=None, bounds=None):
    """mfs.py:909-1108 for a clip resident in HBM as ONE call overlapped inside the clip (csrc/clippipe.hip): cell table + plan +
    crop scan + clip rectangle on `prep_stream` (a torch stream; None = the library's own, forked from the current stream), the warp
    of `chunks` frame ranges on torch's current stream, each waiting for its own table only.  chunks=0: in order on the current
    stream -- table, warp alone, rectangle (early on `prep_stream` when one is given).  Returns (stabilized frames,
    bounds): bounds = int32 {left, top, right, bottom} of the clip -- the caller's tensor when one is given, else table.bounds --,
    folded together by the kernels, final on the prep stream right after the tables' crop scan (and on the current stream after
    the call); per-frame values in table.crop; table.status accumulates degenerate cells.  frames: uint8 or uint16, (n, H, W) uint8 or
    (n, H, W, 4) uint8 (see `warp`)."""
    fmt = _frames_format(frames)
    _need(unstab, torch.float64, 'unstab')
    _need(stab, torch.float64, 'stab')
    n, H, W = frames.shape[:3]
    V2 = (table.R + 1) * (table.C + 1) * 2
    if (n, W, H) != (table.n, table.W, table.H) or unstab.numel() != n * V2 or stab.numel() != n * V2:
        raise ValueError('frames / displacements do not match the cell table')
    out = _out_for(frames, fmt, out)
    if bounds is None:                  # (without a caller-owned tensor: one per table, rewritten by the next call on it)
        if table.bounds is None:
            table.bounds = torch.empty(4, dtype=torch.int32, device=frames.device)
        bounds = table.bounds
    else:
        _need_bounds(bounds)
    prep = ctypes.c_void_p(prep_stream.cuda_stream) if prep_stream is not None else None
    _lib.check(fmt.warp_clip(_ptr(frames), _ptr(out), _ptr(unstab), _ptr(stab), n, W, H, table.R, table.C, fmt.border(border_bgr),
                             _ptr(table.buf), _ptr(table.crop), _ptr(bounds), _ptr(table.status), int(chunks), prep, _stream()))
    return out, bounds


def crop_scan(table, bounds=None):
    """The four edge scans of mfs.py:1075-1098 from the cell table alone (no frame is touched): fills table.crop exactly as
    `warp` would (and folds the clip-level rectangle into `bounds` / table.clip_bounds).  Returns table.crop, (n, 4) int32
    {left, top, right, bottom}."""
    if bounds is None:
        _lib.check(_lib_.mf_crop_scan_f64(_ptr(table.buf), table.n, table.W, table.H, table.R, table.C, _ptr(table.crop), _stream()))
    else:
        _need_bounds(bounds)
        _lib.check(_lib_.mf_crop_scan_bounds_f64(_ptr(table.buf), table.n, table.W, table.H, table.R, table.C, _ptr(table.crop),
                                                 _ptr(bounds), _stream()))
    return table.crop


def _maps_range(table, first, count):
    """(first, count) of a `warp_maps` call as two ints inside the table's frames; count=None: up to the table's last frame."""
    for name, v in (('first', first), ('count', count)):
        if v is not None and (isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer))):
            raise ValueError(f'{name} must be an int, got {v!r}')
    first = int(first)
    if not 0 <= first <= table.n:
        raise ValueError(f'first={first} is not inside the cell table\'s {table.n} frames')
    count = table.n - first if count is None else int(count)
    if count < 0 or count > table.n - first:
        raise ValueError(f'frames first={first} count={count} are not inside the cell table\'s {table.n} frames')
    return first, count


def warp_maps(table, first=0, count=None, out=None, bounds=None):
    """The warp's float32 coordinate maps instead of pixels (mf_warp_maps_f32; the reference's frame_stabilized_x_y, mfs.py:1054-1061, which
    it hands to cv2.remap at mfs.py:1063-1069): for the table's frames first .. first + count - 1 (count=None: up to the last) a
    (count, H, W, 2) float32 tensor on the table's device, x first -- maps[f, y, x] = the source position (u, v) the pixel warps sample for
    output pixel (x, y), bit for bit; a pixel no cell owns holds (W + 1, H + 1) (mfs.py:983-984), which lies outside every frame.  No frame is
    read: sample any layer that has to move with the video (labels, depth, float32 planes) with a sampler of your own, e.g.
    `torch.nn.functional.grid_sample(layer, maps_to_grid(maps))`.  A long clip can be walked through an `out` of a few frames.
    The frames' crop values accumulate in table.crop (rows outside the range are not touched) and the clip-level rectangle in `bounds` /
    table.clip_bounds exactly as `warp` does it; calling both on one table changes nothing."""
    first, count = _maps_range(table, first, count)
    shape = (count, table.H, table.W, 2)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=table.device)
    else:
        _need(out, torch.float32, 'out')
        if tuple(out.shape) != shape:
            raise ValueError(f'out must have shape {shape} for frames {first} .. {first + count - 1}, got {tuple(out.shape)}')
        if out.device != torch.device(table.device):
            raise ValueError(f'out must be on the cell table\'s device {table.device}, got {out.device}')
    if bounds is None:
        _lib.check(_lib_.mf_warp_maps_f32(_ptr(table.buf), _ptr(out), table.n, table.W, table.H, table.R, table.C, first, count,
                                          _ptr(table.crop), _stream()))
    else:
        _need_bounds(bounds)
        _lib.check(_lib_.mf_warp_maps_bounds_f32(_ptr(table.buf), _ptr(out), table.n, table.W, table.H, table.R, table.C, first, count,
                                                 _ptr(table.crop), _ptr(bounds), _stream()))
    return out


def maps_to_grid(maps, align_corners=True):
    """`warp_maps`' pixel coordinates (..., H, W, 2) as the normalised grid `torch.nn.functional.grid_sample` takes: 2 u / (W - 1) - 1 (and
    the same in y with H) for align_corners=True -- pass the same flag to grid_sample --, (2 u + 1) / W - 1 otherwise.  Pixels no cell owns,
    at (W + 1, H + 1), land outside [-1, 1]: padding_mode='zeros' leaves them empty.  Pure torch, on whatever device `maps` lives; float32 in,
    float32 out.  A convenience and NOT bit-exact: the maps are the reference's own arrays, this division and grid_sample's arithmetic are
    torch's."""
    if not isinstance(maps, torch.Tensor) or not maps.is_floating_point() or maps.dim() < 3 or maps.shape[-1] != 2:
        raise ValueError('maps must be a floating-point tensor of shape (..., H, W, 2)')
    H, W = maps.shape[-3], maps.shape[-2]
    if align_corners:
        if W < 2 or H < 2:
            raise ValueError('align_corners=True needs W, H >= 2')
        scale = torch.tensor([2.0 / (W - 1), 2.0 / (H - 1)], dtype=maps.dtype, device=maps.device)
        return maps * scale - 1.0
    size = torch.tensor([float(W), float(H)], dtype=maps.dtype, device=maps.device)
    return (2.0 * maps + 1.0) / size - 1.0


def crop_reduce(crop, W, H):
    """Clip-level bounds (mfs.py:1103-1106): int32 tensor {left, top, right, bottom}."""
    _need(crop, torch.int32, 'crop')
    bounds = torch.empty(4, dtype=torch.int32, device=crop.device)
    _lib.check(_lib_.mf_crop_reduce(_ptr(crop), crop.shape[0], W, H, _ptr(bounds), _stream()))
    return bounds


def check_output_size(size, name='size'):
    """A (width, height) output size -- cv2.resize's dsize order -- as two Python ints in 1 .. 32,767; ValueError otherwise."""
    try:
        w, h = size
    except (TypeError, ValueError):
        raise ValueError(f'{name} must be (width, height), got {size!r}') from None
    for v in (w, h):
        if isinstance(v, (bool, np.bool_)) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= 32767:
            raise ValueError(f'{name} must be two ints in 1 .. 32767 (width, height), got {size!r}')
    return int(w), int(h)


def _device_rectangle(bounds, status):
    """Whether `bounds` is a device rectangle (an int32[4] tensor, checked) and not four host numbers; only a device rectangle takes `status`."""
    if isinstance(bounds, torch.Tensor):
        _need_bounds(bounds)
        return True
    if status is not None:
        raise ValueError('status belongs to a device rectangle: a host rectangle is checked when the call is made')
    return False


def _status_for(status, device):
    """The status word of a device-rectangle call: the caller's int32[1] device tensor, checked, or a new zeroed one on `device`."""
    if status is None:
        return torch.zeros(1, dtype=torch.int32, device=device)
    _need(status, torch.int32, 'status')
    if status.numel() != 1:
        raise ValueError('status must hold 1 int32')
    return status


def crop_resize(frames, bounds, out=None, size=None):
    """Crop to the inclusive (left, top, right, bottom) and resize back to (W, H): mfs.py:1111-1157.  frames: uint8 or uint16 (uint16:
    cv2.resize's float path, mf_crop_resize_u16c3), (n, H, W) uint8 (mf_crop_resize_u8c1) or (n, H, W, 4) uint8 (mf_crop_resize_u8c4: the
    BGR result on channels 0-2, the single-channel one on channel 3); the output has the input's dtype and shape.
    size=(width, height) (cv2.resize's dsize order) scales the crop to that size instead (mf_crop_resize_to_*): the output is then
    (n, height, width[, 3 or 4]), and so must `out` be; size == (W, H) is the default call."""
    fmt = _frames_format(frames)
    n, H, W = frames.shape[:3]
    left, top, right, bottom = (int(v) for v in bounds)
    if size is None:
        out = _out_for(frames, fmt, out)
        work = torch.empty(_lib_.mf_crop_resize_workspace_bytes(W, H), dtype=torch.uint8, device=frames.device)
        _lib.check(fmt.crop_resize(_ptr(frames), _ptr(out), n, W, H, left, top, right, bottom, _ptr(work), _stream()))
        return out
    oW, oH = check_output_size(size)
    shape = (n, oH, oW) + tuple(frames.shape[3:])
    if out is None:
        out = torch.empty(shape, dtype=frames.dtype, device=frames.device)
    else:
        _need(out, fmt.dtype, 'out')
        if tuple(out.shape) != shape:
            raise ValueError(f'out must have shape {shape} for size {(oW, oH)}, got {tuple(out.shape)}')
    work = torch.empty(_lib_.mf_crop_resize_workspace_bytes(oW, oH), dtype=torch.uint8, device=frames.device)
    _lib.check(fmt.crop_resize_to(_ptr(frames), _ptr(out), n, W, H, left, top, right, bottom, oW, oH, _ptr(work), _stream()))
    return out


def crop_resize_resident(frames, bounds, out=None, size=None, status=None):
    """`crop_resize` from a rectangle that stays on the device (mfs.py:1111-1157, mf_crop_resize_dev_*): `bounds` is a 4-element int32
    DEVICE tensor {left, top, right, bottom} -- what `warp_clip` / `stabilize_resident` return -- that the kernels read when they execute,
    in stream order; the host never reads it and the call never waits.  frames, out and size as in `crop_resize`; for a usable rectangle
    the result is byte for byte `crop_resize(frames, tuple(bounds.tolist()), size=size)`.
    Returns (cropped frames, status): status is an int32[1] device tensor -- the caller's (not reset here: it accumulates) or a new zeroed
    one.  A rectangle that cannot be used (empty, a negative edge, outside the frame: what `crop_resize` raises ValueError for) adds 1 to
    it and leaves `out` untouched; the caller reads it whenever it next synchronises."""
    fmt = _frames_format(frames)
    _need_bounds(bounds)
    n, H, W = frames.shape[:3]
    oW, oH = (W, H) if size is None else check_output_size(size)
    shape = (n, oH, oW) + tuple(frames.shape[3:])
    if out is None:
        out = torch.empty(shape, dtype=frames.dtype, device=frames.device)
    else:
        _need(out, fmt.dtype, 'out')
        if tuple(out.shape) != shape:
            raise ValueError(f'out must have shape {shape} for size {(oW, oH)}, got {tuple(out.shape)}')
    status = _status_for(status, frames.device)
    work = torch.empty(_lib_.mf_crop_resize_workspace_bytes(oW, oH), dtype=torch.uint8, device=frames.device)
    _lib.check(fmt.crop_resize_dev(_ptr(frames), _ptr(out), n, W, H, _ptr(bounds), oW, oH, _ptr(work), _ptr(status), _stream()))
    return out, status


def _need_planes(planes, interpolation, name='planes'):
    """Check a stack of side planes for `warp_planes` / `crop_resize_planes`: a contiguous (n, H, W) device tensor, float32 for 'linear',
    any dtype of 1, 2, 4 or 8 bytes for 'nearest' (moved as bytes: nothing depends on torch kernels for the dtype).  Returns the C call's
    elem_bytes (0: the float32 linear call)."""
    if interpolation not in ('linear', 'nearest'):
        raise ValueError(f"interpolation must be 'linear' or 'nearest', got {interpolation!r}")
    if not isinstance(planes, torch.Tensor) or not planes.is_cuda:
        raise ValueError(f'{name} must be a CUDA/HIP torch tensor')
    if planes.dim() != 3:
        raise ValueError(f'{name} must be (n, H, W) planes, got shape {tuple(planes.shape)}')
    if not planes.is_contiguous():
        raise ValueError(f'{name} must be contiguous')
    if interpolation == 'linear':
        if planes.dtype != torch.float32:
            raise ValueError(f"'linear' planes must be {torch.float32}, got {planes.dtype} (labels and masks: interpolation='nearest')")
        return 0
    if planes.is_complex() or planes.element_size() not in (1, 2, 4, 8):
        raise ValueError(f"'nearest' planes must have elements of 1, 2, 4 or 8 bytes, got {planes.dtype}")
    return planes.element_size()


def _fill_bits(fill, dtype):
    """`fill` cast to dtype, as the bit pattern of one element (an int below 2^64)."""
    one = torch.tensor([fill], dtype=dtype)
    return int.from_bytes(one.view(torch.uint8).numpy().tobytes(), 'little')


def _planes_out(planes, shape, out):
    if out is None:
        return torch.empty(shape, dtype=planes.dtype, device=planes.device)
    _need(out, planes.dtype, 'out')
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f'out must have shape {tuple(shape)}, got {tuple(out.shape)}')
    if out.device != planes.device:
        raise ValueError(f'out must be on the planes\' device {planes.device}, got {out.device}')
    return out


def warp_planes(planes, table, interpolation='linear', fill=0, out=None, bounds=None):
    """The mesh warp of side planes -- what travels with a video without being a picture: depth, disparity, flow components, confidence
    (float32, 'linear') or labels and masks ('nearest') -- sampled at the positions the pixel warps of the same table sample
    (mf_warp_plane_f32 / mf_warp_plane_nearest; the arrays the reference hands to cv2.remap at mfs.py:1063-1069).  planes: a contiguous
    (n, H, W) device tensor, n == table.n.  'linear': float32, cv2.remap INTER_LINEAR on CV_32FC1 -- the maps quantised to 1/32 pixel exactly
    as for the colour frames, no rounding or saturation of the result.  'nearest': any dtype of 1, 2, 4 or 8 bytes (bool, (u)int8 ... int64,
    float16, bfloat16, float32, float64), cv2.remap INTER_NEAREST, the element copied as bits.  Where the source lies outside the plane, and
    where no cell owns the pixel, the result is `fill` cast to the planes' dtype.  The frames' crop values accumulate in table.crop and the
    clip-level rectangle in `bounds` / table.clip_bounds exactly as `warp` does it, so a planes-only caller gets the rectangle a frames caller
    gets.  Returns the warped planes (the input's dtype and shape)."""
    es = _need_planes(planes, interpolation)
    n, H, W = planes.shape
    if (n, W, H) != (table.n, table.W, table.H):
        raise ValueError(f'planes {tuple(planes.shape)} do not match the cell table (n, H, W) = {(table.n, table.H, table.W)}')
    out = _planes_out(planes, planes.shape, out)
    if bounds is not None:
        _need_bounds(bounds)
    bptr = _ptr(bounds) if bounds is not None else None
    if es == 0:
        _lib.check(_lib_.mf_warp_plane_f32(_ptr(planes), _ptr(out), _ptr(table.buf), n, W, H, table.R, table.C, float(fill),
                                           _ptr(table.crop), bptr, _stream()))
    else:
        _lib.check(_lib_.mf_warp_plane_nearest(_ptr(planes), _ptr(out), _ptr(table.buf), n, W, H, table.R, table.C, es,
                                               _fill_bits(fill, planes.dtype), _ptr(table.crop), bptr, _stream()))
    return out


# BT.601 limited-range red: what the reference's default border, BGR (0, 0, 255), is in Y, U, V
NV12_BORDER_RED = (81, 90, 240)
# ... at 10 bits, in P010's high bits: NV12_BORDER_RED << 8
P010_BORDER_RED = (81 << 8, 90 << 8, 240 << 8)

# One row per semi-planar YUV format -- a luma plane stack and an interleaved chroma one of half the width --: the samples, the format's noun
# in the messages, whether chroma has half the luma rows (4:2:0; else as many: 4:2:2) and the C calls that serve it.
_FormatYuv = collections.namedtuple('_FormatYuv', 'dtype noun border half_rows warp warp_bounds crop_resize crop_resize_dev workspace_bytes')


def _row_yuv(name, dtype, noun, border, half_rows):
    calls = (getattr(_lib_, f'mf_{op}_{name}') for op in ('warp', 'warp_bounds', 'crop_resize', 'crop_resize_dev'))
    return _FormatYuv(dtype, noun, border, half_rows, *calls, getattr(_lib_, f'mf_crop_resize_{name}_workspace_bytes'))


_nv12_border = _border_samples(ctypes.c_uint8, 255, 3)
_p010_border = _border_samples(ctypes.c_uint16, 65535, 3)
_NV12 = _row_yuv('nv12', torch.uint8, 'an NV12', _nv12_border, True)
_P010 = _row_yuv('p010', torch.uint16, 'a P010', _p010_border, True)  # P012 and P016 alike: plain 16-bit samples
_NV16 = _row_yuv('nv16', torch.uint8, 'an NV16', _nv12_border, False)  # 4:2:2 -- what capture cards, SDI / HDMI grabbers and webcams deliver
_P210 = _row_yuv('p210', torch.uint16, 'a P210', _p010_border, False)  # 10-bit 4:2:2 (P212 and P216 alike) -- SDI / HDMI capture, ProRes, XAVC


def _plane_yuv(t, name, shape, device, dtype):
    """One plane stack of a semi-planar or packed YUV clip: a contiguous device tensor of that dtype and of exactly `shape` on `device`."""
    _need(t, dtype, name)
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f'{name} must have shape {tuple(shape)}, got {tuple(t.shape)}')
    if t.device != device:
        raise ValueError(f'{name} must be on the device of y, {device}, got {t.device}')


def _need_yuv(fmt, y, uv, y_name='y', count='n'):
    """Check the (y, uv) pair of a clip of format `fmt` -- W even, H too where chroma rows are halved; returns (n, H, W) of the luma stack.
    y_name, count: what the caller's messages call the luma stack and its length."""
    _need(y, fmt.dtype, y_name)
    if y.dim() != 3:
        raise ValueError(f'{y_name} must be ({count}, H, W) luma planes, got shape {tuple(y.shape)}')
    n, H, W = (int(v) for v in y.shape)
    if fmt.half_rows:
        if W % 2 or H % 2:
            raise ValueError(f'{fmt.noun} frame has an even width and height, got W={W} H={H}')
    elif W % 2:
        raise ValueError(f'{fmt.noun} frame has an even width, got W={W}')
    _plane_yuv(uv, 'uv', (n, H // 2 if fmt.half_rows else H, W // 2, 2), y.device, fmt.dtype)
    return n, H, W


def _out_yuv(fmt, y, y_shape, uv_shape, out):
    """`out` (None: a new pair) checked as an (out_y, out_uv) pair of these shapes beside `y`."""
    if out is None:
        return torch.empty(y_shape, dtype=fmt.dtype, device=y.device), torch.empty(uv_shape, dtype=fmt.dtype, device=y.device)
    if not isinstance(out, (tuple, list)) or len(out) != 2:
        raise ValueError('out must be a pair (out_y, out_uv)')
    out_y, out_uv = out
    _plane_yuv(out_y, 'out_y', y_shape, y.device, fmt.dtype)
    _plane_yuv(out_uv, 'out_uv', uv_shape, y.device, fmt.dtype)
    return out_y, out_uv


def _warp_yuv(fmt, y, uv, table, border_yuv, out, bounds):
    """`warp_nv12` / `warp_p010` / `warp_nv16` / `warp_p210`: the checks, then the format's C call."""
    n, H, W = _need_yuv(fmt, y, uv)
    if (n, W, H) != (table.n, table.W, table.H):
        raise ValueError(f'y {tuple(y.shape)} does not match the cell table (n, H, W) = {(table.n, table.H, table.W)}')
    if len(border_yuv) != 3:
        raise ValueError(f'border_yuv must be (Y, U, V), got {border_yuv!r}')
    out_y, out_uv = _out_yuv(fmt, y, y.shape, uv.shape, out)
    border = fmt.border(border_yuv)
    if bounds is None:
        _lib.check(fmt.warp(_ptr(y), _ptr(uv), _ptr(out_y), _ptr(out_uv), _ptr(table.buf), n, W, H, table.R, table.C, border, _ptr(table.crop),
                            _stream()))
    else:
        _need_bounds(bounds)
        _lib.check(fmt.warp_bounds(_ptr(y), _ptr(uv), _ptr(out_y), _ptr(out_uv), _ptr(table.buf), n, W, H, table.R, table.C, border,
                                   _ptr(table.crop), _ptr(bounds), _stream()))
    return out_y, out_uv


def warp_nv12(y, uv, table, border_yuv=NV12_BORDER_RED, out=None, bounds=None):
    """The mesh warp of an NV12 clip -- the 4:2:0 surfaces decoders and encoders exchange -- from one cell table, without a conversion to BGR and
    back (mf_warp_nv12; the arrays the reference hands to cv2.remap at mfs.py:1063-1069).  y: (n, H, W) uint8 luma, uv: (n, H/2, W/2, 2) uint8
    interleaved chroma, U first; both contiguous device tensors, W and H even, n == table.n.  (Pitched surfaces, or one tensor that holds a
    frame's two planes together, are not taken: one plane stack per tensor.)
    Luma is byte for byte `warp(y, table, (border_yuv[0],))` -- that very launch: the per-frame crop values in table.crop and the clip-level
    rectangle in `bounds` / table.clip_bounds are its.  Chroma is DEFINED as sited at the even luma sample: output chroma sample (cx, cy) takes
    `warp_maps(table)[f, 2 cy, 2 cx]`, halves it in float32 and samples the (H/2, W/2) two-channel plane like cv2.remap's 8-bit INTER_LINEAR with
    BORDER_CONSTANT; where the source lies outside the plane, and where no cell owns the luma pixel, the result is (border_yuv[1], border_yuv[2]).
    No quarter-pixel correction for left- or centre-sited chroma is applied.  (That the definition registers chroma on luma is checked by the
    tests' `second_opinion` module: a float64 sampler of both planes, and a ramp on which chroma must equal the luma of its even pixel.)
    border_yuv: (Y, U, V), each clamp(round(v), 0, 255).  The default (81, 90, 240) is BT.601 limited-range red, i.e. the reference's default
    BGR (0, 0, 255).  out: an (out_y, out_uv) pair to fill.  Returns (out_y, out_uv)."""
    return _warp_yuv(_NV12, y, uv, table, border_yuv, out, bounds)


def warp_p010(y, uv, table, border_yuv=P010_BORDER_RED, out=None, bounds=None):
    """The mesh warp of a P010 clip -- the 4:2:0 layout with 16-bit samples that hardware decoders write for 10-bit and HDR video -- from one
    cell table, without a conversion to 3-channel uint16 and back (mf_warp_p010).  y: (n, H, W) uint16 luma, uv: (n, H/2, W/2, 2) uint16
    interleaved chroma, U first; both contiguous device tensors, W and H even, n == table.n.  Samples are plain 16-bit numbers, 0 .. 65535:
    P010, P012 and P016 differ only in how many low bits a producer leaves zero, so this call serves all three -- and the OUTPUT's low bits
    carry the blend's fraction: nothing is masked.  (Pitched surfaces, or one tensor that holds a frame's two planes together, are not taken.)
    Luma is bit for bit channel 0 of `warp(stack(y, y, y), table, (b, b, b))`, b = border_yuv[0] -- cv2.remap's CV_16U arithmetic on one
    channel; the per-frame crop values in table.crop and the clip-level rectangle in `bounds` / table.clip_bounds are that call's.  Chroma is
    sited at the even luma sample, as in `warp_nv12`: output chroma sample (cx, cy) takes `warp_maps(table)[f, 2 cy, 2 cx]`, halves it in
    float32 and samples the (H/2, W/2) two-channel plane with the same CV_16U arithmetic per channel; where the source lies outside the plane,
    and where no cell owns the luma pixel, the result is (border_yuv[1], border_yuv[2]).  (Checked for consistency with luma by the tests'
    `second_opinion` module, as for `warp_nv12`.)
    border_yuv: (Y, U, V), each clamp(round(v), 0, 65535).  The default (20736, 23040, 61440) is BT.601 limited-range red at 10 bits in P010's
    high bits.  out: an (out_y, out_uv) pair to fill.  Returns (out_y, out_uv)."""
    return _warp_yuv(_P010, y, uv, table, border_yuv, out, bounds)


# the two packed byte orders of 4:2:2 (the semi-planar form is the NV16 pair)
ORDERS_422 = {'yuyv': 0, 'uyvy': 1}


def _order_422(order):
    if order not in ORDERS_422:
        raise ValueError(f"order must be 'yuyv' or 'uyvy', got {order!r}")
    return ORDERS_422[order]


def _need_packed_422(packed, name='packed'):
    """A packed 4:2:2 clip: a contiguous (n, H, W, 2) uint8 device tensor with W even; returns (n, H, W)."""
    _need(packed, torch.uint8, name)
    if packed.dim() != 4 or packed.shape[3] != 2:
        raise ValueError(f'{name} must be (n, H, W, 2) packed 4:2:2 frames, got shape {tuple(packed.shape)}')
    n, H, W = (int(v) for v in packed.shape[:3])
    if W % 2:
        raise ValueError(f'a packed 4:2:2 frame has an even width, got W={W}')
    if n < 1 or H < 1 or W < 2:
        raise ValueError(f'{name} is empty: shape {tuple(packed.shape)}')
    return n, H, W


def warp_nv16(y, uv, table, border_yuv=NV12_BORDER_RED, out=None, bounds=None):
    """The mesh warp of an NV16 clip -- 4:2:2 in its semi-planar form, what capture cards and grabbers deliver (their packed forms go through
    `warp_packed_422`) -- from one cell table, without a conversion to BGR and without dropping chroma rows (mf_warp_nv16).  y: (n, H, W) uint8
    luma, uv: (n, H, W/2, 2) uint8 interleaved chroma, U first; both contiguous device tensors, W even, H of either parity, n == table.n.
    Luma is byte for byte `warp(y, table, (border_yuv[0],))` -- that very launch: the per-frame crop values in table.crop and the clip-level
    rectangle in `bounds` / table.clip_bounds are its.  Chroma is DEFINED as sited at the even luma sample of the same row: output chroma
    sample (cx, y) takes `warp_maps(table)[f, y, 2 cx]`, halves its x in float32, leaves its y as it is, and samples the (H, W/2) two-channel
    plane like cv2.remap's 8-bit INTER_LINEAR with BORDER_CONSTANT; where the source lies outside the plane, and where no cell owns the luma
    pixel, the result is (border_yuv[1], border_yuv[2]).  No sub-pixel correction for other chroma sitings is applied.
    border_yuv: (Y, U, V), each clamp(round(v), 0, 255); the default is `warp_nv12`'s.  out: an (out_y, out_uv) pair to fill.  Returns
    (out_y, out_uv).  The next step on the path is `crop_resize_nv16`.  (10-bit 4:2:2 is `warp_p210`.)"""
    return _warp_yuv(_NV16, y, uv, table, border_yuv, out, bounds)


def unpack_422(packed, order='yuyv', out=None):
    """A packed 4:2:2 clip as the NV16 pair (mf_unpack_422_u8).  packed: a contiguous (n, H, W, 2) uint8 device tensor, W even -- a flat stream
    of 4-byte words, Y0 U Y1 V for order 'yuyv' (YUY2) and U Y0 V Y1 for 'uyvy' (2vuy).  Returns (y, uv): (n, H, W) luma and (n, H, W/2, 2)
    chroma, U first -- what `warp_nv16` takes, and y is what `estimate_motion` takes.  out: a (y, uv) pair to fill.  One streaming kernel,
    2 bytes moved per byte of the clip."""
    n, H, W = _need_packed_422(packed)
    o = _order_422(order)
    y, uv = _out_yuv(_NV16, packed, (n, H, W), (n, H, W // 2, 2), out)
    _lib.check(_lib_.mf_unpack_422_u8(_ptr(packed), _ptr(y), _ptr(uv), n, W, H, o, _stream()))
    return y, uv


def pack_422(y, uv, order='yuyv', out=None):
    """The inverse of `unpack_422` (mf_pack_422_u8): the NV16 pair y (n, H, W), uv (n, H, W/2, 2) as a packed (n, H, W, 2) uint8 clip of the
    given byte order.  out: the packed tensor to fill.  Returns it."""
    n, H, W = _need_yuv(_NV16, y, uv)
    o = _order_422(order)
    if out is None:
        out = torch.empty((n, H, W, 2), dtype=torch.uint8, device=y.device)
    else:
        _plane_yuv(out, 'out', (n, H, W, 2), y.device, torch.uint8)
    if n < 1 or H < 1 or W < 2:
        raise ValueError(f'y is empty: shape {tuple(y.shape)}')
    _lib.check(_lib_.mf_pack_422_u8(_ptr(y), _ptr(uv), _ptr(out), n, W, H, o, _stream()))
    return out


def warp_packed_422(packed, table, order='yuyv', border_yuv=NV12_BORDER_RED, out=None, bounds=None):
    """The mesh warp of a packed 4:2:2 clip (YUY2 / UYVY), DEFINED as `unpack_422`, `warp_nv16`, `pack_422`: four launches beside the luma's
    own (unpack, the grey warp, the chroma warp, pack).  packed: (n, H, W, 2) uint8, n == table.n; out: the packed tensor to fill.  The crop
    values and the rectangle are `warp_nv16`'s.  Temporary memory: the unpacked pair and its warped twin, 2 n W H bytes each -- twice the
    clip's own size, released on return.  (A tail that reads and writes the packed words directly is not built; profiles/nv16.md has the
    measurement that decides whether it is worth one.)  Returns the warped packed clip."""
    n, H, W = _need_packed_422(packed)
    _order_422(order)
    if out is not None:
        _plane_yuv(out, 'out', (n, H, W, 2), packed.device, torch.uint8)
    if (n, W, H) != (table.n, table.W, table.H):
        raise ValueError(f'packed {tuple(packed.shape)} does not match the cell table (n, H, W) = {(table.n, table.H, table.W)}')
    if len(border_yuv) != 3:
        raise ValueError(f'border_yuv must be (Y, U, V), got {border_yuv!r}')
    if bounds is not None:
        _need_bounds(bounds)
    y, uv = unpack_422(packed, order)
    out_y, out_uv = warp_nv16(y, uv, table, border_yuv, None, bounds)
    return pack_422(out_y, out_uv, order, out)


def warp_p210(y, uv, table, border_yuv=P010_BORDER_RED, out=None, bounds=None):
    """The mesh warp of a P210 clip -- 10-bit 4:2:2 in its semi-planar form, what SDI / HDMI capture and ProRes / XAVC decoders deliver (the
    packed form, Y210 / Y216, goes through `warp_y210`) -- from one cell table, without truncating to 8 bits or converting to 3-channel uint16
    (mf_warp_p210).  y: (n, H, W) uint16 luma, uv: (n, H, W/2, 2) uint16 interleaved chroma, U first; both contiguous device tensors, W even,
    H of either parity, n == table.n.  Samples are plain 16-bit numbers, nothing is masked: P210, P212 and P216 alike.
    Luma is bit for bit `warp_p010`'s luma -- that very launch: the per-frame crop values in table.crop and the clip-level rectangle in
    `bounds` / table.clip_bounds are its.  Chroma is sited at the even luma sample of the same row, as in `warp_nv16`: output chroma sample
    (cx, y) takes `warp_maps(table)[f, y, 2 cx]`, halves its x in float32, leaves its y as it is, and samples the (H, W/2) two-channel plane
    with `warp_p010`'s CV_16U arithmetic per channel; where the 2 x 2 taps lie wholly outside the plane, and where no cell owns the luma
    pixel, the result is (border_yuv[1], border_yuv[2]) itself.
    border_yuv: (Y, U, V), each clamp(round(v), 0, 65535); the default is `warp_p010`'s.  out: an (out_y, out_uv) pair to fill.  Returns
    (out_y, out_uv).  The next step on the path is `crop_resize_p210`.  (Not provided: v210 -- three 10-bit samples per 32-bit word --,
    kernels that warp the packed words directly, the host and clip pipelines.)"""
    return _warp_yuv(_P210, y, uv, table, border_yuv, out, bounds)


def _need_y210(packed, name='packed'):
    """A packed Y210 / Y216 clip: a contiguous (n, H, W, 2) uint16 device tensor with W even; returns (n, H, W)."""
    _need(packed, torch.uint16, name)
    if packed.dim() != 4 or packed.shape[3] != 2:
        raise ValueError(f'{name} must be (n, H, W, 2) packed Y210 frames, got shape {tuple(packed.shape)}')
    n, H, W = (int(v) for v in packed.shape[:3])
    if W % 2:
        raise ValueError(f'a packed Y210 frame has an even width, got W={W}')
    if n < 1 or H < 1 or W < 2:
        raise ValueError(f'{name} is empty: shape {tuple(packed.shape)}')
    return n, H, W


def unpack_y210(packed, out=None):
    """A packed Y210 / Y216 clip as the P210 pair (mf_unpack_y210_u16).  packed: a contiguous (n, H, W, 2) uint16 device tensor, W even, its
    storage 8-byte aligned -- a flat stream of 8-byte words Y0 U Y1 V.  Samples move as bits; nothing is masked or shifted.  Returns (y, uv):
    (n, H, W) luma and (n, H, W/2, 2) chroma, U first -- what `warp_p210` takes.  out: a (y, uv) pair to fill.  One streaming kernel.  (v210 is
    not this layout and is not provided.)"""
    n, H, W = _need_y210(packed)
    y, uv = _out_yuv(_P210, packed, (n, H, W), (n, H, W // 2, 2), out)
    _lib.check(_lib_.mf_unpack_y210_u16(_ptr(packed), _ptr(y), _ptr(uv), n, W, H, _stream()))
    return y, uv


def pack_y210(y, uv, out=None):
    """The inverse of `unpack_y210` (mf_pack_y210_u16): the P210 pair y (n, H, W), uv (n, H, W/2, 2) as a packed (n, H, W, 2) uint16 clip.
    out: the packed tensor to fill (8-byte aligned).  Returns it."""
    n, H, W = _need_yuv(_P210, y, uv)
    if out is None:
        out = torch.empty((n, H, W, 2), dtype=torch.uint16, device=y.device)
    else:
        _plane_yuv(out, 'out', (n, H, W, 2), y.device, torch.uint16)
    if n < 1 or H < 1 or W < 2:
        raise ValueError(f'y is empty: shape {tuple(y.shape)}')
    _lib.check(_lib_.mf_pack_y210_u16(_ptr(y), _ptr(uv), _ptr(out), n, W, H, _stream()))
    return out


def warp_y210(packed, table, border_yuv=P010_BORDER_RED, out=None, bounds=None):
    """The mesh warp of a packed Y210 / Y216 clip, DEFINED as `unpack_y210`, `warp_p210`, `pack_y210`.  packed: (n, H, W, 2) uint16,
    n == table.n; out: the packed tensor to fill.  The crop values and the rectangle are `warp_p210`'s.  Temporary memory: the unpacked pair
    and its warped twin, released on return.  (A tail that reads and writes the packed words directly is not built; profiles/p210.md.)
    Returns the warped packed clip."""
    n, H, W = _need_y210(packed)
    if out is not None:
        _plane_yuv(out, 'out', (n, H, W, 2), packed.device, torch.uint16)
    if (n, W, H) != (table.n, table.W, table.H):
        raise ValueError(f'packed {tuple(packed.shape)} does not match the cell table (n, H, W) = {(table.n, table.H, table.W)}')
    if len(border_yuv) != 3:
        raise ValueError(f'border_yuv must be (Y, U, V), got {border_yuv!r}')
    if bounds is not None:
        _need_bounds(bounds)
    y, uv = unpack_y210(packed)
    out_y, out_uv = warp_p210(y, uv, table, border_yuv, None, bounds)
    return pack_y210(out_y, out_uv, out)


def _even_output_size(size, name='size'):
    """`check_output_size` for an NV12 output: both numbers even as well (the smallest is 2 x 2)."""
    oW, oH = check_output_size(size, name)
    if oW % 2 or oH % 2:
        raise ValueError(f'an NV12 output has an even width and height, got {name}={(oW, oH)}')
    return oW, oH


def _yuv_output_size(fmt, size, name='size'):
    """`check_output_size` for an output of format `fmt`: an even width, and an even height too where chroma rows are halved."""
    if fmt.half_rows:
        return _even_output_size(size, name)
    oW, oH = check_output_size(size, name)
    if oW % 2:
        raise ValueError(f'{fmt.noun} output has an even width, got {name}={(oW, oH)}')
    return oW, oH


def _crop_resize_yuv(fmt, y, uv, bounds, size, out, status):
    """`crop_resize_nv12` / `crop_resize_p010` / `crop_resize_nv16` / `crop_resize_p210`: the checks, then the format's C call for a host or a
    device rectangle."""
    n, H, W = _need_yuv(fmt, y, uv)
    oW, oH = (W, H) if size is None else _yuv_output_size(fmt, size)
    resident = _device_rectangle(bounds, status)
    out_y, out_uv = _out_yuv(fmt, y, (n, oH, oW), (n, oH // 2 if fmt.half_rows else oH, oW // 2, 2), out)
    if resident:
        status = _status_for(status, y.device)
    work = torch.empty(fmt.workspace_bytes(oW, oH), dtype=torch.uint8, device=y.device)
    if not resident:
        left, top, right, bottom = (int(v) for v in bounds)
        _lib.check(fmt.crop_resize(_ptr(y), _ptr(uv), _ptr(out_y), _ptr(out_uv), n, W, H, left, top, right, bottom, oW, oH, _ptr(work), _stream()))
        return out_y, out_uv
    _lib.check(fmt.crop_resize_dev(_ptr(y), _ptr(uv), _ptr(out_y), _ptr(out_uv), n, W, H, _ptr(bounds), oW, oH, _ptr(work), _ptr(status),
                                   _stream()))
    return out_y, out_uv, status


def crop_resize_nv12(y, uv, bounds, size=None, out=None, status=None):
    """`crop_resize` for an NV12 clip (mfs.py:1111-1157 without a conversion to BGR and back; mf_crop_resize_nv12 / mf_crop_resize_dev_nv12):
    crop to the inclusive {left, top, right, bottom} -- in luma pixels, of any parity -- and scale to `size` = (width, height), even, by default
    back to (W, H).  y, uv as in `warp_nv12`.  bounds: a 4-tuple the host knows, or an int32[4] DEVICE tensor (what `stabilized_nv12` returns)
    that the kernels read when they execute -- the host never reads it and the call never waits; the bytes are the same.
    Luma is byte for byte `crop_resize(y, bounds, size=size)` (`crop_resize_resident` for a device rectangle) -- that very launch.  Chroma is
    DEFINED as sited at the even luma sample: output chroma sample cx takes the luma source position of output luma pixel 2 cx, made absolute in
    the frame and halved, clamped to the chroma samples whose siting luma pixel lies inside the crop, and cv2.resize's 8-bit INTER_LINEAR
    arithmetic per channel (include/meshflow_hip.h has every expression).  The full frame at its own size is a copy.
    (The definition's consistency with luma -- positions, parity, clamp range -- is checked by the tests' `second_opinion` module against
    float64 positions of its own.)
    out: an (out_y, out_uv) pair to fill.  status (device rectangle only): as in `crop_resize_resident` -- an int32[1] device tensor, the
    caller's (it accumulates) or a new zeroed one, that an unusable rectangle adds exactly 1 to, leaving both outputs untouched.
    Returns (out_y, out_uv), or (out_y, out_uv, status) for a device rectangle."""
    return _crop_resize_yuv(_NV12, y, uv, bounds, size, out, status)


def crop_resize_p010(y, uv, bounds, size=None, out=None, status=None):
    """`crop_resize_nv12` for a P010 clip (mfs.py:1111-1157 without a conversion to 3-channel uint16 and back; mf_crop_resize_p010 /
    mf_crop_resize_dev_p010): crop to the inclusive {left, top, right, bottom} -- in luma pixels, of any parity -- and scale to `size` = (width,
    height), even, by default back to (W, H).  y, uv as in `warp_p010`: uint16, plain 16-bit numbers, nothing masked.  bounds: a 4-tuple the
    host knows, or an int32[4] DEVICE tensor (what `stabilized_p010` returns) that the kernels read when they execute -- the host never reads
    it and the call never waits; the bits are the same.
    Luma is bit for bit channel 0 of `crop_resize(stack(y, y, y), bounds, size=size)` (`crop_resize_resident` for a device rectangle):
    cv2.resize's float path on CV_16UC1, and INTER_AREA's (S00 + S01 + S10 + S11 + 2) >> 2 where the crop is exactly twice the output in both
    axes.  Chroma is sited at the even luma sample with `crop_resize_nv12`'s positions and clamps and the same float arithmetic per channel,
    weights (1 - f, f) in float32 -- no 2048 quantisation and no area branch (include/meshflow_hip.h has every expression).  The full frame at
    its own size is a copy.  (Checked for consistency with luma by the tests' `second_opinion` module, as for `crop_resize_nv12`.)
    out: an (out_y, out_uv) pair to fill.  status (device rectangle only): as in `crop_resize_resident` -- an int32[1] device tensor, the
    caller's (it accumulates) or a new zeroed one, that an unusable rectangle adds exactly 1 to, leaving both outputs untouched.
    Returns (out_y, out_uv), or (out_y, out_uv, status) for a device rectangle."""
    return _crop_resize_yuv(_P010, y, uv, bounds, size, out, status)


def crop_resize_nv16(y, uv, bounds, size=None, out=None, status=None):
    """`crop_resize_nv12` for an NV16 (4:2:2) clip (mfs.py:1111-1157 without a conversion to BGR and without dropping chroma rows;
    mf_crop_resize_nv16 / mf_crop_resize_dev_nv16): crop to the inclusive {left, top, right, bottom} -- in luma pixels, of any parity -- and scale
    to `size` = (width, height), the width even and the height of either parity, by default back to (W, H).  y, uv as in `warp_nv16`.  bounds: a
    4-tuple the host knows, or an int32[4] DEVICE tensor (what `stabilized_nv16` returns) that the kernels read when they execute -- the host
    never reads it and the call never waits; the bytes are the same.
    Luma is byte for byte `crop_resize(y, bounds, size=size)` (`crop_resize_resident` for a device rectangle) -- that very launch.  Chroma, x
    axis: `crop_resize_nv12`'s -- sited at the even luma sample, the luma source position of output luma pixel 2 cx made absolute in the frame
    and halved, clamped to the chroma samples whose siting luma pixel lies inside the crop.  Chroma, y axis: chroma has luma's rows, so output
    chroma row y takes the luma table's own rows and weights for row y.  cv2.resize's 8-bit INTER_LINEAR arithmetic per channel
    (include/meshflow_hip.h has every expression).  The full frame at its own size is a copy, and so is an even-`left` rectangle at its own size.
    out: an (out_y, out_uv) pair to fill, (n, height, width) and (n, height, width/2, 2).  status (device rectangle only): as in
    `crop_resize_resident` -- an int32[1] device tensor, the caller's (it accumulates) or a new zeroed one, that an unusable rectangle adds
    exactly 1 to, leaving both outputs untouched.
    Returns (out_y, out_uv), or (out_y, out_uv, status) for a device rectangle."""
    return _crop_resize_yuv(_NV16, y, uv, bounds, size, out, status)


def crop_resize_packed_422(packed, bounds, order='yuyv', size=None, out=None, status=None):
    """`crop_resize_nv16` for a packed 4:2:2 clip (YUY2 / UYVY), DEFINED as `unpack_422`, `crop_resize_nv16`, `pack_422`.  packed: (n, H, W, 2)
    uint8; bounds, size and status as in `crop_resize_nv16`; out: the packed (n, height, width, 2) tensor to fill.  Temporary memory: the
    unpacked pair and its resized twin, released on return.  (A kernel that crops the packed words directly is not built;
    profiles/nv16_crop.md has the measurement that decides whether it is worth one.)
    Returns the packed clip, or (packed clip, status) for a device rectangle."""
    n, H, W = _need_packed_422(packed)
    _order_422(order)
    oW, oH = (W, H) if size is None else _yuv_output_size(_NV16, size)
    if out is not None:
        _plane_yuv(out, 'out', (n, oH, oW, 2), packed.device, torch.uint8)
    _device_rectangle(bounds, status)
    y, uv = unpack_422(packed, order)
    res = crop_resize_nv16(y, uv, bounds, (oW, oH), None, status)
    out = pack_422(res[0], res[1], order, out)
    return out if len(res) == 2 else (out, res[2])


def crop_resize_p210(y, uv, bounds, size=None, out=None, status=None):
    """`crop_resize_nv16` for a P210 (10-bit 4:2:2) clip (mf_crop_resize_p210 / mf_crop_resize_dev_p210): crop to the inclusive {left, top,
    right, bottom} -- in luma pixels, of any parity -- and scale to `size` = (width, height), the width even and the height of either parity,
    by default back to (W, H).  y, uv as in `warp_p210`: uint16, plain 16-bit numbers, nothing masked.  bounds: a 4-tuple the host knows, or an
    int32[4] DEVICE tensor (what `stabilized_p210` returns) that the kernels read when they execute.
    Luma is bit for bit `crop_resize_p010`'s luma -- that very launch: cv2.resize's float path on CV_16UC1, and INTER_AREA's box where the crop
    is exactly twice the output in both axes.  Chroma, x axis: `crop_resize_p010`'s -- sited at the even luma sample, float32 weights (1 - f, f).
    Chroma, y axis: chroma has luma's rows, so output chroma row y takes the luma table's own rows and fraction for row y.  The same float
    arithmetic per channel; NO area branch for chroma, also at exactly 2x where luma takes the box (include/meshflow_hip.h has every
    expression).  The full frame at its own size is a copy.
    out: an (out_y, out_uv) pair to fill, (n, height, width) and (n, height, width/2, 2).  status (device rectangle only): as in
    `crop_resize_resident`.  Returns (out_y, out_uv), or (out_y, out_uv, status) for a device rectangle."""
    return _crop_resize_yuv(_P210, y, uv, bounds, size, out, status)


def crop_resize_y210(packed, bounds, size=None, out=None, status=None):
    """`crop_resize_p210` for a packed Y210 / Y216 clip, DEFINED as `unpack_y210`, `crop_resize_p210`, `pack_y210`.  packed: (n, H, W, 2)
    uint16; bounds, size and status as in `crop_resize_p210`; out: the packed (n, height, width, 2) tensor to fill.  Temporary memory: the
    unpacked pair and its resized twin, released on return.  (A kernel that crops the packed words directly is not built.)
    Returns the packed clip, or (packed clip, status) for a device rectangle."""
    n, H, W = _need_y210(packed)
    oW, oH = (W, H) if size is None else _yuv_output_size(_P210, size)
    if out is not None:
        _plane_yuv(out, 'out', (n, oH, oW, 2), packed.device, torch.uint16)
    _device_rectangle(bounds, status)
    y, uv = unpack_y210(packed)
    res = crop_resize_p210(y, uv, bounds, (oW, oH), None, status)
    out = pack_y210(res[0], res[1], out)
    return out if len(res) == 2 else (out, res[2])


def crop_resize_planes(planes, bounds, interpolation='linear', size=None, out=None, status=None):
    """`crop_resize` for side planes (mfs.py:1111-1157 on a plane; mf_crop_resize_plane_* / mf_crop_resize_dev_plane_*): crop to the inclusive
    {left, top, right, bottom} and scale to `size` = (width, height), by default back to (W, H).  planes and interpolation as in
    `warp_planes`: 'linear' is cv2.resize INTER_LINEAR on CV_32FC1 (a crop exactly twice the output in both axes takes INTER_AREA's fast
    path, as cv2 does), 'nearest' cv2.resize INTER_NEAREST with the element copied as bits.  bounds: a 4-tuple the host knows, or an int32[4]
    DEVICE tensor (what `warp_clip`, `stabilize_resident`, `stabilized_planes` return) that the kernels read when they execute -- the host
    never reads it and the call never waits; the bytes are the same.  status (device rectangle only): as in `crop_resize_resident` -- an
    int32[1] device tensor, the caller's (it accumulates) or a new zeroed one, that an unusable rectangle adds 1 to, leaving `out` untouched.
    Returns the planes (n, height, width), or (planes, status) for a device rectangle."""
    es = _need_planes(planes, interpolation)
    n, H, W = planes.shape
    oW, oH = (W, H) if size is None else check_output_size(size)
    resident = _device_rectangle(bounds, status)
    out = _planes_out(planes, (n, oH, oW), out)
    work = torch.empty(_lib_.mf_crop_resize_workspace_bytes(oW, oH), dtype=torch.uint8, device=planes.device)
    if not resident:
        left, top, right, bottom = (int(v) for v in bounds)
        if es == 0:
            _lib.check(_lib_.mf_crop_resize_plane_f32(_ptr(planes), _ptr(out), n, W, H, left, top, right, bottom, oW, oH, _ptr(work), _stream()))
        else:
            _lib.check(_lib_.mf_crop_resize_plane_nearest(_ptr(planes), _ptr(out), n, W, H, left, top, right, bottom, oW, oH, es, _ptr(work),
                                                          _stream()))
        return out
    status = _status_for(status, planes.device)
    if es == 0:
        _lib.check(_lib_.mf_crop_resize_dev_plane_f32(_ptr(planes), _ptr(out), n, W, H, _ptr(bounds), oW, oH, _ptr(work), _ptr(status), _stream()))
    else:
        _lib.check(_lib_.mf_crop_resize_dev_plane_nearest(_ptr(planes), _ptr(out), n, W, H, _ptr(bounds), oW, oH, es, _ptr(work), _ptr(status),
                                                          _stream()))
    return out, status


def track_subframe_grid(W, H, sub_rows, sub_cols):
    """(sub_w, sub_h, columns, rows) of the sub-frame grid of mfs.py:493-504: ceil-sized sub-frames, possibly fewer than sub_rows x sub_cols.
    Sub-frame s = column * rows + row (left outer, top inner) starts at (column * sub_w, row * sub_h)."""
    sub_rows, sub_cols = int(sub_rows), int(sub_cols)
    if sub_rows < 1 or sub_cols < 1 or sub_rows > H or sub_cols > W:
        raise ValueError(f'sub_rows must be in 1 .. H and sub_cols in 1 .. W (got {sub_rows} x {sub_cols} for {W} x {H})')
    sub_w, sub_h = -(-W // sub_cols), -(-H // sub_rows)
    return sub_w, sub_h, -(-W // sub_w), -(-H // sub_h)


def _need_grey(t, name):
    _need(t, torch.uint8, name)
    if t.dim() != 3 or t.shape[0] < 1:
        raise ValueError(f'{name} must have shape (n, H, W): one-channel uint8 images (got {tuple(t.shape)})')


LUMA_MAX_DIM = 32767
# (dtype, dimensions, channels) of a clip `luma` converts -> (its C call, whether the call takes red_first)
_LUMA_CALLS = {(torch.uint8, 4, 3): (_lib_.mf_luma_u8c3, True), (torch.uint8, 4, 4): (_lib_.mf_luma_u8c4, True),
               (torch.uint16, 4, 3): (_lib_.mf_luma_u16c3, True), (torch.uint16, 3, 1): (_lib_.mf_luma_u16, False)}


def luma_source(frames):
    """The key of `_LUMA_CALLS` for a clip `luma` converts, or None: (n, H, W, 3) uint8 / uint16, (n, H, W, 4) uint8, (n, H, W) uint16."""
    if not isinstance(frames, torch.Tensor) or frames.dim() not in (3, 4):
        return None
    key = (frames.dtype, frames.dim(), int(frames.shape[3]) if frames.dim() == 4 else 1)
    return key if key in _LUMA_CALLS else None


def luma(frames, red_first=False, out=None):
    """The luma of a resident clip as a (n, H, W) uint8 stack -- what `fast_corners`, `lk_track` and the device tracker take -- bit for bit
    tests/luma_model.py.  frames: (n, H, W, 3) uint8 BGR or (n, H, W, 4) uint8 BGRA (OpenCV's 8U COLOR_BGR2GRAY: (b*3735 + g*19235 + r*9798
    + 16384) >> 15; alpha is ignored), (n, H, W, 3) uint16 BGR (OpenCV's 16U arithmetic, then the high byte) or (n, H, W) uint16, the luma
    plane of a P010 clip (the high byte); 16-bit values are truncated, not rounded.  red_first: channel 0 is red (RGB / RGBA).  A (n, H, W)
    uint8 stack is luma already and is refused: pass it on as it is.  out: a contiguous (n, H, W) uint8 tensor on the device of frames that
    does not overlap them.  One launch per 2^28 pixels on torch's current stream; does not wait for it."""
    name = 'luma'
    if not isinstance(frames, torch.Tensor):
        raise ValueError(f'{name}: frames must be a CUDA/HIP torch tensor')
    if frames.dtype == torch.uint8 and frames.dim() == 3:
        raise ValueError(f'{name}: a (n, H, W) uint8 stack is already luma: pass it to the tracker as it is')
    key = luma_source(frames)
    if key is None:
        raise ValueError(f'{name}: frames must be (n, H, W, 3) uint8 or uint16, (n, H, W, 4) uint8 or (n, H, W) uint16 '
                         f'(got {tuple(frames.shape)} {frames.dtype})')
    n, H, W = (int(v) for v in frames.shape[:3])
    if n < 1 or not 1 <= H <= LUMA_MAX_DIM or not 1 <= W <= LUMA_MAX_DIM:
        raise ValueError(f'{name}: frames need n >= 1 and H, W in 1 .. {LUMA_MAX_DIM} (got {tuple(frames.shape)})')
    if red_first not in (False, True):
        raise ValueError(f'{name}: red_first must be False or True (got {red_first!r})')
    call, takes_order = _LUMA_CALLS[key]
    if red_first and not takes_order:
        raise ValueError(f'{name}: red_first has no meaning for a one-channel (n, H, W) uint16 plane')
    _need(frames, frames.dtype, 'frames')
    if out is None:
        out = torch.empty((n, H, W), dtype=torch.uint8, device=frames.device)
    else:
        _need(out, torch.uint8, 'out')
        if tuple(out.shape) != (n, H, W) or out.device != frames.device:
            raise ValueError(f'{name}: out must have shape {(n, H, W)} on the device of frames (got {tuple(out.shape)} on {out.device})')
    order = (int(bool(red_first)),) if takes_order else ()
    _lib.check(call(_ptr(frames), n, W, H, *order, _ptr(out), _stream()))
    return out


def _track_work(n, W, H, sub_rows, sub_cols, max_per_subframe, device):
    size = _lib_.mf_track_workspace_bytes(n, W, H, sub_rows, sub_cols, max_per_subframe)
    if size == 0:                                  # outside the limits: let the call itself say which
        size = 16
    return torch.empty(size, dtype=torch.uint8, device=device)


def fast_corners(grey, sub_rows, sub_cols, max_per_subframe=1024, threshold=10):
    """FAST corners (cv2.FastFeatureDetector_create() defaults: TYPE_9_16, non-maximum suppression) of every sub-frame of every image of a
    (n, H, W) uint8 stack, each sub-frame an image of its own (mfs.py:505-516, 613).  Returns (points (n, S, max_per_subframe, 2) float32 --
    (x, y) relative to the sub-frame, row-major order, zeros behind a sub-frame's corners --, counts (n, S) int32 -- the TRUE number of
    corners --, status (n, S) int32 -- bit _lib.TRACK_OVERFLOW where the count exceeds max_per_subframe and only the first ones were kept).
    S and the sub-frames' order: `track_subframe_grid`."""
    _need_grey(grey, 'grey')
    n, H, W = grey.shape
    _, _, cols, rows = track_subframe_grid(W, H, sub_rows, sub_cols)
    max_per_subframe = int(max_per_subframe)
    if not 1 <= max_per_subframe <= _lib.TRACK_MAX_PER_SUBFRAME:
        raise ValueError(f'max_per_subframe must be in 1 .. {_lib.TRACK_MAX_PER_SUBFRAME} (got {max_per_subframe})')
    dev = grey.device
    points = torch.zeros((n, cols * rows, max_per_subframe, 2), dtype=torch.float32, device=dev)
    counts = torch.empty((n, cols * rows), dtype=torch.int32, device=dev)
    status = torch.empty((n, cols * rows), dtype=torch.int32, device=dev)
    work = _track_work(n, W, H, int(sub_rows), int(sub_cols), max_per_subframe, dev)
    _lib.check(_lib_.mf_fast_corners_u8(_ptr(grey), n, W, H, int(sub_rows), int(sub_cols), max_per_subframe, int(threshold), _ptr(points),
                                        _ptr(counts), _ptr(status), _ptr(work), _stream()))
    return points, counts, status


def lk_track(early, late, points, counts, sub_rows, sub_cols):
    """Pyramidal Lucas-Kanade (cv2.calcOpticalFlowPyrLK defaults) of `fast_corners`' points from the (n, H, W) uint8 stack `early` into `late`,
    sub-frame by sub-frame.  Returns (moved (n, S, max_per_subframe, 2) float32, found (n, S, max_per_subframe) uint8 = cv2's status), zeros
    behind a sub-frame's corners.  The adjacent pairs of a clip: early = clip[:-1], late = clip[1:]."""
    _need_grey(early, 'early')
    _need_grey(late, 'late')
    if early.shape != late.shape or early.device != late.device:
        raise ValueError(f'early and late must have the same shape and device (got {tuple(early.shape)} and {tuple(late.shape)})')
    n, H, W = early.shape
    _, _, cols, rows = track_subframe_grid(W, H, sub_rows, sub_cols)
    _need(points, torch.float32, 'points')
    _need(counts, torch.int32, 'counts')
    if points.dim() != 4 or points.shape[:2] != (n, cols * rows) or points.shape[3] != 2 or points.shape[2] < 1:
        raise ValueError(f'points must have shape (n, S, max_per_subframe, 2) = ({n}, {cols * rows}, *, 2), got {tuple(points.shape)}')
    if counts.shape != (n, cols * rows):
        raise ValueError(f'counts must have shape (n, S) = ({n}, {cols * rows}), got {tuple(counts.shape)}')
    max_per_subframe = points.shape[2]
    dev = early.device
    moved = torch.zeros((n, cols * rows, max_per_subframe, 2), dtype=torch.float32, device=dev)
    found = torch.zeros((n, cols * rows, max_per_subframe), dtype=torch.uint8, device=dev)
    work = _track_work(n, W, H, int(sub_rows), int(sub_cols), max_per_subframe, dev)
    _lib.check(_lib_.mf_lk_track_u8(_ptr(early), _ptr(late), n, W, H, int(sub_rows), int(sub_cols), max_per_subframe, _ptr(points),
                                    _ptr(counts), _ptr(moved), _ptr(found), _ptr(work), _stream()))
    return moved, found


def _need_tracks(points, moved, name):
    """points / moved (n, S, max_per_subframe, 2) float32 on one device: (n, S, max_per_subframe)."""
    _need(points, torch.float32, 'points')
    _need(moved, torch.float32, 'moved')
    if points.dim() != 4 or points.shape[3] != 2 or min(points.shape[:3]) < 1:
        raise ValueError(f'{name}: points must have shape (n, S, max_per_subframe, 2), got {tuple(points.shape)}')
    if moved.shape != points.shape or moved.device != points.device:
        raise ValueError(f'{name}: moved must have the shape and device of points (got {tuple(moved.shape)} and {tuple(points.shape)})')
    return tuple(points.shape[:3])


def _need_like(t, dtype, shape, device, what, name):
    _need(t, dtype, what)
    if tuple(t.shape) != tuple(shape) or t.device != device:
        raise ValueError(f'{name}: {what} must have shape {tuple(shape)} on the device of points (got {tuple(t.shape)})')


def ransac_inliers(points, counts, moved, found, min_features=4, threshold=3.0, confidence=0.995, max_iters=2000, seed=0):
    """The outlier step per sub-frame on the device (mfs.py:564-579, 614, 626), bit for bit tests/ransac_model.py: `fast_corners`' points and
    counts, `lk_track`'s moved and found.  Returns (inlier (n, S, max_per_subframe) uint8 -- 1 for the candidates in the best hypothesis'
    consensus set --, info (n, S, 4) int32 -- (status, candidates, inliers, iterations run), status _lib.RANSAC_OK / RANSAC_TOO_FEW /
    RANSAC_NO_CONSENSUS)."""
    name = 'ransac_inliers'
    n, S, max_per_subframe = _need_tracks(points, moved, name)
    dev = points.device
    _need_like(counts, torch.int32, (n, S), dev, 'counts', name)
    _need_like(found, torch.uint8, (n, S, max_per_subframe), dev, 'found', name)
    seed = int(seed)
    if not 0 <= seed < 1 << 32:
        raise ValueError(f'{name}: seed must be in 0 .. 2^32 - 1 (got {seed})')
    inlier = torch.empty((n, S, max_per_subframe), dtype=torch.uint8, device=dev)
    info = torch.empty((n, S, 4), dtype=torch.int32, device=dev)
    size = _lib_.mf_ransac_workspace_bytes(n, S, max_per_subframe)
    work = torch.empty(size if size else 16, dtype=torch.uint8, device=dev)      # (0: outside the limits -- let the call itself say which)
    _lib.check(_lib_.mf_ransac_inliers_f32(_ptr(points), _ptr(moved), _ptr(counts), _ptr(found), n, S, max_per_subframe, int(min_features),
                                           float(threshold), float(confidence), int(max_iters), seed, _ptr(inlier), _ptr(info), _ptr(work),
                                           _stream()))
    return inlier, info


def gather_inliers(points, moved, inlier, info, W, H, sub_rows, sub_cols, min_features):
    """The survivors of `ransac_inliers` packed per pair as `host.pack_features` packs `tracker.finish_pair`'s (mfs.py:521, 578): sub-frame
    order outer, point order inner, float64 frame coordinates.  Returns (early (K_total, 2) float64, late, offsets (n + 1,) int32, pair_status
    (n,) int32 -- _lib.TRACK_PAIR_TOO_FEW where a pair has fewer than min_features survivors: its range is empty): what `vertex_motion` takes.
    Reads offsets[-1] to size the result, so it waits for the stream."""
    name = 'gather_inliers'
    n, S, max_per_subframe = _need_tracks(points, moved, name)
    dev = points.device
    _, _, cols, rows = track_subframe_grid(W, H, sub_rows, sub_cols)
    if cols * rows != S:
        raise ValueError(f'{name}: {W} x {H} cut {sub_rows} x {sub_cols} has {cols * rows} sub-frames, points has {S}')
    _need_like(inlier, torch.uint8, (n, S, max_per_subframe), dev, 'inlier', name)
    _need_like(info, torch.int32, (n, S, 4), dev, 'info', name)
    early = torch.empty((n * S * max_per_subframe, 2), dtype=torch.float64, device=dev)
    late = torch.empty_like(early)
    offsets = torch.empty(n + 1, dtype=torch.int32, device=dev)
    pair_status = torch.empty(n, dtype=torch.int32, device=dev)
    _lib.check(_lib_.mf_track_gather_f64(_ptr(points), _ptr(moved), _ptr(inlier), _ptr(info), n, int(W), int(H), int(sub_rows), int(sub_cols),
                                         max_per_subframe, int(min_features), _ptr(early), _ptr(late), _ptr(offsets), _ptr(pair_status),
                                         _stream()))
    total = int(offsets[-1].item())
    return early[:total], late[:total], offsets, pair_status


def fit_homographies(early, late, offsets):
    """The homography over each pair's packed survivors on the device (mfs.py:524-526), bit for bit tests/homography_model.py -- a
    specification of its own, not `host.lsq_homography`: the two minimise the same algebraic error in the same normalised coordinates and
    differ by rounding.  early / late (K_total, 2) float64 and offsets (P + 1,) int32 as `gather_inliers` leaves them.  Returns
    (homographies (P, 3, 3) float64 -- what `vertex_motion` takes --, info (P, 4) int32 -- (status, K, sweeps run, index of the chosen
    eigenvalue), status _lib.HFIT_OK / HFIT_TOO_FEW / HFIT_COLLINEAR / HFIT_AT_INFINITY / HFIT_NOT_CONVERGED --, diag (P, 8) float64 -- the
    two scales, the two centroids, the smallest and second smallest eigenvalue).  A pair that is not HFIT_OK gets the identity.  Runs on
    torch's current stream and does not wait for it: `fit_check` does."""
    name = 'fit_homographies'
    _need(early, torch.float64, 'early')
    _need(late, torch.float64, 'late')
    _need(offsets, torch.int32, 'offsets')
    if early.dim() != 2 or early.shape[1] != 2 or late.shape != early.shape or late.device != early.device:
        raise ValueError(f'{name}: early and late must be (K_total, 2) points on one device, got {tuple(early.shape)} and {tuple(late.shape)}')
    if offsets.dim() != 1 or offsets.numel() < 1 or offsets.device != early.device:
        raise ValueError(f'{name}: offsets must have shape (P + 1,) on the device of early, got {tuple(offsets.shape)}')
    P, K, dev = offsets.numel() - 1, early.shape[0], early.device
    homographies = torch.empty((P, 3, 3), dtype=torch.float64, device=dev)
    info = torch.empty((P, 4), dtype=torch.int32, device=dev)
    diag = torch.empty((P, 8), dtype=torch.float64, device=dev)
    size = _lib_.mf_homography_fit_workspace_bytes(P)
    work = torch.empty(size if size else 16, dtype=torch.uint8, device=dev)      # (0: outside the limits -- let the call itself say which)
    # (an empty tensor has no address; the call takes null features where K_total is 0, and every output of P == 0 is empty as well)
    held = [t if t.numel() else torch.empty(16, dtype=torch.uint8, device=dev) for t in (homographies, info, diag)]
    _lib.check(_lib_.mf_homography_fit_f64(_ptr(early) if K else None, _ptr(late) if K else None, _ptr(offsets), P, K, _ptr(held[0]), _ptr(held[1]),
                                           _ptr(held[2]), _ptr(work), _stream()))
    return homographies, info, diag


def fit_check(info):
    """The first pair of `fit_homographies`' info whose status is not _lib.HFIT_OK, or None.  Waits for the stream."""
    bad = torch.nonzero(info[:, 0] != _lib.HFIT_OK)
    return int(bad[0].item()) if bad.numel() else None


def feature_scores(homographies, info=None):
    """The cropping ratio and the distortion score of a clip from its per-frame (unstabilized -> cropped) homographies on the device
    (mfs.py:1196-1212 after the tracker), bit for bit tests/scores_model.py -- the eigenvalues of the affine part in closed form, not
    np.linalg.eigvals; the two agree within one float32 ulp.  homographies (P, 3, 3) float64 and info (P, 4) int32 as `fit_homographies`
    returns them: with info only the pairs whose status is _lib.HFIT_OK are scored, without it all are.  Returns (scores (2,) float32 --
    (cropping_ratio, distortion_score), two NaNs where no pair was scored --, per_pair (P, 2) float32 -- each pair's (ratio, distortion),
    NaNs where it was not scored --, record (2,) int32 -- (pairs scored, the first pair that was not scored or -1)).  One launch on torch's
    current stream; does not wait for it: `feature_scores_check` does."""
    name = 'feature_scores'
    _need(homographies, torch.float64, 'homographies')
    if homographies.dim() != 3 or tuple(homographies.shape[1:]) != (3, 3):
        raise ValueError(f'{name}: homographies must have shape (P, 3, 3), got {tuple(homographies.shape)}')
    P, dev = homographies.shape[0], homographies.device
    if info is not None:
        _need(info, torch.int32, 'info')
        if tuple(info.shape) != (P, 4) or info.device != dev:
            raise ValueError(f'{name}: info must have shape ({P}, 4) on the device of homographies, got {tuple(info.shape)}')
    if P < 1:
        raise ValueError(f'{name}: no pair to score (homographies has shape {tuple(homographies.shape)})')
    scores = torch.empty(2, dtype=torch.float32, device=dev)
    per_pair = torch.empty((P, 2), dtype=torch.float32, device=dev)
    record = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.check(_lib_.mf_feature_scores_f64(_ptr(homographies), _ptr(info) if info is not None else None, P, _ptr(per_pair), _ptr(scores),
                                           _ptr(record), _stream()))
    return scores, per_pair, record


def feature_scores_check(record):
    """The first pair `feature_scores` did not score (its record's second word), or None.  Waits for the stream."""
    first = int(record[1].item())
    return None if first < 0 else first


def vertex_motion(early, late, offsets, homographies, max_per_pair, W, H, R, C, ellipse_rows, ellipse_cols):
    """Vertex velocities and their running sum from matched features (mfs.py:236-452 after the tracker).
    early/late: (K_total, 2) float64 device tensors; offsets: (P+1,) int32; homographies: (P, 3, 3) float64.
    Returns (displacements (P+1, R+1, C+1, 2) float64, velocities (P, R+1, C+1, 2) float32, status (1,) int32);
    status != 0 means the reference's math.sqrt would have raised (mfs.py:444) -- see `vertex_motion_check`."""
    _need(early, torch.float64, 'early')
    _need(late, torch.float64, 'late')
    _need(offsets, torch.int32, 'offsets')
    _need(homographies, torch.float64, 'homographies')
    P = offsets.numel() - 1
    K = early.shape[0]
    if early.shape != late.shape or early.dim() != 2 or early.shape[1] != 2 or P < 0 or homographies.numel() != 9 * P:
        raise ValueError('features must be (K, 2) pairs with (P+1,) offsets and (P, 3, 3) homographies')
    dev = early.device
    vel = torch.empty((P, R + 1, C + 1, 2), dtype=torch.float32, device=dev)
    disp = torch.empty((P + 1, R + 1, C + 1, 2), dtype=torch.float64, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    work = torch.empty(_lib_.mf_vertex_motion_workspace_bytes(K, int(max_per_pair), P, R, C), dtype=torch.uint8, device=dev)
    _lib.check(_lib_.mf_vertex_motion_f64(_ptr(early), _ptr(late), _ptr(offsets), _ptr(homographies), P, K,
                                          int(max_per_pair), W, H, R, C, int(ellipse_rows), int(ellipse_cols),
                                          _ptr(vel), _ptr(disp), _ptr(work), _ptr(status), _stream()))
    return disp, vel, status


def vertex_motion_check(status):
    if int(status.item()):
        raise ValueError('math domain error')          # what math.sqrt raises at mfs.py:444


class OnlineState:
    """What `online_smooth` carries from block to block (include/meshflow_hip.h, mf_online_smooth_f64): the last L - 1 frames of the
    unstabilized path `c`, of the previous window's solution `q` -- both (L - 1, S) float64 -- and of the weights `lam` (L - 1,), on
    `device`, plus `seen`, the frames pushed so far.  `reset()` empties it."""

    def __init__(self, S, L, device):
        S, L = int(S), int(L)
        if S < 1 or not 2 <= L <= _lib.ONLINE_MAX_WINDOW:
            raise ValueError(f'OnlineState: S must be at least 1 and L in 2 .. {_lib.ONLINE_MAX_WINDOW} (got S={S}, L={L})')
        self.S, self.L = S, L
        self.c = torch.zeros((L - 1, S), dtype=torch.float64, device=device)
        self.device = self.c.device                       # (with its index: 'cuda' is the current device)
        self.q = torch.zeros((L - 1, S), dtype=torch.float64, device=self.device)
        self.lam = torch.zeros(L - 1, dtype=torch.float64, device=self.device)
        self.seen = 0

    def reset(self):
        for t in (self.c, self.q, self.lam):
            t.zero_()
        self.seen = 0


def online_smooth(vel, lam_known, state, taps, omega, iters, beta, lam_newest):
    """One block of n new frames through the online smoother (mf_online_smooth_f64, bit for bit tests/online_model.py): every frame is
    smoothed over the window of `state.L` frames that ends at it.  vel: (n, S) or (n, R+1, C+1, 2) float32 device tensor, row i the vertex
    velocity of the pair that ends at new frame i (`vertex_motion`'s velocities); lam_known: (n,) float64, entry i the adaptive weight of
    the frame before new frame i; row 0 / entry 0 are not read while the state is empty.  taps: (omega,) float64, `host.online_taps`.
    Returns (c, p): the unstabilized and the stabilized path of the n frames, (n, S) float64; `state` is updated in place.  Runs on
    torch's current stream and does not wait for it."""
    n = _online_smooth_args('online_smooth', vel, lam_known, state, taps, omega)
    c = torch.empty((n, state.S), dtype=torch.float64, device=state.device)
    p = torch.empty((n, state.S), dtype=torch.float64, device=state.device)
    _lib.check(_lib_.mf_online_smooth_f64(_ptr(vel), _ptr(lam_known), _ptr(taps), n, state.S, int(omega), state.L, int(iters), float(beta),
                                          float(lam_newest), state.seen, _ptr(state.c), _ptr(state.q), _ptr(state.lam), _ptr(c), _ptr(p),
                                          _stream()))
    state.seen += n
    return c, p


def _online_smooth_args(name, vel, lam_known, state, taps, omega):
    """What `online_smooth` and `online_smooth_lag` ask of their tensors; returns n."""
    if not isinstance(state, OnlineState):
        raise ValueError(f'{name}: state must be an OnlineState')
    _need(vel, torch.float32, 'vel')
    _need(lam_known, torch.float64, 'lam_known')
    _need(taps, torch.float64, 'taps')
    n = vel.shape[0] if vel.dim() else 0
    if n < 1 or vel.numel() != n * state.S:
        raise ValueError(f'{name}: vel must hold (n, {state.S}) velocities with n >= 1, got {tuple(vel.shape)}')
    if tuple(lam_known.shape) != (n,):
        raise ValueError(f'{name}: lam_known must have shape ({n},), got {tuple(lam_known.shape)}')
    if tuple(taps.shape) != (int(omega),):
        raise ValueError(f'{name}: taps must have shape ({int(omega)},), got {tuple(taps.shape)}')
    for t, what in ((vel, 'vel'), (lam_known, 'lam_known'), (taps, 'taps')):
        if t.device != state.device:
            raise ValueError(f'{name}: {what} must be on the device of the state, {state.device}, got {t.device}')
    return n


class OnlineGroupState:
    """The `OnlineState` of B streams stacked, for `online_smooth_group` (mf_online_smooth_group_f64): `c`, `q` (B, L - 1, S) and `lam`
    (B, L - 1) float64 on `device`, and `seen`, a host list of B frame counts.  `reset(stream)` forgets one stream -- its count goes to 0,
    at which the kernel reads none of its slices, so no byte is cleared --, `reset()` all of them."""

    def __init__(self, B, S, L, device):
        B, S, L = int(B), int(S), int(L)
        if B < 1 or S < 1 or not 2 <= L <= _lib.ONLINE_MAX_WINDOW:
            raise ValueError(f'OnlineGroupState: B and S must be at least 1 and L in 2 .. {_lib.ONLINE_MAX_WINDOW} (got B={B}, S={S}, L={L})')
        self.B, self.S, self.L = B, S, L
        self.c = torch.zeros((B, L - 1, S), dtype=torch.float64, device=device)
        self.device = self.c.device
        self.q = torch.zeros((B, L - 1, S), dtype=torch.float64, device=self.device)
        self.lam = torch.zeros((B, L - 1), dtype=torch.float64, device=self.device)
        self.seen = [0] * B

    def reset(self, stream=None):
        for b in (range(self.B) if stream is None else check_streams([stream], self.B, 'OnlineGroupState.reset: stream')):
            self.seen[b] = 0


def check_streams(streams, B, name='streams'):
    """`streams` as a list of ints: ints (no bool), distinct, each in 0 .. B - 1, at least one; else ValueError."""
    try:
        ids = list(streams)
    except TypeError:
        raise ValueError(f'{name} must be a sequence of stream indices (got {streams!r})') from None
    if not ids or any(isinstance(v, bool) or not isinstance(v, (int, np.integer)) for v in ids):
        raise ValueError(f'{name} must be a non-empty sequence of ints (got {streams!r})')
    ids = [int(v) for v in ids]
    if any(not 0 <= v < B for v in ids):
        raise ValueError(f'{name} must lie in 0 .. {B - 1} (got {ids})')
    if len(set(ids)) != len(ids):
        raise ValueError(f'{name} must be distinct: a stream takes one row per call (got {ids})')
    return ids


def online_smooth_group(vel, lam_known, state, streams, taps, omega, iters, beta, lam_newest):
    """`online_smooth` for K rows of n new frames, row r of stream streams[r] of `state`, an `OnlineGroupState`, in one pair of launches
    (mf_online_smooth_group_f64): every row's bytes are `online_smooth`'s on an `OnlineState` of that stream's history.  vel: (K, n, S)
    float32; lam_known: (K, n) float64; streams: K ints (no bool), distinct, in 0 .. state.B - 1; taps, omega, iters, beta, lam_newest are
    shared.  Returns (c, p), (K, n, S) float64; the named streams' slices of `state` are updated in place and their `seen` advanced by n, the
    others keep their bytes.  The ids and counts go up in one small copy; runs on torch's current stream and does not wait for it."""
    ids, K, n, d_rows, c, p = _online_smooth_group_args('online_smooth_group', vel, lam_known, state, streams, taps, omega)
    _lib.check(_lib_.mf_online_smooth_group_f64(_ptr(vel), _ptr(lam_known), _ptr(taps), _ptr(d_rows[2 * K:]), _ptr(d_rows), K, state.B, n, state.S,
                                                int(omega), state.L, int(iters), float(beta), float(lam_newest), _ptr(state.c), _ptr(state.q),
                                                _ptr(state.lam), _ptr(c), _ptr(p), _stream()))
    for b in ids:
        state.seen[b] += n
    return c, p


def _online_smooth_group_args(name, vel, lam_known, state, streams, taps, omega):
    """What `online_smooth_group` and `online_smooth_group_lag` ask alike; returns (ids, K, n, the uploaded counts and ids, c, p): the outputs
    (K, n, S) float64, not written yet."""
    if not isinstance(state, OnlineGroupState):
        raise ValueError(f'{name}: state must be an OnlineGroupState')
    ids = check_streams(streams, state.B, f'{name}: streams')
    K = len(ids)
    _need(vel, torch.float32, 'vel')
    _need(lam_known, torch.float64, 'lam_known')
    _need(taps, torch.float64, 'taps')
    n = int(vel.shape[1]) if vel.dim() == 3 else 0
    if n < 1 or tuple(vel.shape) != (K, n, state.S):
        raise ValueError(f'{name}: vel must have shape ({K}, n, {state.S}) with n >= 1, got {tuple(vel.shape)}')
    if tuple(lam_known.shape) != (K, n):
        raise ValueError(f'{name}: lam_known must have shape ({K}, {n}), got {tuple(lam_known.shape)}')
    if tuple(taps.shape) != (int(omega),):
        raise ValueError(f'{name}: taps must have shape ({int(omega)},), got {tuple(taps.shape)}')
    for t, what in ((vel, 'vel'), (lam_known, 'lam_known'), (taps, 'taps')):
        if t.device != state.device:
            raise ValueError(f'{name}: {what} must be on the device of the state, {state.device}, got {t.device}')
    # one upload: K int64 counts, then K int32 ids behind them (8-byte aligned in front, 4-byte behind)
    rows = np.empty(K * 3, dtype=np.int32)
    rows[:2 * K].view(np.int64)[:] = [state.seen[b] for b in ids]
    rows[2 * K:] = ids
    d_rows = torch.from_numpy(rows).to(state.device, non_blocking=True)
    c = torch.empty((K, n, state.S), dtype=torch.float64, device=state.device)
    p = torch.empty((K, n, state.S), dtype=torch.float64, device=state.device)
    return ids, K, n, d_rows, c, p


def check_online_lag(lag, L, name='lag'):
    """`lag` as an int: an int (no bool) in 0 .. L - 1 -- the lagged frame must be in the window, and the state must still hold every frame
    not yet handed out --, else ValueError."""
    if isinstance(lag, bool) or not isinstance(lag, (int, np.integer)) or not 0 <= int(lag) <= int(L) - 1:
        raise ValueError(f'{name} must be an int in 0 .. window - 1 = {int(L) - 1} (got {lag!r})')
    return int(lag)


def online_smooth_lag(vel, lam_known, state, taps, omega, iters, beta, lam_newest, lag):
    """`online_smooth` with `lag` frames of look-ahead (mf_online_smooth_lag_f64, bit for bit tests/online_lag_model.py): the n new frames
    are smoothed as `online_smooth` smooths them and leave the same state, but what comes back is each frame as it stands in the window
    that ends `lag` frames after it -- P_t = x_t of window t + lag after its last sweep, C_t unchanged.  Arguments and checks are
    `online_smooth`'s; lag: an int (no bool) in 0 .. state.L - 1.  Returns (c, p) of the frames that became final with this block, session
    indices max(0, seen - lag) .. seen + n - lag - 1: (m, S) float64 with m = max(0, seen + n - lag) - max(0, seen - lag), which is 0 while the
    session has no more than `lag` frames (the rows of frames that do not exist are dropped).  `online_pending` has the rest when the stream
    ends.  lag = 0 gives `online_smooth`'s bytes.  Runs on torch's current stream and does not wait for it."""
    name = 'online_smooth_lag'
    if not isinstance(state, OnlineState):
        raise ValueError(f'{name}: state must be an OnlineState')
    lag = check_online_lag(lag, state.L, f'{name}: lag')
    n = _online_smooth_args(name, vel, lam_known, state, taps, omega)
    c = torch.empty((n, state.S), dtype=torch.float64, device=state.device)
    p = torch.empty((n, state.S), dtype=torch.float64, device=state.device)
    _lib.check(_lib_.mf_online_smooth_lag_f64(_ptr(vel), _ptr(lam_known), _ptr(taps), n, state.S, int(omega), state.L, lag, int(iters),
                                              float(beta), float(lam_newest), state.seen, _ptr(state.c), _ptr(state.q), _ptr(state.lam),
                                              _ptr(c), _ptr(p), _stream()))
    drop = min(n, max(0, lag - state.seen))                 # the leading rows whose frame seen + i - lag does not exist
    state.seen += n
    return c[drop:], p[drop:]


def online_pending(state, lag):
    """The frames `online_smooth_lag` has not handed out when the stream ends: (c, p), clones of the last min(lag, state.seen) rows of
    `state.c` / `state.q` -- the final window's solution for frames seen - min(lag, seen) .. seen - 1, oldest first.  No kernel of the
    library's; the state is left as it is."""
    if not isinstance(state, OnlineState):
        raise ValueError('online_pending: state must be an OnlineState')
    lag = check_online_lag(lag, state.L, 'online_pending: lag')
    rows = min(lag, state.seen)
    return state.c[state.L - 1 - rows:].clone(), state.q[state.L - 1 - rows:].clone()


def online_smooth_group_lag(vel, lam_known, state, streams, taps, omega, iters, beta, lam_newest, lag):
    """`online_smooth_lag` for K rows of n new frames, row r of stream streams[r] of `state`, an `OnlineGroupState`, in one pair of launches
    (mf_online_smooth_group_lag_f64; tests/online_lag_model.py per row).  Arguments and checks are `online_smooth_group`'s; lag: an int (no
    bool) in 0 .. state.L - 1, shared by the rows.  The state after a call is `online_smooth_group`'s: it does not depend on lag.  Returns
    (c, p, final): c, p (K, n, S) float64, and final, a host list of K counts, final[r] = max(0, seen_r + n - lag) - max(0, seen_r - lag) with
    seen_r the stream's count before the call: the TRAILING final[r] rows of row r are the frames that became final, session indices
    max(0, seen_r - lag) .. seen_r + n - lag - 1, and the rows in front of them hold the kernel's zeros (`online_smooth_lag` drops them; the
    rows of a group differ in how many there are).  `online_pending_group` has the rest when a stream ends.  lag = 0 gives
    `online_smooth_group`'s bytes.  Runs on torch's current stream and does not wait for it."""
    name = 'online_smooth_group_lag'
    if not isinstance(state, OnlineGroupState):
        raise ValueError(f'{name}: state must be an OnlineGroupState')
    lag = check_online_lag(lag, state.L, f'{name}: lag')
    ids, K, n, d_rows, c, p = _online_smooth_group_args(name, vel, lam_known, state, streams, taps, omega)
    _lib.check(_lib_.mf_online_smooth_group_lag_f64(_ptr(vel), _ptr(lam_known), _ptr(taps), _ptr(d_rows[2 * K:]), _ptr(d_rows), K, state.B, n,
                                                    state.S, int(omega), state.L, lag, int(iters), float(beta), float(lam_newest), _ptr(state.c),
                                                    _ptr(state.q), _ptr(state.lam), _ptr(c), _ptr(p), _stream()))
    final = [max(0, state.seen[b] + n - lag) - max(0, state.seen[b] - lag) for b in ids]
    for b in ids:
        state.seen[b] += n
    return c, p, final


def online_pending_group(state, streams, lag):
    """`online_pending` for each stream of `streams` on its slices of an `OnlineGroupState`: a list of (c, p), one per named stream, clones of
    the last min(lag, state.seen[b]) rows of state.c[b] / state.q[b], oldest first.  No kernel of the library's; the state is left as it is."""
    name = 'online_pending_group'
    if not isinstance(state, OnlineGroupState):
        raise ValueError(f'{name}: state must be an OnlineGroupState')
    lag = check_online_lag(lag, state.L, f'{name}: lag')
    pending = []
    for b in check_streams(streams, state.B, f'{name}: streams'):
        rows = min(lag, state.seen[b])
        pending.append((state.c[b, state.L - 1 - rows:].clone(), state.q[b, state.L - 1 - rows:].clone()))
    return pending


def ring_exchange(ring, new, rows, M):
    """One tick of a ring of owed frames (mf_ring_exchange_u8, bit for bit tests/ring_model.py): ring (B, lag, ...) and new (K, ...) device
    tensors of one dtype and trailing shape, contiguous; rows: a (K, 3) int32 host array of (id, slot, out_row) per row of `new`, uploaded in
    one small copy.  Row r with out_row >= 0: out[out_row] = ring[id, slot], then ring[id, slot] = new[r]; with out_row < 0 only the store.
    M: the number of rows that hand a frame out, their out_row 0 .. M - 1, each once; the ids distinct.  Returns out (M, ...); M = 0 gives
    0 frames.  `ring` is updated in place.  Samples of any width go through as bytes.  Runs on torch's current stream and does not wait."""
    name = 'ring_exchange'
    if not isinstance(ring, torch.Tensor) or not isinstance(new, torch.Tensor):
        raise ValueError(f'{name}: ring and new must be torch tensors')
    if ring.dim() < 3 or new.dim() != ring.dim() - 1 or new.dtype != ring.dtype or new.shape[1:] != ring.shape[2:]:
        raise ValueError(f'{name}: ring must be (B, lag, ...) and new (K, ...) of the same dtype and trailing shape (got {ring.dtype} '
                         f'{tuple(ring.shape)} and {new.dtype} {tuple(new.shape)})')
    for t, what in ((ring, 'ring'), (new, 'new')):
        if not t.is_cuda or t.device != ring.device:
            raise ValueError(f'{name}: {what} must be a CUDA/HIP torch tensor, both on one device')
        if not t.is_contiguous():
            raise ValueError(f'{name}: {what} must be contiguous')
    B, lag, K = int(ring.shape[0]), int(ring.shape[1]), int(new.shape[0])
    N = int(new[0].numel()) * new.element_size() if K else 0
    if B < 1 or lag < 1 or K < 1 or N < 1 or K > _lib.ONLINE_GROUP_MAX_ROWS:
        raise ValueError(f'{name}: B, lag, K and the bytes of a frame must be at least 1 and K <= {_lib.ONLINE_GROUP_MAX_ROWS} (got ring '
                         f'{tuple(ring.shape)}, new {tuple(new.shape)})')
    rows = np.ascontiguousarray(rows)
    if rows.dtype != np.int32 or rows.shape != (K, 3):
        raise ValueError(f'{name}: rows must be a ({K}, 3) int32 array of (id, slot, out_row) (got {rows.dtype} {rows.shape})')
    M = int(M)
    handed = sorted(int(v) for v in rows[:, 2] if v >= 0)
    if handed != list(range(M)):
        raise ValueError(f'{name}: the out_row of the rows that hand a frame out must be 0 .. M - 1 = {M - 1}, each once (got {handed})')
    if ((rows[:, 0] < 0) | (rows[:, 0] >= B) | (rows[:, 1] < 0) | (rows[:, 1] >= lag)).any() or len(set(rows[:, 0].tolist())) != K:
        raise ValueError(f'{name}: ids must be distinct and in 0 .. {B - 1}, slots in 0 .. {lag - 1} (got {rows[:, :2].tolist()})')
    d_rows = torch.from_numpy(rows).to(ring.device, non_blocking=True)
    # (room for K frames, as the library's overlap rule takes d_out -- it cannot see M --; the steady tick has M = K)
    out = torch.empty((K,) + tuple(new.shape[1:]), dtype=new.dtype, device=new.device)
    _lib.check(_lib_.mf_ring_exchange_u8(_ptr(ring), _ptr(new), _ptr(out), _ptr(d_rows), K, B, lag, N, _stream()))
    return out[:M]


CUT_THRESHOLD = 0.30            # a design choice, not a value tuned on footage (profiles/cuts.md)


def check_cut_threshold(threshold, name='threshold'):
    """`threshold` as a float: a finite number in [0, 1], else ValueError."""
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or not 0.0 <= float(threshold) <= 1.0:
        raise ValueError(f'{name} must be a finite number in [0, 1] (got {threshold!r})')           # (a NaN fails both comparisons)
    return float(threshold)


def cut_bound(threshold, W, H):
    """The largest distance of two W x H frames that is not a cut: floor(threshold * 2 H W)."""
    return math.floor(float(threshold) * (2 * int(H) * int(W)))


def frame_signatures(d_luma):
    """The scene-cut signature of every frame of a (n, H, W) uint8 luma stack on the device: a (n, 256) int32 device tensor, bit for bit
    tests/cuts_model.py -- 4 x 4 tiles, 16 counters of value >> 4 per tile, [tile_row][tile_col][bin] (include/meshflow_hip.h,
    mf_frame_signature_u8).  On torch's current stream; does not wait for it."""
    name = 'frame_signatures'
    _need(d_luma, torch.uint8, 'd_luma')
    if d_luma.dim() != 3:
        raise ValueError(f'{name}: d_luma must have shape (n, H, W): one-channel uint8 images (got {tuple(d_luma.shape)})')
    n, H, W = (int(v) for v in d_luma.shape)
    if n < 1 or not 1 <= H <= _lib.CUT_MAX_DIM or not 1 <= W <= _lib.CUT_MAX_DIM:
        raise ValueError(f'{name}: d_luma needs n >= 1 and H, W in 1 .. {_lib.CUT_MAX_DIM} (got {tuple(d_luma.shape)})')
    sig = torch.empty((n, _lib.CUT_COUNTERS), dtype=torch.int32, device=d_luma.device)
    _lib.check(_lib_.mf_frame_signature_u8(_ptr(d_luma), n, W, H, _ptr(sig), _stream()))
    return sig


def cut_distances(d_sig, d_prev=None):
    """The distance of every signature of d_sig, (n, 256) int32 on the device, from the one before it: a (n,) int32 device tensor, entry i the
    sum over the 256 counters of |d_sig[i] - d_sig[i - 1]|; entry 0 is measured from d_prev, a (256,) int32 signature, and is 0 without one
    (mf_cut_distance_i32).  On torch's current stream; does not wait for it."""
    name = 'cut_distances'
    _need(d_sig, torch.int32, 'd_sig')
    if d_sig.dim() != 2 or d_sig.shape[0] < 1 or d_sig.shape[1] != _lib.CUT_COUNTERS:
        raise ValueError(f'{name}: d_sig must have shape (n, {_lib.CUT_COUNTERS}) with n >= 1 (got {tuple(d_sig.shape)})')
    if d_prev is not None:
        _need(d_prev, torch.int32, 'd_prev')
        if tuple(d_prev.shape) != (_lib.CUT_COUNTERS,) or d_prev.device != d_sig.device:
            raise ValueError(f'{name}: d_prev must have shape ({_lib.CUT_COUNTERS},) on the device of d_sig (got {tuple(d_prev.shape)} on {d_prev.device})')
    n = int(d_sig.shape[0])
    dist = torch.empty(n, dtype=torch.int32, device=d_sig.device)
    _lib.check(_lib_.mf_cut_distance_i32(_ptr(d_prev) if d_prev is not None else None, _ptr(d_sig), n, _ptr(dist), _stream()))
    return dist


def cut_distance_pairs(d_prev, d_sig):
    """`cut_distances` for rows that are frames of n different streams: entry r is the distance of d_sig[r] from d_prev[r], both (n, 256)
    int32 on the device (mf_cut_distance_pairs_i32).  A (n,) int32 device tensor.  On torch's current stream; does not wait for it."""
    name = 'cut_distance_pairs'
    _need(d_sig, torch.int32, 'd_sig')
    if d_sig.dim() != 2 or d_sig.shape[0] < 1 or d_sig.shape[1] != _lib.CUT_COUNTERS:
        raise ValueError(f'{name}: d_sig must have shape (n, {_lib.CUT_COUNTERS}) with n >= 1 (got {tuple(d_sig.shape)})')
    _need(d_prev, torch.int32, 'd_prev')
    if d_prev.shape != d_sig.shape or d_prev.device != d_sig.device:
        raise ValueError(f'{name}: d_prev must have shape {tuple(d_sig.shape)} on the device of d_sig (got {tuple(d_prev.shape)} on {d_prev.device})')
    n = int(d_sig.shape[0])
    dist = torch.empty(n, dtype=torch.int32, device=d_sig.device)
    _lib.check(_lib_.mf_cut_distance_pairs_i32(_ptr(d_prev), _ptr(d_sig), n, _ptr(dist), _stream()))
    return dist


def find_cuts(d_luma, threshold=CUT_THRESHOLD, d_prev=None):
    """Where the shots of a (n, H, W) uint8 luma stack on the device begin: (the indices i, relative to the stack, of the frames with
    distance[i] > floor(threshold * 2 H W); the distances as a NumPy (n,) int32 array; the last frame's signature, a (256,) int32 device
    tensor -- the next block's d_prev).  Frame 0 is measured from d_prev, the signature of the frame before the stack, and is never a cut
    without one.  threshold: a finite number in [0, 1]; at 1.0 nothing is a cut.  The decision is made on the host from the integers,
    which are handed out so that a caller can apply a rule of their own.  Two launches; the one wait is for the n distances."""
    threshold = check_cut_threshold(threshold)
    sig = frame_signatures(d_luma)
    dist = cut_distances(sig, d_prev).cpu().numpy()
    bound = cut_bound(threshold, d_luma.shape[2], d_luma.shape[1])
    return [int(i) for i in np.nonzero(dist.astype(np.int64) > bound)[0]], dist, sig[-1]


PATH_LIMIT_STEPS, PATH_LIMIT_GUARD, PATH_LIMIT_RISE = 32, 2.0, 2          # the guard from CPU trials, the rest by design (profiles/path_limit.md)


def check_path_limit(steps, guard, rise, names=('steps', 'guard', 'rise')):
    """(steps, guard, rise) as (int, float, int): steps in 1 .. 64, guard finite and >= 0, rise in 1 .. steps; else ValueError."""
    def whole(v):
        return isinstance(v, (int, np.integer)) and not isinstance(v, bool)
    if not whole(steps) or not 1 <= int(steps) <= _lib.PATH_LIMIT_MAX_STEPS:
        raise ValueError(f'{names[0]} must be an integer in 1 .. {_lib.PATH_LIMIT_MAX_STEPS} (got {steps!r})')
    if isinstance(guard, bool) or not isinstance(guard, (int, float, np.integer, np.floating)) or not 0.0 <= float(guard) < math.inf:
        raise ValueError(f'{names[1]} must be a finite number >= 0 (got {guard!r})')                 # (a NaN fails both comparisons)
    if not whole(rise) or not 1 <= int(rise) <= int(steps):
        raise ValueError(f'{names[2]} must be an integer in 1 .. {names[0]} = {int(steps)} (got {rise!r})')
    return int(steps), float(guard), int(rise)


def _path_limit_args(name, unstab, stab, W, H, R, C, rectangle, steps, guard, rise, out):
    """What `path_limit` and `path_limit_group` ask alike; returns (n, the rectangle as ints, steps, guard, rise, out -- made where None)."""
    W, H, R, C = int(W), int(H), int(R), int(C)
    if R < 1 or C < 1 or 2 * (R + C) > _lib.PATH_LIMIT_MAX_BOUNDARY:
        raise ValueError(f'{name}: the mesh needs R, C >= 1 and 2 (R + C) <= {_lib.PATH_LIMIT_MAX_BOUNDARY} (got R={R}, C={C})')
    if W < 2 or H < 2:
        raise ValueError(f'{name}: W and H must be at least 2 (got {W} x {H})')
    try:
        left, top, right, bottom = (int(v) for v in rectangle)
    except (TypeError, ValueError):
        raise ValueError(f'{name}: rectangle must be (left, top, right, bottom) (got {rectangle!r})') from None
    if not (0 <= left <= right <= W - 1 and 0 <= top <= bottom <= H - 1):
        raise ValueError(f'{name}: rectangle {(left, top, right, bottom)} is not inside a {W} x {H} frame')
    steps, guard, rise = check_path_limit(steps, guard, rise)
    _need(unstab, torch.float64, 'unstab')
    _need(stab, torch.float64, 'stab')
    S = (R + 1) * (C + 1) * 2
    n = unstab.shape[0] if unstab.dim() else 0
    if n < 1 or unstab.numel() != n * S or stab.numel() != n * S or stab.shape[0] != n:
        raise ValueError(f'{name}: unstab and stab must both hold (n, {S}) values with n >= 1, got {tuple(unstab.shape)} and {tuple(stab.shape)}')
    if stab.device != unstab.device:
        raise ValueError(f'{name}: stab must be on the device of unstab, {unstab.device}, got {stab.device}')
    if out is None:
        out = torch.empty((n, S), dtype=torch.float64, device=unstab.device)
    else:
        _need(out, torch.float64, 'out')
        if tuple(out.shape) != (n, S) or out.device != unstab.device:
            raise ValueError(f'{name}: out must have shape ({n}, {S}) on the device of unstab (got {tuple(out.shape)} on {out.device})')
    return n, (left, top, right, bottom), steps, guard, rise, out


def path_limit(unstab, stab, W, H, R, C, rectangle, steps=PATH_LIMIT_STEPS, guard=PATH_LIMIT_GUARD, rise=PATH_LIMIT_RISE, k_prev=None, out=None):
    """The stabilized path of n frames limited so that the warped mesh keeps covering `rectangle` (mf_path_limit_f64, bit for bit
    tests/path_limit_model.py): per frame the correction stab - unstab is scaled by k / steps, k the largest step at which the mesh's
    perimeter still encloses the rectangle widened by `guard` pixels, falling at once and rising by at most `rise` per frame.
    unstab, stab: (n, S) or (n, R+1, C+1, 2) float64 device tensors (`cell_table`'s); rectangle: (left, top, right, bottom), inclusive,
    `crop_resize`'s convention; k_prev: a 1-element int32 device tensor, the last k of the call before (a chain of calls so linked equals one
    call), None: no frame came before.  out: an (n, S) float64 device tensor to write into.  Returns (limited (n, S) float64, k (n,) int32),
    device tensors.  On torch's current stream; does not wait for it."""
    name = 'path_limit'
    n, (left, top, right, bottom), steps, guard, rise, out = _path_limit_args(name, unstab, stab, W, H, R, C, rectangle, steps, guard, rise, out)
    if k_prev is not None:
        _need(k_prev, torch.int32, 'k_prev')
        if k_prev.numel() != 1 or k_prev.device != unstab.device:
            raise ValueError(f'{name}: k_prev must hold 1 int32 on the device of unstab (got {tuple(k_prev.shape)} on {k_prev.device})')
    words = torch.empty((2, n), dtype=torch.int32, device=unstab.device)            # k_raw, k
    _lib.check(_lib_.mf_path_limit_f64(_ptr(unstab), _ptr(stab), n, int(W), int(H), int(R), int(C), left, top, right, bottom, guard, steps, rise,
                                       _ptr(k_prev) if k_prev is not None else None, _ptr(words[0]), _ptr(words[1]), _ptr(out), _stream()))
    return out, words[1]


def path_limit_group(unstab, stab, W, H, R, C, rectangle, steps=PATH_LIMIT_STEPS, guard=PATH_LIMIT_GUARD, rise=PATH_LIMIT_RISE, k_prev=None, out=None):
    """`path_limit` for K rows that are ONE frame each of K different streams (mf_path_limit_group_f64): nothing is chained between the rows;
    row r gets the bytes of a one-frame `path_limit` call with k_prev[r] carried.  Arguments and checks are `path_limit`'s, but k_prev: a
    (K,) int32 device tensor, a NEGATIVE entry saying that the row carries nothing (`path_limit`'s k_prev=None), and required.  Returns
    (limited (K, S) float64, k (K,) int32).  On torch's current stream; does not wait for it."""
    name = 'path_limit_group'
    n, (left, top, right, bottom), steps, guard, rise, out = _path_limit_args(name, unstab, stab, W, H, R, C, rectangle, steps, guard, rise, out)
    _need(k_prev, torch.int32, 'k_prev')
    if tuple(k_prev.shape) != (n,) or k_prev.device != unstab.device:
        raise ValueError(f'{name}: k_prev must have shape ({n},) on the device of unstab (got {tuple(k_prev.shape)} on {k_prev.device})')
    words = torch.empty((2, n), dtype=torch.int32, device=unstab.device)            # k_raw, k
    _lib.check(_lib_.mf_path_limit_group_f64(_ptr(unstab), _ptr(stab), n, int(W), int(H), int(R), int(C), left, top, right, bottom, guard, steps,
                                             rise, _ptr(k_prev), _ptr(words[0]), _ptr(words[1]), _ptr(out), _stream()))
    return out, words[1]


def stability_score(stab):
    """Stability score (mfs.py:1216-1259) of device-resident paths: (F, R+1, C+1, 2) or (F, S) float64 tensor ->
    (score (1,) float64 tensor, per-series fractions (S,))."""
    _need(stab, torch.float64, 'stab')
    F = stab.shape[0]
    S = stab.numel() // F
    series = torch.empty(S, dtype=torch.float64, device=stab.device)
    score = torch.empty(1, dtype=torch.float64, device=stab.device)
    _lib.check(_lib_.mf_stability_score_f64(_ptr(stab), F, S, _ptr(series), _ptr(score), _stream()))
    return score, series
