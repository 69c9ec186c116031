"""The largest frames the shape checks accept, one per pixel format: 32767 x 32767 (u8c1 1.07 GB, u8c3 3.2 GB, u8c4 4.29 GB, u16c3
6.4 GB) and a 16400 x 32767 u8c4 frame (2.15 GB) -- single frames whose byte offsets pass 2^31 (and 2^32 for u16c3) -- through warp and
crop-resize on the device.

The frames are a cheap integer formula of (x, y, channel) (`pattern`), filled on the device in row chunks, and the motions have closed
forms: an integer shift that uncovers the bottom and right edges (every pixel a copy of one source pixel, the border beyond the frame)
and a half-pixel shift in both axes (OpenCV's 1/32 fixed point gives (a + b + c + d + 2) >> 2 for 8-bit samples; border taps enter as the
border value).  The GPU output is compared with the closed form in row bands at the top, the bottom and across the rows where the frame's
byte offset crosses 2^31 and 2^32.  The test without a GPU pins every closed form against the C oracle, the NumPy oracle and
tests/cv16_model.py on small frames, so the large test relies only on formulas that have been checked."""
import numpy as np
import pytest

import cv16_area
import cv16_model

# format: (channels (0: an (n, H, W) frame), dtype, border of the warps)
FORMATS = {'u8c1': (0, np.uint8, (201,)), 'u8c3': (3, np.uint8, (11, 122, 233)), 'u8c4': (4, np.uint8, (11, 122, 233, 44)),
           'u16c3': (3, np.uint16, (1111, 40000, 65535))}
MOTIONS = {'shift': (3, 2), 'half': (0.5, 0.5)}                   # the source pixel of output (x, y) is (x + sx, y + sy)


def channels(fmt):
    return max(FORMATS[fmt][0], 1)


def pattern(fmt, ys, xs, cs):
    """Sample (x, y, c) of every frame of the largest-frame tests, for broadcastable int64 arrays or tensors (numpy or torch)."""
    if fmt == 'u16c3':
        return (37 * xs + 101 * ys + 4099 * cs + (xs ^ ys) + ((xs * ys) >> 7)) & 65535
    return (3 * xs + 5 * ys + 67 * cs + ((xs ^ ys) >> 3) + ((xs * ys) >> 9)) & 255


def rows_np(fmt, y0, y1, x0, x1, W, H, border=None):
    """Rows y0 .. y1 - 1, columns x0 .. x1 - 1 of the frame as int64 (rows, cols, channels); outside the frame: `border` (or nothing: the
    range must lie inside)."""
    ys = np.arange(y0, y1, dtype=np.int64)[:, None, None]
    xs = np.arange(x0, x1, dtype=np.int64)[None, :, None]
    cs = np.arange(channels(fmt), dtype=np.int64)[None, None, :]
    v = pattern(fmt, ys, xs, cs)
    inside = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
    if border is None:
        assert inside.all()
        return v
    return np.where(inside, v, np.asarray(border, dtype=np.int64)[:channels(fmt)])


def border_of(fmt):
    return FORMATS[fmt][2]


def expect_warp(fmt, motion, y0, y1, W, H):
    """Closed form of output rows y0 .. y1 - 1 (rows, W, channels) of a frame moved by MOTIONS[motion]."""
    border = border_of(fmt)
    sx, sy = MOTIONS[motion]
    if motion == 'shift':
        return rows_np(fmt, y0 + sy, y1 + sy, sx, W + sx, W, H, border)
    t = rows_np(fmt, y0, y1 + 1, 0, W + 1, W, H, border)
    s = t[:-1, :-1] + t[:-1, 1:] + t[1:, :-1] + t[1:, 1:]
    if fmt == 'u16c3':
        return np.rint(s / 4.0).astype(np.int64)                     # float weights 1/4, cvRound: halves to even
    return (s + 2) >> 2


def expect_crop(motion, W, H):
    """Closed form of the frame's crop values (left, top, right, bottom): the last column and row whose source lies within one pixel
    of the frame's last."""
    sx, sy = MOTIONS[motion]
    return (0, 0, W - 1 - int(np.ceil(sx)), H - 1 - int(np.ceil(sy)))


def motion_mesh(motion, R, C):
    """(unstabilised, stabilised) vertex displacements of one frame: a still camera stabilised to a translation by -MOTIONS[motion]."""
    unstab = np.zeros((1, R + 1, C + 1, 2))
    stab = unstab.copy()
    stab[..., 0], stab[..., 1] = (-v for v in MOTIONS[motion])
    return unstab, stab


def as_frames(fmt, v):
    """int64 samples (.., channels) -> frames of the format's dtype and shape."""
    a = v.astype(FORMATS[fmt][1])
    return a[..., 0] if fmt == 'u8c1' else a


def rgb(a):
    return np.ascontiguousarray(np.repeat(a[..., None], 3, axis=-1))


def oracle_warp(fmt, frames, R, C, unstab, stab):
    """The CPU reference of the edge suite (tests/test_gpu_pixel_edges.py): (frames, crop values)."""
    from oracle import clib
    border = border_of(fmt)
    if fmt == 'u16c3':
        return cv16_model.warp_clip_u16(frames, R, C, unstab, stab, border)
    if fmt == 'u8c1':
        b = border[0]
        out, crop, bad = clib.warp_clip(rgb(frames), R, C, unstab, stab, (b, b, b))
        assert bad == 0
        return out[..., 0], crop
    out, crop, bad = clib.warp_clip(np.ascontiguousarray(frames[..., :3]), R, C, unstab, stab, border[:3])
    assert bad == 0
    if fmt == 'u8c3':
        return out, crop
    a = border[3]
    out_a, crop_a, bad_a = clib.warp_clip(rgb(frames[..., 3]), R, C, unstab, stab, (a, a, a))
    assert bad_a == 0 and np.array_equal(crop_a, crop)
    return np.concatenate([out, out_a[..., :1]], axis=-1), crop


def oracle_resize(fmt, crop, ow, oh):
    """cv2.resize(crop, (ow, oh)) INTER_LINEAR as the oracles restate it, for one frame's crop of the format."""
    from oracle import meshflow_oracle as mo
    if fmt == 'u16c3':
        return cv16_area.resize_u16(crop, ow, oh)
    if fmt == 'u8c1':
        return mo.resize_linear_u8(rgb(crop), ow, oh)[..., 0]
    out = mo.resize_linear_u8(np.ascontiguousarray(crop[..., :3]), ow, oh)
    if fmt == 'u8c3':
        return out
    return np.concatenate([out, mo.resize_linear_u8(rgb(crop[..., 3]), ow, oh)[..., :1]], axis=-1)


MESHES = (('shift', (1, 1)), ('half', (2, 2)), ('shift', (2, 2)), ('half', (1, 1)))


@pytest.mark.parametrize('fmt', sorted(FORMATS))
@pytest.mark.parametrize('W,H', [(40, 56), (33, 70)])
def test_closed_forms_equal_the_oracles(fmt, W, H):
    """No GPU: every closed form the large test uses -- the warped frame and its crop values for both motions on a 1 x 1 and a 2 x 2 mesh,
    the same-size crop-resize (the identity) and a corner crop resized -- equals the CPU reference on small frames of the same pattern."""
    frames = as_frames(fmt, rows_np(fmt, 0, H, 0, W, W, H))[None]
    for motion, (R, C) in MESHES:
        unstab, stab = motion_mesh(motion, R, C)
        want, crop = oracle_warp(fmt, frames, R, C, unstab, stab)
        assert np.array_equal(as_frames(fmt, expect_warp(fmt, motion, 0, H, W, H)), want[0]), (motion, R, C)
        assert tuple(crop[0].tolist()) == expect_crop(motion, W, H), (motion, crop)
        assert np.array_equal(as_frames(fmt, expect_warp(fmt, motion, H - 7, H, W, H)), want[0, H - 7:])        # a band alone
    assert np.array_equal(oracle_resize(fmt, frames[0], W, H), frames[0])
    l, t = W - 17, H - 13
    corner = as_frames(fmt, rows_np(fmt, t, H, l, W, W, H))
    assert np.array_equal(corner, frames[0, t:, l:])
    assert oracle_resize(fmt, corner, 7, 5).shape[:2] == (5, 7)


# ---- on the GPU ----------------------------------------------------------------------------------------------------------------------

LARGEST = [('u8c1', 32767, 32767), ('u8c3', 32767, 32767), ('u8c4', 16400, 32767), ('u8c4', 32767, 32767), ('u16c3', 32767, 32767)]


def bands(W, H, bpp):
    """Row ranges to compare: the top, the bottom, and 5 rows around each row where the frame's byte offset crosses 2^31 and 2^32."""
    out = [(0, 3), (H - 3, H)]
    for edge in (1 << 31, 1 << 32):
        y = edge // (W * bpp)
        if y < H:
            out.append((max(0, y - 2), min(H, y + 3)))
    return out


def device_frame(fmt, W, H, dev, chunk=512):
    """The pattern as one (1, H, W[, channels]) frame on `dev`, computed there in chunks of rows."""
    import torch
    ch = channels(fmt)
    shape = (1, H, W) if fmt == 'u8c1' else (1, H, W, ch)
    frame = torch.empty(shape, dtype=torch.int16 if fmt == 'u16c3' else torch.uint8, device=dev)
    xs = torch.arange(W, dtype=torch.int64, device=dev)[None, :, None]
    cs = torch.arange(ch, dtype=torch.int64, device=dev)[None, None, :]
    for y0 in range(0, H, chunk):
        ys = torch.arange(y0, min(H, y0 + chunk), dtype=torch.int64, device=dev)[:, None, None]
        v = pattern(fmt, ys, xs, cs).to(frame.dtype)                   # (int64 -> int16 keeps the low 16 bits)
        frame[0, y0:y0 + v.shape[0]] = v[..., 0] if fmt == 'u8c1' else v
        del v
    return frame.view(torch.uint16) if fmt == 'u16c3' else frame


def host_rows(t):
    import torch
    if t.dtype == torch.uint16:
        return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize('fmt,W,H', LARGEST)
def test_largest_frame_warp_and_crop_resize(fmt, W, H):
    """One frame of the largest shape: both motions through ops.warp (rows compared in bands with the closed form, crop values and clip
    rectangle with theirs), the whole-frame same-size crop-resize (the identity, in the same bands) and the frame's far corner resized
    to 23 x 17 against the oracle on that crop."""
    import torch
    from meshflow_amd import ops
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    dev = torch.device('cuda:0')
    bpp = channels(fmt) * np.dtype(FORMATS[fmt][1]).itemsize
    need = 2 * W * H * bpp + (1 << 30)
    torch.cuda.empty_cache()
    free = torch.cuda.mem_get_info(dev)[0]
    if free < need:
        pytest.skip(f'not enough free device memory for a {W} x {H} {fmt} frame and its output: {need / 1e9:.1f} GB needed, '
                    f'{free / 1e9:.1f} GB free')
    frame = device_frame(fmt, W, H, dev)
    out = torch.empty_like(frame)
    try:
        for motion, (R, C) in (('shift', (1, 1)), ('half', (2, 2))):
            unstab, stab = motion_mesh(motion, R, C)
            table = ops.cell_table(torch.from_numpy(unstab).to(dev), torch.from_numpy(stab).to(dev), W, H, R, C)
            ops.warp(frame, table, FORMATS[fmt][2], out=out)
            torch.cuda.synchronize()
            table.check()
            want_crop = expect_crop(motion, W, H)
            assert tuple(table.crop.cpu().numpy()[0].tolist()) == want_crop, (motion, table.crop)
            assert tuple(table.clip_bounds.cpu().numpy().tolist()) == want_crop, (motion, table.clip_bounds)
            for y0, y1 in bands(W, H, bpp):
                got = host_rows(out[0, y0:y1])
                want = as_frames(fmt, expect_warp(fmt, motion, y0, y1, W, H))
                assert np.array_equal(got, want), (motion, (y0, y1), int((got != want).sum()))
            del table
        ops.crop_resize(frame, (0, 0, W - 1, H - 1), out=out)
        torch.cuda.synchronize()
        for y0, y1 in bands(W, H, bpp):
            assert np.array_equal(host_rows(out[0, y0:y1]), as_frames(fmt, rows_np(fmt, y0, y1, 0, W, W, H))), ('identity', (y0, y1))
        l, t = W - 61, H - 45
        small = host_rows(ops.crop_resize(frame, (l, t, W - 1, H - 1), size=(23, 17)))
        want = oracle_resize(fmt, as_frames(fmt, rows_np(fmt, t, H, l, W, W, H)), 23, 17)
        assert np.array_equal(small[0], want)
    finally:
        del frame, out
        torch.cuda.empty_cache()
