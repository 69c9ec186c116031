"""-m gpu: the P210 crop-resize -- `ops.crop_resize_p210` with a host rectangle and with one that stays on the device, and
`ops.crop_resize_y210`.

Every equality is bit for bit.  Both planes are compared with tests/p210_model.py over the whole case table (tests/p210_crop_cases.py: the
NV16 table's frames, rectangles and sizes, exactly 2x among them -- luma takes the box there, chroma does not); the host path with the device
path.  The table is checked on the CPU to hold low-clamped, high-clamped and interior chroma samples in x and in y before a kernel result is
looked at.  (uint16 tensors are compared as NumPy arrays or as int16 views.)"""
import ctypes
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cv16_area  # noqa: E402
import p210_crop_cases as cases  # noqa: E402
import p210_model as model  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def put(a, dev):
    return torch.from_numpy(np.array(a, dtype=np.uint16, copy=True)).to(dev)    # (a writable copy: the cases' arrays are read-only)


def get(t):
    return t.cpu().numpy()


def same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16))


def differing(got, want):
    d = got != want
    return int(d.sum()), np.argwhere(d)[:5].tolist()


def rect_tensor(rect, dev):
    return torch.tensor(rect, dtype=torch.int32, device=dev)


@pytest.mark.parametrize('name', cases.NAMES)
def test_crop_resize_p210_equals_the_model(dev, name):
    from meshflow_amd import ops
    counts = cases.class_counts()                                       # from the model alone, before any kernel result
    for axis in ('x', 'y'):
        assert min(counts[axis]) > 0, counts
    c = cases.frame(name)
    print(name, len(c['cases']), 'cases; classes of the table (low, high, interior):', counts)
    y, uv = put(c['y'], dev), put(c['uv'], dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    exact = 0
    for rect, size in c['cases']:
        want_y, want_uv = cases.want(name, rect, size)
        arg = None if size == (c['W'], c['H']) and rect[0] % 2 == 0 else size          # (the default size, taken now and then)
        got_y, got_uv = ops.crop_resize_p210(y, uv, rect, size=arg)
        dev_y, dev_uv, st = ops.crop_resize_p210(y, uv, rect_tensor(rect, dev), size=arg, status=status)
        assert st is status
        assert tuple(got_y.shape) == want_y.shape and tuple(got_uv.shape) == want_uv.shape == (c['n'], size[1], size[0] // 2, 2), (rect, size)
        g = get(got_y)
        assert np.array_equal(g, want_y), (rect, size, differing(g, want_y))
        g = get(got_uv)
        assert np.array_equal(g, want_uv), (rect, size, differing(g, want_uv))
        assert same(dev_y, got_y) and same(dev_uv, got_uv), (rect, size)
        if cases.is_exact_2x(rect, size):                               # luma took the box (the model's luma is cv16_area's), chroma did not
            left, top, right, bottom = rect
            assert np.array_equal(get(got_y)[0], cv16_area.area_fast_u16(c['y'][0][top:bottom + 1, left:right + 1, None])[..., 0])
            exact += 1
    print(name, 'exactly 2x:', exact)
    assert int(status.item()) == 0
    assert np.array_equal(get(y), c['y']) and np.array_equal(get(uv), c['uv'])


def test_the_table_s_exact_2x_cases_tell_a_chroma_box_from_the_definition():
    """(CPU, beside the run above: the planted area-box mutant differs from the model on the very cases the kernel passed.)"""
    n = 0
    for name in ('64x48', '100x71'):
        c = cases.frame(name)
        for rect, size in c['cases']:
            if cases.is_exact_2x(rect, size):
                n += int(not np.array_equal(model.crop_resize_chroma(c['uv'][0], rect, size, area_box=True), cases.want(name, rect, size)[1][0]))
    assert n > 0


def offset(a, off, dev, pad=48):
    """uint16 `a` in a sentinel-filled buffer, `off` bytes (even) past a 16-byte boundary: (buffer, lead, bytes, the view)."""
    raw = np.array(a, dtype=np.uint16, copy=True).reshape(-1).view(np.uint8)
    buf = torch.full((raw.size + pad,), 0xA5, dtype=torch.uint8, device=dev)
    lead = (-buf.data_ptr()) % 16 + off
    t = buf[lead:lead + raw.size]
    t.copy_(torch.from_numpy(raw).to(dev))
    return buf, lead, raw.size, t.view(torch.uint16).view(a.shape)


def test_stacks_aligned_to_2_bytes_only_and_canaries_around_every_buffer(dev):
    """`out=`: the pair comes back; all four stacks 2, 6, 10 and 14 bytes past a 16-byte boundary give the same bits and leave the sentinel
    around all four buffers alone."""
    from meshflow_amd import ops
    name = '66x49'
    c = cases.frame(name)
    for rect, size in (((3, 3, 62, 46), (92, 73)), ((2, 1, 65, 48), (64, 48)), ((3, 2, 65, 48), (14, 9))):
        want_y, want_uv = cases.want(name, rect, size)
        bounds = rect_tensor(rect, dev)
        for y_off, uv_off in ((0, 0), (2, 6), (6, 2), (10, 14)):
            iy, iuv = offset(c['y'], y_off, dev), offset(c['uv'], uv_off, dev)
            for b in (rect, bounds):
                oy = offset(np.full_like(want_y, 0xA5A5), y_off, dev)
                ouv = offset(np.full_like(want_uv, 0xA5A5), uv_off, dev)
                res = ops.crop_resize_p210(iy[3], iuv[3], b, size=size, out=(oy[3], ouv[3]))
                assert res[0].data_ptr() == oy[3].data_ptr() and res[1].data_ptr() == ouv[3].data_ptr()
                assert np.array_equal(get(oy[3]), want_y) and np.array_equal(get(ouv[3]), want_uv), (rect, size, y_off, uv_off)
                for buf, lead, nbytes, _ in (oy, ouv, iy, iuv):
                    assert bool((buf[:lead] == 0xA5).all()) and bool((buf[lead + nbytes:] == 0xA5).all()), (rect, size, y_off, uv_off)
            assert np.array_equal(get(iy[3]), c['y']) and np.array_equal(get(iuv[3]), c['uv'])


def at_the_end(a, lead, dev):
    """uint16 `a` as the LAST bytes of a device tensor of its own, `lead` bytes (even) into it."""
    raw = np.array(a, dtype=np.uint16, copy=True).reshape(-1).view(np.uint8)
    buf = torch.empty((lead + raw.size,), dtype=torch.uint8, device=dev)
    t = buf[lead:]
    t.copy_(torch.from_numpy(raw).to(dev))
    assert t.data_ptr() + t.numel() == buf.data_ptr() + buf.numel()
    return t.view(torch.uint16).view(a.shape)


def test_the_last_sample_of_the_stack_at_the_end_of_its_allocation(dev):
    """The stacks end where their tensors' bytes end, at 2-byte aligned addresses, and the rectangles reach the last column and row of the
    last frame: where s == c1 only the 4-byte sample is read, so the call reads nothing behind the stack -- and gives the model's bits."""
    from meshflow_amd import ops
    for name in ('66x49', '2x35', '2x2'):
        c = cases.frame(name)
        W, H = c['W'], c['H']
        y, uv = at_the_end(c['y'], 34, dev), at_the_end(c['uv'], 38, dev)
        for rect in ((0, 0, W - 1, H - 1), (W - 1, H - 1, W - 1, H - 1), (1, 1, W - 1, H - 1)):
            for size in ((W, H), (2 * W + 2, 2 * H + 1), (2, 3)):
                want_y, want_uv = model.crop_resize_clip(c['y'], c['uv'], rect, size)
                got_y, got_uv = ops.crop_resize_p210(y, uv, rect, size=size)
                dev_y, dev_uv, st = ops.crop_resize_p210(y, uv, rect_tensor(rect, dev), size=size)
                assert int(st.item()) == 0
                for g, w in ((got_y, want_y), (dev_y, want_y), (got_uv, want_uv), (dev_uv, want_uv)):
                    assert np.array_equal(get(g), w), (name, rect, size)


def test_output_at_the_crop_s_own_size_and_at_the_frame_s(dev):
    """An even-left rectangle at its own size is a copy of both sub-planes; the full frame at the frame's size is a copy of the clip."""
    from meshflow_amd import ops
    c = cases.frame('100x71')
    W, H = c['W'], c['H']
    y, uv = put(c['y'], dev), put(c['uv'], dev)
    for rect in ((0, 0, W - 1, H - 1), (2, 3, W - 3, H - 4), (4, 1, W - 1, H - 1), (6, 5, 9, 6)):
        left, top, right, bottom = rect
        cw, ch = right - left + 1, bottom - top + 1
        got_y, got_uv = ops.crop_resize_p210(y, uv, rect, size=(cw, ch))
        assert np.array_equal(get(got_y), c['y'][:, top:bottom + 1, left:right + 1])
        assert np.array_equal(get(got_uv), c['uv'][:, top:bottom + 1, left // 2:right // 2 + 1])
        frame_y, frame_uv = ops.crop_resize_p210(y, uv, rect)
        want_y, want_uv = model.crop_resize_clip(c['y'], c['uv'], rect, (W, H))
        assert np.array_equal(get(frame_y), want_y) and np.array_equal(get(frame_uv), want_uv)


def test_unusable_device_rectangles(dev):
    """Empty, negative, outside the frame: the status rises by exactly 1 per call and accumulates, the sentinel-filled outputs, the planes AND
    the workspace -- the luma y table included -- stay untouched (the C call, on a workspace of the test's own), and a usable call afterwards
    is correct."""
    from meshflow_amd import _lib, ops
    name = '66x49'
    c = cases.frame(name)
    W, H, n = c['W'], c['H'], c['n']
    y, uv = put(c['y'], dev), put(c['uv'], dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    bad = [(5, 3, 4, 40), (2, 9, 60, 8), (-1, 3, 60, 40), (2, -2, 60, 40), (2, 3, W, 40), (2, 3, 60, H), (W, H, W + 4, H + 4),
           (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 0, -2 ** 31, 5)]
    vp = ctypes.c_void_p
    stream = torch.cuda.current_stream().cuda_stream
    for size in ((W, H), (92, 73), (30, 9)):
        oy = put(np.full((n, size[1], size[0]), 0x5A5A, np.uint16), dev)
        ouv = put(np.full((n, size[1], size[0] // 2, 2), 0x5A5A, np.uint16), dev)
        nbytes = _lib.lib.mf_crop_resize_p210_workspace_bytes(*size)
        assert nbytes == 8 * (size[0] + size[1]) + 8 * (size[0] // 2)
        work = torch.full((nbytes,), 0x3C, dtype=torch.uint8, device=dev)
        before = int(status.item())
        for k, rect in enumerate(bad):
            bounds = rect_tensor(rect, dev)
            if k % 2:
                _, _, st = ops.crop_resize_p210(y, uv, bounds, size=size, out=(oy, ouv), status=status)
                assert st is status
            else:
                _lib.check(_lib.lib.mf_crop_resize_dev_p210(vp(y.data_ptr()), vp(uv.data_ptr()), vp(oy.data_ptr()), vp(ouv.data_ptr()), n, W, H,
                                                            vp(bounds.data_ptr()), size[0], size[1], vp(work.data_ptr()), vp(status.data_ptr()),
                                                            vp(stream)))
            assert int(status.item()) == before + k + 1, (rect, size)
        assert (get(oy) == 0x5A5A).all() and (get(ouv) == 0x5A5A).all() and bool((work == 0x3C).all()), size
        rect = (3, 3, 62, 46)
        ops.crop_resize_p210(y, uv, rect_tensor(rect, dev), size=size, out=(oy, ouv), status=status)
        assert int(status.item()) == before + len(bad)
        want_y, want_uv = model.crop_resize_clip(c['y'], c['uv'], rect, size)
        assert np.array_equal(get(oy), want_y) and np.array_equal(get(ouv), want_uv), size
    _, _, fresh = ops.crop_resize_p210(y, uv, rect_tensor(bad[0], dev))
    assert int(fresh.item()) == 1                                       # a status of the call's own starts at zero
    assert np.array_equal(get(y), c['y']) and np.array_equal(get(uv), c['uv'])


def test_crop_resize_y210_is_its_definition(dev):
    from meshflow_amd import ops
    c = cases.frame('100x71')
    y, uv = put(c['y'], dev), put(c['uv'], dev)
    packed = ops.pack_y210(y, uv)
    assert np.array_equal(get(packed), model.pack_y210(c['y'], c['uv']))
    rect = (3, 2, 96, 68)
    for size in (None, (128, 91), (48, 33)):
        ny, nuv = ops.crop_resize_p210(y, uv, rect, size=size)
        want = ops.pack_y210(ny, nuv)
        got = ops.crop_resize_y210(packed, rect, size=size)
        got_dev, st = ops.crop_resize_y210(packed, rect_tensor(rect, dev), size=size)
        assert int(st.item()) == 0 and same(got, want) and same(got_dev, want), size
        assert np.array_equal(get(got), model.pack_y210(*model.crop_resize_clip(c['y'], c['uv'], rect, size)))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _, st = ops.crop_resize_y210(packed, rect_tensor((5, 3, 4, 40), dev), status=status)
    assert st is status and int(status.item()) == 1
    assert np.array_equal(get(packed), model.pack_y210(c['y'], c['uv']))
