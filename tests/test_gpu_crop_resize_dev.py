"""-m gpu: crop-resize from a rectangle that stays on the device -- mf_crop_resize_dev_u8c3 / _u16c3 / _u8c1 / _u8c4 and
ops.crop_resize_resident.  The kernels read {left, top, right, bottom} from device memory when they execute; for a usable rectangle
the output and the tables are byte for byte those of the host-rectangle call (ops.crop_resize / mf_crop_resize_to_*, themselves pinned to
the oracle by test_gpu_crop_resize_to.py and its neighbours; a few cases and a random sweep here go to the oracle's resize and the uint16
models directly).  The call never waits for the device; an unusable rectangle writes nothing, counts 1 in the caller's status word and
faults nothing; what the host can check without the rectangle it refuses without launching."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from meshflow_amd import _lib, ops  # noqa: E402
from test_gpu_crop_resize_to import SWEEP_CLASSES, frames_of, reference, sweep_draw, to_dev, to_np  # noqa: E402

FORMATS = ('u8c3', 'u8c1', 'u16c3', 'u8c4')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def dev_rect(rect, dev):
    """The rectangle as a 4-element int32 device tensor, written by a device op (an add kernel), never read back."""
    return torch.tensor(rect, dtype=torch.int32).to(dev) + torch.zeros(4, dtype=torch.int32, device=dev)


def rects_of(W, H):
    """whole frame, one pixel, one row, one column, odd offsets, touching the last row and column, a typical 85 % crop (even sizes, so
    that the exact-2x output exists)"""
    w85, h85 = int(W * 0.85) // 2 * 2, int(H * 0.85) // 2 * 2
    l85, t85 = (W - w85) // 2, (H - h85) // 2
    return [(0, 0, W - 1, H - 1), (W // 3, H // 3, W // 3, H // 3), (0, H // 2, W - 1, H // 2), (W // 2, 0, W // 2, H - 1),
            (3, 5, W - 8, H - 6), (W // 4 + 1, H // 4 + 1, W - 1, H - 1), (l85, t85, l85 + w85 - 1, t85 + h85 - 1)]


def sizes_of(fmt, W, H, rect):
    """None (the same size), larger than the frame in both axes, larger in one and smaller in the other, 1.5x down, exactly 2x down of the
    crop (where its sides are even), more than 2.6x down (u8c1: more than 4x) -- and an upscale of the crop that stays below the frame,
    where the host would pick `up` and the device-rectangle call takes `down`"""
    cw, ch = rect[2] - rect[0] + 1, rect[3] - rect[1] + 1
    k = 5 if fmt == 'u8c1' else 3
    sizes = [None, (W + 13, H + 7), (W + 9, max(1, ch // 2)), (max(1, int(cw / 1.5)), max(1, int(ch / 1.5))),
             (max(1, cw // 2), max(1, ch // 2)), (max(1, cw // k), max(1, ch // k))]
    if cw < W - 1 or ch < H - 1:
        sizes.append((min(W - 1, cw + 1) if cw < W - 1 else cw, ch + 1 if ch < H - 1 else ch))
    return sizes


def raw_calls(fmt):
    return getattr(_lib.lib, f'mf_crop_resize_to_{fmt}'), getattr(_lib.lib, f'mf_crop_resize_dev_{fmt}')


def vp(t):
    return ctypes.c_void_p(t.data_ptr())


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize('fmt', FORMATS)
def test_small_frames_equal_the_host_rectangle_call_tables_included(dev, fmt):
    """W % 4 != 0, through the raw C calls with workspaces of the test's own: output AND tables byte for byte."""
    n, H, W = 3, 46, 67
    frames = to_dev(frames_of(fmt, n, H, W, seed=3), dev)
    host_call, dev_call = raw_calls(fmt)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    for rect in rects_of(W, H):
        d_rect = dev_rect(rect, dev)
        for size in sizes_of(fmt, W, H, rect):
            ow, oh = size or (W, H)
            shape = (n, oh, ow) + tuple(frames.shape[3:])
            tab_bytes = (ow + oh) * 8
            assert _lib.lib.mf_crop_resize_workspace_bytes(ow, oh) == tab_bytes
            a, b = (torch.zeros(shape, dtype=frames.dtype, device=dev) for _ in range(2))
            wa, wb = (torch.full((tab_bytes + 64,), 0x5A, dtype=torch.uint8, device=dev) for _ in range(2))
            assert host_call(vp(frames), vp(a), n, W, H, *rect, ow, oh, vp(wa), stream()) == 0, _lib.lib.mf_last_error()
            assert dev_call(vp(frames), vp(b), n, W, H, vp(d_rect), ow, oh, vp(wb), vp(status), stream()) == 0, _lib.lib.mf_last_error()
            torch.cuda.synchronize()
            assert torch.equal(a, b), (fmt, rect, size)
            assert torch.equal(wa, wb) and bool((wb[tab_bytes:] == 0x5A).all()), (fmt, rect, size)
    assert int(status.item()) == 0


@pytest.mark.parametrize('fmt', FORMATS)
def test_1080p_equals_the_host_rectangle_call(dev, fmt):
    n, H, W = 2, 1080, 1920
    frames = to_dev(frames_of(fmt, n, H, W, seed=4), dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    for rect in rects_of(W, H):
        d_rect = dev_rect(rect, dev)
        for size in sizes_of(fmt, W, H, rect):
            got, st = ops.crop_resize_resident(frames, d_rect, size=size, status=status)
            assert st is status
            want = ops.crop_resize(frames, rect, size=size)
            assert got.shape == want.shape and torch.equal(got, want), (fmt, rect, size)
    assert int(status.item()) == 0


@pytest.mark.parametrize('fmt', ('u8c3', 'u16c3'))
def test_against_the_oracle_and_the_uint16_models(dev, fmt):
    """... so that this file does not rest on device code alone: oracle.meshflow_oracle.resize_linear_u8 (u8c3), tests/cv16_model.py +
    cv16_area.py (u16c3: the exact-2x case takes the area branch, chosen on the device from the loaded rectangle)."""
    n, H, W = 2, 90, 130
    frames = frames_of(fmt, n, H, W, seed=6)
    d_frames = to_dev(frames, dev)
    for rect, size in (((1, 3, 120, 82), (60, 40)),            # exactly 2x down
                       ((1, 3, 120, 82), None), ((0, 0, W - 1, H - 1), (200, 140)), ((7, 9, 7, 9), (31, 17)),
                       ((5, 0, 124, 89), (40, 30)), ((2, 2, 100, 50), (150, 20)), ((10, 10, 109, 79), (66, 47))):
        ow, oh = size or (W, H)
        got, status = ops.crop_resize_resident(d_frames, dev_rect(rect, dev), size=size)
        g, want = to_np(got), reference(fmt, frames, rect, ow, oh)
        assert np.array_equal(g, want), (fmt, rect, size, int((g != want).sum()))
        assert int(status.item()) == 0


@pytest.mark.parametrize('fmt', FORMATS)
def test_random_sweep(dev, fmt):
    """test_gpu_crop_resize_to.py's seeded draws (300 per format: 1 x 1, up, exactly 2x and 3x down, both sides of the staged / direct
    cut-over, mixed), each with a crop placed at random and one in the last rows of the frame, against the oracle's model and against
    the host-rectangle call."""
    rng = np.random.default_rng({'u8c3': 41, 'u8c1': 42, 'u16c3': 43, 'u8c4': 44}[fmt])
    kinds = set()
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    for d in range(300):
        n, H, W, cw, ch, (ow, oh), kind = sweep_draw(rng, fmt)
        frames = frames_of(fmt, n, H, W, seed=2000 * d + 9)
        d_frames = to_dev(frames, dev)
        for (l, t) in ((int(rng.integers(0, W - cw + 1)), int(rng.integers(0, H - ch + 1))), (int(rng.integers(0, W - cw + 1)), H - ch)):
            rect = (l, t, l + cw - 1, t + ch - 1)
            got, _ = ops.crop_resize_resident(d_frames, dev_rect(rect, dev), size=(ow, oh), status=status)
            assert torch.equal(got, ops.crop_resize(d_frames, rect, size=(ow, oh))), (fmt, d, kind, (n, H, W), rect, (ow, oh))
            g, want = to_np(got), reference(fmt, frames, rect, ow, oh)
            assert np.array_equal(g, want), (fmt, d, kind, (n, H, W), rect, (ow, oh), int((g != want).sum()))
        kinds.add(kind)
    assert kinds == set(SWEEP_CLASSES) and int(status.item()) == 0


@pytest.mark.parametrize('fmt', FORMATS)
def test_the_rectangle_is_read_when_the_kernels_execute(dev, fmt):
    """Two calls on one stream with the SAME bounds tensor, its contents replaced by a device-side copy_ in between."""
    n, H, W = 2, 60, 84
    frames = to_dev(frames_of(fmt, n, H, W, seed=8), dev)
    first, second = (4, 6, 70, 50), (20, 1, 83, 33)
    bounds, other = dev_rect(first, dev), dev_rect(second, dev)
    for size in (None, (50, 31)):
        bounds.copy_(dev_rect(first, dev))
        a, _ = ops.crop_resize_resident(frames, bounds, size=size)
        bounds.copy_(other)
        b, _ = ops.crop_resize_resident(frames, bounds, size=size)
        torch.cuda.synchronize()
        assert torch.equal(a, ops.crop_resize(frames, first, size=size)) and torch.equal(b, ops.crop_resize(frames, second, size=size))
        assert not torch.equal(a, b)


@pytest.mark.parametrize('fmt', FORMATS)
def test_no_host_wait(dev, fmt):
    """Under torch's sync debug mode 'error' the call succeeds; and behind a device-side delay that dwarfs a launch, an event recorded
    after the call is still pending when the call has returned."""
    n, H, W = 2, 120, 160
    frames = to_dev(frames_of(fmt, n, H, W, seed=10), dev)
    rect = (3, 4, 150, 110)
    bounds = dev_rect(rect, dev)
    out = torch.empty_like(frames)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    ops.crop_resize_resident(frames, bounds, out=out, status=status)          # (allocator and one-time device probe warmed up)
    # size the delay from a measured short one: cycles for ~0.3 s
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    probe = 2_000_000
    torch.cuda._sleep(probe)
    torch.cuda.synchronize()
    t0.record()
    torch.cuda._sleep(probe)
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1)
    assert ms > 0
    cycles = int(probe * 300.0 / ms)
    out.zero_()
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode('error')
        torch.cuda._sleep(cycles)
        got, _ = ops.crop_resize_resident(frames, bounds, out=out, status=status)
        got2, _ = ops.crop_resize_resident(frames, bounds, size=(77, 201), status=status)
        done = torch.cuda.Event()
        done.record()
        pending = not done.query()
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert pending, f'the call returned only after the {ms * cycles / probe:.0f} ms delay had run'
    torch.cuda.synchronize()
    assert torch.equal(got, ops.crop_resize(frames, rect)) and torch.equal(got2, ops.crop_resize(frames, rect, size=(77, 201)))
    assert int(status.item()) == 0


def unusable(W, H):
    """right < left, bottom < top, a negative edge (two of them), right >= W, bottom >= H -- and 16 bytes of anything"""
    i32 = np.iinfo(np.int32)
    return [(20, 3, 10, 20), (2, 20, 30, 10), (-1, 3, 30, 20), (2, -5, 30, 20), (2, 3, W, 20), (2, 3, 30, H),
            (i32.min, i32.min, i32.max, i32.max), (i32.max, i32.max, i32.min, i32.min), (0, 0, i32.max, 5), (-7, -7, -7, -7)]


@pytest.mark.parametrize('fmt', FORMATS)
def test_unusable_rectangles_write_nothing_and_count(dev, fmt):
    """Guarded refusals on the device: `out` and the workspace keep their pattern, the status word goes up by 1 per call, and the next
    good call is exact."""
    n, H, W = 2, 30, 40
    frames = to_dev(frames_of(fmt, n, H, W, seed=12), dev)
    _, dev_call = raw_calls(fmt)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    calls = 0
    for size in (None, (25, 15), (90, 70), (50, 10)):
        ow, oh = size or (W, H)
        shape = (n, oh, ow) + tuple(frames.shape[3:])
        out = torch.empty(shape, dtype=frames.dtype, device=dev)
        out.view(torch.uint8).fill_(0xA5)
        work = torch.full(((ow + oh) * 8,), 0x5A, dtype=torch.uint8, device=dev)
        for rect in unusable(W, H):
            assert dev_call(vp(frames), vp(out), n, W, H, vp(dev_rect(rect, dev)), ow, oh, vp(work), vp(status), stream()) == 0
            calls += 1
            torch.cuda.synchronize()
            assert int(status.item()) == calls, (fmt, size, rect)
        assert bool((out.view(torch.uint8) == 0xA5).all()) and bool((work == 0x5A).all()), (fmt, size)
        got, st = ops.crop_resize_resident(frames, dev_rect(rect := (2, 3, 30, 20), dev), out=out, size=size, status=status)
        assert torch.equal(got, ops.crop_resize(frames, rect, size=size)) and int(st.item()) == calls
    # ops: a fresh status word per call when none is given
    out, st = ops.crop_resize_resident(frames, dev_rect((5, 5, 4, 9), dev))
    assert int(st.item()) == 1


@pytest.mark.parametrize('fmt', FORMATS)
def test_host_side_refusals_launch_nothing(dev, fmt):
    n, H, W = 2, 30, 40
    frames = to_dev(frames_of(fmt, n, H, W, seed=11), dev)
    out = torch.full((4 * 1024 * 1024,), 0xA5, dtype=torch.uint8, device=dev)
    work = torch.full((_lib.lib.mf_crop_resize_workspace_bytes(32767, 32767),), 0x5A, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    bounds = dev_rect((2, 3, 30, 20), dev)
    _, call = raw_calls(fmt)
    F, O, B, Wk, S = (vp(t) for t in (frames, out, bounds, work, status))
    bad = [
        (None, O, n, W, H, B, 25, 15, Wk, S), (F, None, n, W, H, B, 25, 15, Wk, S), (F, O, n, W, H, None, 25, 15, Wk, S),      # null pointers
        (F, O, n, W, H, B, 25, 15, None, S), (F, O, n, W, H, B, 25, 15, Wk, None), (F, F, n, W, H, B, 25, 15, Wk, S),           # ... aliasing
        (F, O, n, W, H, B, 0, 15, Wk, S), (F, O, n, W, H, B, 25, 0, Wk, S), (F, O, n, W, H, B, 32768, 15, Wk, S),               # output sizes
        (F, O, n, W, H, B, 25, -1, Wk, S),
        (F, O, 0, W, H, B, 25, 15, Wk, S), (F, O, n, 0, H, B, 25, 15, Wk, S), (F, O, n, W, 32768, B, 25, 15, Wk, S),            # shapes
        (F, O, 1 << 20, W, H, B, 32767, 32767, Wk, S),                                                                          # too many tiles
    ]
    for args in bad:
        assert call(*args, stream()) == _lib.MF_ERR_INVALID_ARG, args
        assert f'mf_crop_resize_dev_{fmt}' in _lib.lib.mf_last_error().decode(), _lib.lib.mf_last_error()
    # the whole text of one refusal of each kind (the strings the library has always given)
    texts = [
        ((F, O, n, W, 32768, B, 25, 15, Wk, S), f'mf_crop_resize_dev_{fmt}: unsupported shape n=2 W=40 H=32768'),
        ((F, O, n, W, H, B, 25, -1, Wk, S), f'mf_crop_resize_dev_{fmt}: unsupported output size 25x-1 (1 .. 32,767 each)'),
        ((F, O, 1 << 20, W, H, B, 32767, 32767, Wk, S), f'mf_crop_resize_dev_{fmt}: too many tiles'),
    ]
    for args, text in texts:
        assert call(*args, stream()) == _lib.MF_ERR_INVALID_ARG, args
        assert _lib.lib.mf_last_error().decode() == text
    # ops: `out` of the wrong shape, a host tensor, a wrong dtype or a wrong length as bounds, a bad size, a bad status
    good_out = torch.empty_like(frames)
    for kw in (dict(bounds=bounds, out=good_out, size=(25, 15)), dict(bounds=bounds, out=torch.empty_like(frames)[:1]),
               dict(bounds=torch.tensor([2, 3, 30, 20], dtype=torch.int32)), dict(bounds=bounds.to(torch.int64)),
               dict(bounds=bounds.to(torch.float32)), dict(bounds=torch.zeros(5, dtype=torch.int32, device=dev)),
               dict(bounds=(2, 3, 30, 20)), dict(bounds=bounds, size=(0, 5)), dict(bounds=bounds, size=(5.0, 5)),
               dict(bounds=bounds, status=torch.zeros(1, dtype=torch.int64, device=dev)),
               dict(bounds=bounds, status=torch.zeros(2, dtype=torch.int32, device=dev))):
        with pytest.raises(ValueError):
            ops.crop_resize_resident(frames, **kw)
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((work == 0x5A).all()) and int(status.item()) == 0
