"""-m gpu: crop-resize to a caller-chosen output size on the device -- mf_crop_resize_to_u8c3 / _u16c3 / _u8c1 / _u8c4 and
ops.crop_resize(size=...) -- equal, sample for sample, to cv2.resize(crop, (out_W, out_H)) INTER_LINEAR as the oracle restates it
(oracle.meshflow_oracle.resize_linear_u8; grey = channel 0 of that on the frame repeated three times; 4-channel = that on B G R and
channel 0 of it on the alpha plane repeated three times; uint16: tests/cv16_model.py's float path plus tests/cv16_area.py's exact-2x
branch).  Upscale, downscale, mixed, 1-pixel crops and outputs, outputs larger than the frame,
W % 4 != 0, unaligned stacks, many tiles, both sides of the staged / direct cut-over; the same size equals today's call byte for byte;
every refusal leaves the output untouched."""
import ctypes

import numpy as np
import pytest

import cv16_area

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from meshflow_amd import _lib, ops  # noqa: E402
from oracle import meshflow_oracle as mo  # noqa: E402

FORMATS = ('u8c3', 'u8c1', 'u16c3', 'u8c4')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def frames_of(fmt, n, H, W, seed):
    rng = np.random.default_rng(seed)
    if fmt == 'u16c3':
        return rng.integers(0, 65536, (n, H, W, 3), dtype=np.uint16)
    return rng.integers(0, 256, {'u8c3': (n, H, W, 3), 'u8c1': (n, H, W), 'u8c4': (n, H, W, 4)}[fmt], dtype=np.uint8)


def to_dev(a, dev):
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.uint8)).to(dev)
    return t.view(torch.uint16) if a.dtype == np.uint16 else t


def to_np(t):
    return t.contiguous().view(torch.uint8).cpu().numpy().view(np.uint16) if t.dtype == torch.uint16 else t.cpu().numpy()


def reference(fmt, frames, rect, ow, oh):
    l, t, r, b = rect
    out = []
    for f in frames:
        crop = f[t:b + 1, l:r + 1]
        if fmt == 'u8c3':
            out.append(mo.resize_linear_u8(crop, ow, oh))
        elif fmt == 'u8c1':
            out.append(mo.resize_linear_u8(np.repeat(crop[..., None], 3, axis=2), ow, oh)[..., 0])
        elif fmt == 'u8c4':
            alpha = mo.resize_linear_u8(np.repeat(crop[..., 3:], 3, axis=2), ow, oh)[..., :1]
            out.append(np.concatenate([mo.resize_linear_u8(np.ascontiguousarray(crop[..., :3]), ow, oh), alpha], axis=-1))
        else:
            out.append(cv16_area.resize_u16(crop, ow, oh))
    return np.stack(out)


# (n, H, W, rect, (out_W, out_H)): what each covers
CASES = [
    (3, 48, 64, (5, 3, 40, 30), (90, 70)),            # upscale, non-integer ratios
    (3, 120, 200, (3, 5, 190, 110), (61, 37)),        # downscale, non-integer
    (2, 160, 96, (10, 10, 50, 150), (120, 40)),       # up in x, down in y
    (2, 96, 160, (10, 10, 150, 50), (40, 120)),       # down in x, up in y
    (3, 90, 130, (1, 3, 120, 82), (60, 40)),          # exactly 2x down (u16: INTER_AREA's fast path)
    (2, 95, 127, (2, 1, 121, 90), (40, 30)),          # exactly 3x down
    (2, 33, 47, (4, 2, 40, 30), (1, 1)),              # 1 x 1 output
    (2, 33, 47, (4, 2, 40, 30), (1, 37)),             # 1 x N
    (2, 33, 47, (4, 2, 40, 30), (29, 1)),             # N x 1
    (2, 21, 19, (5, 7, 5, 7), (17, 9)),               # 1-pixel crop
    (2, 21, 19, (0, 7, 18, 7), (13, 5)),              # 1-row crop, down in x
    (2, 30, 41, (0, 0, 40, 29), (301, 203)),          # output larger than the frame
    (2, 31, 67, (3, 2, 66, 30), (129, 61)),           # W % 4 != 0 in and out
    (2, 40, 700, (20, 0, 619, 39), (250, 20)),        # 2.4x in x: u8c3 staged
    (2, 40, 1000, (10, 0, 684, 39), (250, 20)),       # 2.7x in x: just above the u8c3 cut-over
    (2, 40, 900, (20, 0, 819, 39), (250, 20)),        # 3.2x in x: u8c3 direct, u8c1 staged
    (2, 40, 1400, (20, 0, 1269, 39), (250, 20)),      # 5x in x: both direct
    (1, 300, 1000, (0, 0, 999, 299), (97, 29)),       # ~10x down in both axes
    (20, 64, 300, (7, 5, 290, 60), (700, 90)),        # many frames and tiles (XCD tile order), up
    (20, 300, 520, (7, 5, 510, 290), (170, 150)),     # many frames, down
]


@pytest.mark.parametrize('fmt', FORMATS)
@pytest.mark.parametrize('case', range(len(CASES)))
def test_matches_cv2_resize_model(dev, fmt, case):
    n, H, W, rect, (ow, oh) = CASES[case]
    frames = frames_of(fmt, n, H, W, seed=100 + case)
    got = ops.crop_resize(to_dev(frames, dev), rect, size=(ow, oh))
    torch.cuda.synchronize()
    assert tuple(got.shape) == (n, oh, ow) + frames.shape[3:]
    want = reference(fmt, frames, rect, ow, oh)
    g = to_np(got)
    assert np.array_equal(g, want), (fmt, CASES[case], int((g != want).sum()))


def test_u16_exact_2x_takes_the_area_branch(dev):
    """The 2x case above is only a test of the area branch where the float path would differ: check that it does on these frames."""
    from cv16_model import resize_linear_u16
    n, H, W, (l, t, r, b), (ow, oh) = CASES[4]
    frames = frames_of('u16c3', n, H, W, seed=104)
    crop = frames[0, t:b + 1, l:r + 1]
    assert not np.array_equal(cv16_area.area_fast_u16(crop), resize_linear_u16(crop, ow, oh))
    got = to_np(ops.crop_resize(to_dev(frames, dev), (l, t, r, b), size=(ow, oh)))
    assert np.array_equal(got[0], cv16_area.area_fast_u16(crop))


@pytest.mark.parametrize('fmt', FORMATS)
def test_same_size_is_todays_call(dev, fmt):
    n, H, W = 4, 70, 99
    frames = to_dev(frames_of(fmt, n, H, W, seed=5), dev)
    for rect in ((3, 2, 90, 60), (0, 0, W - 1, H - 1), (10, 10, 10, 10)):
        assert torch.equal(ops.crop_resize(frames, rect, size=(W, H)), ops.crop_resize(frames, rect))


@pytest.mark.parametrize('fmt', FORMATS)
def test_unaligned_stacks(dev, fmt):
    """Frames and output at every misalignment a stack of this format can have (u8: 1-3 bytes, u16: 2 bytes), cut to end exactly at the
    end of their allocation."""
    n, H, W, rect = 3, 37, 53, (2, 3, 50, 33)
    frames = frames_of(fmt, n, H, W, seed=9)
    raw = np.ascontiguousarray(frames).view(np.uint8).reshape(-1)
    step = 2 if fmt == 'u16c3' else 1
    call = getattr(_lib.lib, f'mf_crop_resize_to_{fmt}')
    for ow, oh in ((71, 45), (20, 11), (W, H)):
        want = reference(fmt, frames, rect, ow, oh)
        ob = want.nbytes
        for mis in range(step, 4, step):
            src = torch.empty(raw.size + mis, dtype=torch.uint8, device=dev)
            src[mis:] = torch.from_numpy(raw).to(dev)
            dst = torch.empty(ob + mis, dtype=torch.uint8, device=dev)
            work = torch.empty(_lib.lib.mf_crop_resize_workspace_bytes(ow, oh), dtype=torch.uint8, device=dev)
            rc = call(ctypes.c_void_p(src.data_ptr() + mis), ctypes.c_void_p(dst.data_ptr() + mis), n, W, H, *rect, ow, oh,
                      ctypes.c_void_p(work.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            assert rc == 0, _lib.lib.mf_last_error()
            torch.cuda.synchronize()
            got = dst[mis:].cpu().numpy().view(want.dtype).reshape(want.shape)
            assert np.array_equal(got, want), (fmt, ow, oh, mis)


@pytest.mark.parametrize('fmt', FORMATS)
def test_refusals_leave_the_output_untouched(dev, fmt):
    n, H, W = 2, 30, 40
    frames = to_dev(frames_of(fmt, n, H, W, seed=11), dev)
    out = torch.full((4 * 1024 * 1024,), 0xA5, dtype=torch.uint8, device=dev)
    work = torch.empty(_lib.lib.mf_crop_resize_workspace_bytes(32767, 32767), dtype=torch.uint8, device=dev)
    call = getattr(_lib.lib, f'mf_crop_resize_to_{fmt}')
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    F, O, Wk = (ctypes.c_void_p(t.data_ptr()) for t in (frames, out, work))
    good = (n, W, H, 2, 3, 30, 20, 25, 15)
    bad = [
        (None, O, *good, Wk), (F, None, *good, Wk), (F, O, *good, None), (F, F, *good, Wk),                 # null / aliasing pointers
        (F, O, n, W, H, 2, 3, 30, 20, 0, 15, Wk), (F, O, n, W, H, 2, 3, 30, 20, 25, 0, Wk),                 # output sizes
        (F, O, n, W, H, 2, 3, 30, 20, 32768, 15, Wk), (F, O, n, W, H, 2, 3, 30, 20, 25, -1, Wk),
        (F, O, n, W, H, 20, 3, 10, 20, 25, 15, Wk), (F, O, n, W, H, 2, 20, 30, 10, 25, 15, Wk),             # empty rectangles
        (F, O, n, W, H, -1, 3, 30, 20, 25, 15, Wk), (F, O, n, W, H, 2, 3, W, 20, 25, 15, Wk),               # out of the frame
        (F, O, n, W, H, 2, 3, 30, H, 25, 15, Wk),
        (F, O, 0, W, H, 2, 3, 30, 20, 25, 15, Wk), (F, O, n, 0, H, 0, 0, 0, 0, 25, 15, Wk),                 # shapes
        (F, O, 1 << 20, W, H, 2, 3, 30, 20, 32767, 32767, Wk),                                              # too many tiles
    ]
    for args in bad:
        rc = call(*args, st)
        assert rc == _lib.MF_ERR_INVALID_ARG, args
        assert f'mf_crop_resize_to_{fmt}' in _lib.lib.mf_last_error().decode(), _lib.lib.mf_last_error()
    # the whole text of one refusal of each kind, of this call and of the same-size call (the strings the library has always given)
    same = getattr(_lib.lib, f'mf_crop_resize_{fmt}')
    texts = [
        (call, (F, O, 0, W, H, 2, 3, 30, 20, 25, 15, Wk), f'mf_crop_resize_to_{fmt}: unsupported shape n=0 W=40 H=30'),
        (call, (F, O, n, W, H, 2, 3, 30, 20, 32768, 15, Wk), f'mf_crop_resize_to_{fmt}: unsupported output size 32768x15 (1 .. 32,767 each)'),
        (call, (F, O, n, W, H, 20, 3, 10, 20, 25, 15, Wk), f'mf_crop_resize_to_{fmt}: empty or out-of-frame crop rectangle (20, 3, 10, 20) for '
                                                           '40x30 (cv2.resize would fail on an empty source)'),
        (call, (F, O, 1 << 20, W, H, 2, 3, 30, 20, 32767, 32767, Wk), f'mf_crop_resize_to_{fmt}: too many tiles'),
        (same, (F, O, n, 0, H, 0, 0, 0, 0, Wk), f'mf_crop_resize_{fmt}: unsupported shape n=2 W=0 H=30'),
        (same, (F, O, n, W, H, 2, 3, W, 20, Wk), f'mf_crop_resize_{fmt}: empty or out-of-frame crop rectangle (2, 3, 40, 20) for 40x30 '
                                                 '(cv2.resize would fail on an empty source)'),
        (same, (F, O, 1 << 20, 32767, 32767, 2, 3, 30, 20, Wk), f'mf_crop_resize_{fmt}: too many tiles'),
    ]
    for fn, args, text in texts:
        assert fn(*args, st) == _lib.MF_ERR_INVALID_ARG, args
        assert _lib.lib.mf_last_error().decode() == text
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all())


def test_ops_size_checks(dev):
    frames = to_dev(frames_of('u8c3', 2, 20, 30, seed=1), dev)
    for size in ((0, 5), (5, 0), (32768, 5), (5.0, 5), (5,), 'ab', (True, 5), (5, 5, 5)):
        with pytest.raises(ValueError):
            ops.crop_resize(frames, (0, 0, 9, 9), size=size)
    with pytest.raises(ValueError):
        ops.crop_resize(frames, (0, 0, 9, 9), out=torch.empty((2, 20, 30, 3), dtype=torch.uint8, device=dev), size=(31, 20))
    out = torch.empty((2, 7, 31, 3), dtype=torch.uint8, device=dev)
    assert ops.crop_resize(frames, (0, 0, 9, 9), out=out, size=(31, 7)) is out


# ---- seeded random sweep ----------------------------------------------------------------------------------------------------------

# scale_x = crop width / output width at which each format's down instantiation leaves its staged form for the direct one: the widest span
# 256 output pixels can take, px (ceil(255 scale_x) + 3) bytes (+ slack), must fit its LDS row -- u8c3: kDownPitch 2048 (resize_body.h,
# slack 15), u8c1: kDown1Pitch 1024 (resize_c1_body.h, slack 3), u8c4: kDown4Pitch 2432 (resize_c4_body.h).  As the largest ceil(255 scale_x) that still fits.
# uint16 has one kernel (no staging): its draws sit at u8c3's.
CUT_CEIL = {'u8c3': 674, 'u8c1': 1018, 'u8c4': 605, 'u16c3': 674}
SWEEP_OFFSETS = {'u8c3': ((None, None), (1, 3), (2, 1), (3, 2)), 'u8c1': ((None, None), (1, 3), (2, 1), (3, 2)),
                 'u8c4': ((None, None), (1, 3), (2, 1), (3, 2), (8, 12)), 'u16c3': ((None, None), (2, 2), (0, 2))}
SWEEP_CLASSES = ('one', 'up', 'down2', 'down3', 'cut_below', 'cut_above', 'mixed', 'any')


def at_offset(a, dev, offset):
    """numpy stack -> device tensor of its dtype and shape: offset None = an allocation of exactly its bytes; else `offset` bytes into a
    zeroed buffer with 16 bytes to spare."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if offset is None:
        t = torch.from_numpy(raw).to(dev)
    else:
        buf = torch.zeros(raw.size + 16, dtype=torch.uint8, device=dev)
        t = buf[offset:offset + raw.size]
        t.copy_(torch.from_numpy(raw).to(dev))
        assert t.data_ptr() % 16 == offset % 16
    return (t.view(torch.uint16) if a.dtype == np.uint16 else t).view(a.shape)


def sweep_draw(rng, fmt):
    """One draw: (n, H, W, crop width and height, (out_W, out_H), class).  The crop is placed by the caller."""
    W, H, n = int(rng.integers(1, 301)), int(rng.integers(1, 201)), int(rng.integers(1, 4))
    kind = SWEEP_CLASSES[int(rng.integers(0, len(SWEEP_CLASSES)))]
    ri = lambda lo, hi: int(rng.integers(lo, hi + 1))                      # noqa: E731
    cw, ch = ri(1, W), ri(1, H)
    if kind == 'one':
        size = [(1, 1), (1, ri(1, 4 * ch)), (ri(1, 4 * cw), 1)][ri(0, 2)]
    elif kind == 'up':
        size = (ri(cw, 4 * cw), ri(ch, 4 * ch))
    elif kind in ('down2', 'down3') and min(W, H) >= int(kind[-1]):
        k = int(kind[-1])
        ow, oh = ri(1, W // k), ri(1, H // k)
        cw, ch, size = k * ow, k * oh, (ow, oh)
    elif kind in ('cut_below', 'cut_above'):
        # the widest output whose crop still fits the frame, then the crop width on this side of the cut: ceil(255 cw / oW) <= CUT_CEIL
        # just holds (below) or just fails (above)
        top = CUT_CEIL[fmt]
        ow = ri(1, max(1, (W - 1) * 255 // (top + 1)))
        below = top * ow // 255
        cw = min(W, max(1, below if kind == 'cut_below' else below + 1))
        size = (ow, ri(1, 2 * ch))
    elif kind == 'mixed':
        size = (ri(cw, 4 * cw), ri(1, ch)) if rng.random() < 0.5 else (ri(1, cw), ri(ch, 4 * ch))
    else:
        size = (ri(1, 4 * cw), ri(1, 4 * ch))
    return n, H, W, cw, ch, size, kind


@pytest.mark.parametrize('fmt', FORMATS)
def test_random_sweep(dev, fmt):
    """Seeded draws of frames of 1-300 x 1-200, 1-3 frames, crops and output sizes of every class above: 1 x 1, 1 x N and N x 1; up to 4x up;
    exactly 2x down (u16c3: the area branch) and 3x down; scale_x just below and just above the format's staged / direct cut-over; up in
    one axis and down in the other.  Each draw resizes one crop placed at random and one in the last rows of the frame (where a
    wavefront's last staged row ends past the stack and it takes the direct form), from every input / output offset of SWEEP_OFFSETS, the
    aligned input an allocation that ends with the stack."""
    rng = np.random.default_rng({'u8c3': 31, 'u8c1': 32, 'u16c3': 33, 'u8c4': 34}[fmt])
    pairs = SWEEP_OFFSETS[fmt]
    draws, kinds, cut = 300, set(), {'cut_below': 0, 'cut_above': 0}
    for d in range(draws):
        n, H, W, cw, ch, (ow, oh), kind = sweep_draw(rng, fmt)
        frames = frames_of(fmt, n, H, W, seed=1000 * d + 7)
        l = int(rng.integers(0, W - cw + 1))
        rects = [(l, int(rng.integers(0, H - ch + 1))), (int(rng.integers(0, W - cw + 1)), H - ch)]
        srcs = {si: at_offset(frames, dev, si) for si in {p[0] for p in pairs}}
        for (l, t) in rects:
            rect = (l, t, l + cw - 1, t + ch - 1)
            want = reference(fmt, frames, rect, ow, oh)
            for si, di in pairs:
                out = None if di is None else at_offset(np.zeros_like(want), dev, di)
                got = to_np(ops.crop_resize(srcs[si], rect, size=(ow, oh), out=out))
                assert np.array_equal(got, want), (fmt, d, kind, (n, H, W), rect, (ow, oh), si, di, int((got != want).sum()))
        kinds.add(kind)
        if kind in cut:
            cut[kind] += 1
    assert kinds == set(SWEEP_CLASSES) and min(cut.values()) >= 10, (kinds, cut)
