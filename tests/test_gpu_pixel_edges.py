"""-m gpu: the uint16 BGR ("u16c3"), single-channel uint8 ("u8c1") and 4-channel uint8 ("u8c4") warp and crop-resize kernels at the
edges where the uint8 BGR kernels broke before -- tiny frames, the 32767 size limits, stress geometries, non-finite and huge paths, extreme
sample values, unaligned stacks, the crop-resize corner sweep and a random campaign -- against references that do not use the GPU:
  * u16c3: tests/cv16_model.py (the model of cv2.remap / cv2.resize on CV_16UC3);
  * u8c1:  channel 0 of the C oracle (warp) and of the NumPy oracle (crop-resize) on the frame repeated three times (cv2's 8-bit
           remap and resize work per channel);
  * u8c4:  the same oracles split per channel: channels 0-2 are the BGR result of X[..., :3] with border[:3], channel 3 is channel 0 of
           the result of the alpha plane repeated three times with border (a, a, a) (a = 0 for a 3-component border); crop values,
           rectangle and degenerate count are the BGR call's, and the alpha call must agree on them.
Where a case has cells without a homography, the GPU's count must equal clib.cell_table's, and frames are compared only where it is 0."""
import itertools
import os

import numpy as np
import pytest

import cv16_model as m
import plan_words

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

PIXELS = ('u16c3', 'u8c1', 'u8c4')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


# ---- frames, device buffers, references ---------------------------------------------------------------------------------------------

def rgb(g):
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=-1))


def rand_frames(pixel, rng, n, H, W):
    if pixel == 'u16c3':
        return rng.integers(0, 65536, (n, H, W, 3), dtype=np.uint16)
    if pixel == 'u8c4':
        return rng.integers(0, 256, (n, H, W, 4), dtype=np.uint8)
    return rng.integers(0, 256, (n, H, W), dtype=np.uint8)


def border8(border):
    """A border colour as the uint8 kernels take it, restated here (not through ops): clamp(round(v), 0, 255) per component, missing
    components 0 (cv::Scalar's padding)."""
    v = [int(np.clip(round(float(c)), 0, 255)) for c in border[:4]]
    return tuple(v + [0] * (4 - len(v)))


def put(a, dev, offset=None):
    """numpy frames -> device tensor of the same dtype and shape.  offset=None: an allocation of exactly the frames' bytes; else the
    frames start `offset` bytes into a zeroed buffer with 16 bytes to spare."""
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    if offset is None:
        t = torch.from_numpy(raw).to(dev)
    else:
        buf = torch.zeros(raw.size + 16, dtype=torch.uint8, device=dev)
        t = buf[offset:offset + raw.size]
        t.copy_(torch.from_numpy(raw).to(dev))
        assert t.data_ptr() % 16 == offset % 16
    if a.dtype == np.uint16:
        t = t.view(torch.uint16)
    return t.view(a.shape)


def get(t):
    if t.dtype == torch.uint16:
        return t.contiguous().view(torch.uint8).cpu().numpy().view(np.uint16)
    return t.cpu().numpy()


def dev64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def bad_cells(W, H, R, C, unstab, stab):
    from oracle import clib
    return sum(clib.cell_table(W, H, R, C, unstab[f], stab[f])[1] for f in range(unstab.shape[0]))


def ref_warp(pixel, frames, R, C, unstab, stab, border):
    """(frames, per-frame crop values, degenerate-cell count) of the reference; frames and crop are None where the count is not 0."""
    from oracle import clib
    n, H, W = frames.shape[:3]
    bad = bad_cells(W, H, R, C, unstab, stab)
    if bad:
        return None, None, bad
    if pixel == 'u16c3':
        want, crop = m.warp_clip_u16(frames, R, C, unstab, stab, border)
        return want, crop, 0
    if pixel == 'u8c4':
        return ref_warp_u8c4(frames, R, C, unstab, stab, border)
    b = int(np.clip(round(float(border[0])), 0, 255))
    want, crop, bad8 = clib.warp_clip(rgb(frames), R, C, unstab, stab, (b, b, b), use_bbox=True, openmp=True)
    assert bad8 == 0
    return want[..., 0], crop, 0


def ref_warp_u8c4(frames, R, C, unstab, stab, border):
    """The split oracle of a 4-channel clip with no degenerate cell: (frames, crop values, 0)."""
    from oracle import clib
    b, g, r, a = border8(border)
    want_c, crop, bad = clib.warp_clip(np.ascontiguousarray(frames[..., :3]), R, C, unstab, stab, (b, g, r), use_bbox=True, openmp=True)
    want_a, crop_a, bad_a = clib.warp_clip(rgb(frames[..., 3]), R, C, unstab, stab, (a, a, a), use_bbox=True, openmp=True)
    assert bad == bad_a == 0 and np.array_equal(crop, crop_a)
    return np.concatenate([want_c, want_a[..., :1]], axis=-1), crop, 0


def gpu_warp(dev, frames, R, C, unstab, stab, border, offset=None):
    """ops.warp from (and into) stacks at `offset`: (frames, per-frame crop values, degenerate-cell count, table)."""
    from meshflow_amd import ops
    n, H, W = frames.shape[:3]
    table = ops.cell_table(dev64(unstab, dev), dev64(stab, dev), W, H, R, C)
    src = put(frames, dev, offset)
    dst = put(np.full_like(frames, 0xEE), dev, offset)
    ops.warp(src, table, border, out=dst)
    torch.cuda.synchronize()
    return get(dst), table.crop.cpu().numpy(), int(table.status.item()), table


def check_warp(dev, pixel, frames, R, C, unstab, stab, border, offsets=(None,), what=''):
    """GPU == reference (frames, crop values, degenerate count) from every offset; returns (compared?, grey or 4-channel paths seen)."""
    want, want_crop, want_bad = ref_warp(pixel, frames, R, C, unstab, stab, border)
    seen = set()
    for off in offsets:
        got, crop, bad, table = gpu_warp(dev, frames, R, C, unstab, stab, border, off)
        assert bad == want_bad, (what, off, bad, want_bad)
        if want_bad:
            continue
        assert np.array_equal(got, want), (what, off, int((got != want).sum()))
        assert np.array_equal(crop, want_crop), (what, off)
        if pixel == 'u8c1':
            seen |= plan_words.grey_paths(table, aligned=off is None or off % 4 == 0)
        elif pixel == 'u8c4':
            seen |= plan_words.c4_paths(table, off)
    return not want_bad, seen


def clip(n, H, W, R, C, seed, **kw):
    from meshflow_amd import synthetic
    from oracle import meshflow_oracle as mo
    disp, hom = synthetic.motion(n, R, C, seed=seed, **kw)
    stab = mo.stabilized_vertex_displacements(W, H, 0, disp, hom, 3, 10)
    return disp, stab


# ---- 1. tiny frames -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('pixel', PIXELS)
def test_tiny_frames_equal_the_reference(dev, pixel):
    """test_gpu_parity.py::test_tiny_frames_equal_the_oracle for the new pixel types: frames of 2-100 columns and 2-40 rows (the
    restated `deep` bound and the x0 + 3 < W store split), meshes of 1-3 rows and columns, still and moving, 1 and 3 frames; then meshes
    finer than the pixel grid (repeated vertices: the degenerate count is the oracle's, nothing faults)."""
    rng = np.random.default_rng(11)
    border = {'u16c3': (9, 60000, 65535), 'u8c1': (9, 0, 0), 'u8c4': (9, 140, 0, 201)}[pixel]
    n = 0
    for W, H, (R, C), nfr in itertools.product((2, 3, 4, 5, 6, 7, 8, 12, 31, 32, 33, 64, 100), (2, 3, 4, 5, 8, 9, 12, 13, 17, 40),
                                               ((1, 1), (1, 2), (2, 1), (2, 3), (3, 3)), (1, 3)):
        if C > W - 1 or R > H - 1:
            continue
        frames = rand_frames(pixel, rng, nfr, H, W)
        unstab = np.zeros((nfr, R + 1, C + 1, 2))
        scale = rng.choice([0.0, 0.3, 1.5, 4.0])
        stab = rng.normal(0, 1, size=(nfr, 1, 1, 2)) * scale + rng.normal(0, 0.2, size=(nfr, R + 1, C + 1, 2)) * min(scale, 1.0)
        compared, _ = check_warp(dev, pixel, frames, R, C, unstab, stab, border, what=(W, H, R, C, nfr, float(scale)))
        n += compared
    assert n > 800
    for (W, H), (R, C) in itertools.product(((2, 2), (3, 5), (4, 4), (8, 3), (16, 16), (33, 20)), ((2, 2), (4, 4), (8, 16), (16, 8), (40, 40), (64, 64))):
        frames = rand_frames(pixel, rng, 2, H, W)
        unstab = np.zeros((2, R + 1, C + 1, 2))
        stab = rng.normal(0, 0.3, size=(2, R + 1, C + 1, 2))
        check_warp(dev, pixel, frames, R, C, unstab, stab, (1, 2, 3), what=('fine mesh', W, H, R, C))


# ---- 2. size limits and aspect ratios -------------------------------------------------------------------------------------------------

LIMITS = [(24, 32764, 1, 64), (40, 16384, 2, 64), (16388, 32, 64, 1), (20, 8196, 1, 3), (2, 32767, 1, 1), (32767, 3, 64, 1), (9, 32767, 2, 33),
          (32767, 4, 9, 1)]
GREY_TALL = [(32767, 80, 64, 1), (32764, 84, 64, 2), (30000, 128, 48, 2)]      # the grey window at rows up to 32,7xx (sy0 in float32)
C4_TALL = [(32767, 84, 64, 2), (32766, 56, 64, 1), (32761, 72, 48, 2), (32759, 64, 64, 1)]   # the 4-byte window there (and its right clamp)


def limit_case(H, W, R, C):
    from meshflow_amd import synthetic
    from oracle import meshflow_oracle as mo
    disp, hom = synthetic.motion(2, R, C, seed=H + W, jitter_sigma=0.6, translation_sigma=2.0)
    stab = mo.stabilized_vertex_displacements(W, H, 0, disp, hom, 3, 10)
    return disp, stab


@pytest.mark.parametrize('pixel,H,W,R,C', [(p,) + g for p in PIXELS for g in LIMITS] + [('u8c1',) + g for g in GREY_TALL] +
                         [('u8c4',) + g for g in C4_TALL])
def test_size_limits_equal_the_reference(dev, pixel, H, W, R, C):
    """test_gpu_parity.py::test_warp_extreme_aspect_ratios_bit_exact's frames at the size limits (coordinates up to 32767), and for grey
    and 4-channel frames tall frames whose staged windows start at rows up to 32,7xx (sy0 recovered in float32); 4-channel frames from an
    aligned stack and one 8 bytes past a 16-byte boundary."""
    disp, stab = limit_case(H, W, R, C)
    frames = rand_frames(pixel, np.random.default_rng(H * W), 2, H, W)
    border, offsets = ((200, 65535, 0, 99), (None, 8)) if pixel == 'u8c4' else ((200, 65535, 0), (None,))
    compared, _ = check_warp(dev, pixel, frames, R, C, disp, stab, border, offsets, what=(H, W, R, C))
    assert compared


# ---- 3. stress geometries -----------------------------------------------------------------------------------------------------------

# 4-channel stacks: an allocation of exactly the stack, and 0-3, 4, 8 and 12 bytes into a buffer (4, 8, 12: STAGE on, the 16-byte
# global->LDS chunks off a 16-byte boundary)
C4_OFFSETS = (None, 0, 1, 2, 3, 4, 8, 12)
STRESS = [(130, 260, 4, 4, 8.0, 1), (130, 260, 4, 4, 20.0, 2), (64, 96, 8, 8, 6.0, 3), (200, 300, 64, 64, 0.4, 4), (17, 23, 2, 3, 1.0, 5)]


def stress_case(H, W, R, C, sigma, seed):
    from meshflow_amd import synthetic
    n = np.arange(2 * (R + 1) * (C + 1) * 2, dtype=np.int64).reshape(2, R + 1, C + 1, 2)
    return np.zeros((2, R + 1, C + 1, 2)), sigma * synthetic.normal(n, seed=100 + seed)


@pytest.mark.parametrize('H,W,R,C,sigma,seed', STRESS)
@pytest.mark.parametrize('pixel', PIXELS)
def test_stress_geometries_equal_the_reference(dev, pixel, H, W, R, C, sigma, seed):
    """Non-affine and folded quads, more than 8 candidate cells, the 64 x 64 mesh, a frame smaller than a tile; from an aligned and an
    unaligned stack (2 mod 4 for uint16, 1 and 3 for grey, every offset of C4_OFFSETS for 4-channel frames)."""
    unstab, stab = stress_case(H, W, R, C, sigma, seed)
    frames = rand_frames(pixel, np.random.default_rng(seed), 2, H, W)
    offsets = {'u16c3': (None, 2), 'u8c1': (None, 1, 3), 'u8c4': C4_OFFSETS}[pixel]
    border = {'u16c3': (65535, 0, 65535), 'u8c1': (255,), 'u8c4': (255, 0, 255, 17)}[pixel]
    check_warp(dev, pixel, frames, R, C, unstab, stab, border, offsets, what=(H, W, R, C, sigma))


# ---- 4. non-finite and huge paths ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('pixel', PIXELS)
def test_non_finite_and_huge_paths(dev, pixel):
    """test_gpu_parity.py::test_non_finite_and_huge_paths_never_fault for the new pixel types: NaN, +-inf, 1e300, 1e18, 1e7, -1e5 and a
    denormal at one vertex, in one frame, everywhere: the oracle's degenerate count, its frames where that is 0, no fault."""
    rng = np.random.default_rng(2)
    H, W, R, C, n = 48, 64, 3, 4, 3
    frames = rand_frames(pixel, rng, n, H, W)
    unstab = np.zeros((n, R + 1, C + 1, 2))
    for poison in (np.nan, np.inf, -np.inf, 1e300, 1e18, 1e7, -1e5, 5e-324):
        for where in range(3):
            stab = rng.normal(0, 0.5, size=(n, R + 1, C + 1, 2))
            if where == 0:
                stab[1, 2, 2, 0] = poison
            elif where == 1:
                stab[1] = poison
            else:
                stab[:] = poison
            check_warp(dev, pixel, frames, R, C, unstab, stab, (1, 2, 3), what=(poison, where))


# ---- 5. uint16 values at the extremes -----------------------------------------------------------------------------------------------

def extreme_frames(kind, n, H, W):
    if kind == 'max':
        return np.full((n, H, W, 3), 65535, np.uint16)
    if kind == 'checker':
        y, x = np.indices((H, W))
        c = np.where(((x + y) & 1)[..., None] == 1, 65535, 0).astype(np.uint16)
        c = np.repeat(c, 3, axis=-1)
        c[..., 1] = 65535 - c[..., 1]
        return np.ascontiguousarray(np.broadcast_to(c, (n, H, W, 3)))
    return np.random.default_rng(n * H + W).integers(65000, 65536, (n, H, W, 3), dtype=np.uint16)


@pytest.mark.parametrize('kind', ['max', 'checker', 'high'])
@pytest.mark.parametrize('border', [(65535, 0, 65535), (-3, 70000.4, 12.5), (0, 0, 255)])
def test_uint16_extreme_values_warp_and_crop_resize(dev, kind, border):
    """Samples at and near 65535 (the fast blend has no clamp: warp.hip's bound on its rounding), the extreme border colours and ones
    ops._border must clamp and round; sub-pixel motion -- a half-pixel shift and strong jitter -- through warp and crop_resize."""
    from meshflow_amd import ops
    F, H, W, R, C = 3, 72, 100, 3, 5
    frames = extreme_frames(kind, F, H, W)
    unstab = np.zeros((F, R + 1, C + 1, 2))
    half = unstab.copy()
    half[..., 0] = 0.5
    half[..., 1] = -0.25
    jit = np.random.default_rng(7).normal(0, 2.0, (F, R + 1, C + 1, 2))
    for stab in (half, jit):
        compared, _ = check_warp(dev, 'u16c3', frames, R, C, unstab, stab, border, offsets=(None, 2), what=(kind, border))
        assert compared
    fr = put(frames, dev)
    for rect in ((0, 0, W - 1, H - 1), (1, 1, W - 2, H - 2), (3, 5, 44, 31), (50, 0, 50, H - 1), (0, 10, W - 1, 10)):
        got = get(ops.crop_resize(fr, rect))
        assert np.array_equal(got, m.crop_frames_u16(frames, rect)), (kind, rect)


# ---- 5b. 4-channel values at the extremes ------------------------------------------------------------------------------------------

def extreme_frames_u8c4(kind, n, H, W):
    if kind == 'max':
        return np.full((n, H, W, 4), 255, np.uint8)
    if kind == 'checker':
        y, x = np.indices((H, W))
        c = np.repeat(np.where(((x + y) & 1)[..., None] == 1, 255, 0).astype(np.uint8), 4, axis=-1)
        c[..., 3] = 255 - c[..., 3]                                    # alpha the inverse of B G R
        return np.ascontiguousarray(np.broadcast_to(c, (n, H, W, 4)))
    return np.random.default_rng(n * H + W).integers(250, 256, (n, H, W, 4), dtype=np.uint8)


@pytest.mark.parametrize('kind', ['max', 'checker', 'high'])
@pytest.mark.parametrize('border', [(255, 255, 255, 255), (-3, 300.4, 12.7, 254.5), (0, 0, 255)])
def test_u8c4_extreme_values_warp_and_crop_resize(dev, kind, border):
    """4-channel samples at and near 255 (blend_c4 and vpass_c4 have no clamp), a checkerboard whose alpha is the inverse of its colour,
    the all-255 border, one that ops must clamp and round per component (-3 -> 0, 300.4 -> 255, 12.7 -> 13, 254.5 -> 254: round half
    to even, as cv::saturate_cast) and a 3-component one (alpha 0); a half-pixel shift and strong jitter through warp (aligned, 4 bytes
    and 1 byte into a buffer), then crop_resize at the same size and to a chosen size."""
    from meshflow_amd import ops
    F, H, W, R, C = 3, 72, 100, 3, 5
    frames = extreme_frames_u8c4(kind, F, H, W)
    unstab = np.zeros((F, R + 1, C + 1, 2))
    half = unstab.copy()
    half[..., 0] = 0.5
    half[..., 1] = -0.5
    jit = np.random.default_rng(7).normal(0, 2.0, (F, R + 1, C + 1, 2))
    for stab in (half, jit):
        compared, _ = check_warp(dev, 'u8c4', frames, R, C, unstab, stab, border, offsets=(None, 4, 1), what=(kind, border))
        assert compared
    fr = put(frames, dev)
    for rect in ((0, 0, W - 1, H - 1), (1, 1, W - 2, H - 2), (3, 5, 44, 31), (50, 0, 50, H - 1), (0, 10, W - 1, 10)):
        assert np.array_equal(get(ops.crop_resize(fr, rect)), ref_crop('u8c4', frames, rect)), (kind, rect)
        for size in ((37, 23), (W * 2 + 3, H + 1)):
            l, t, r, b = rect
            want = np.stack([ref_resize_u8c4(f[t:b + 1, l:r + 1], *size) for f in frames])
            assert np.array_equal(get(ops.crop_resize(fr, rect, size=size)), want), (kind, rect, size)


# ---- 6. crop-resize corner sweep ------------------------------------------------------------------------------------------------------

def ref_resize_u8c4(crop, ow, oh):
    """cv2.resize of one 4-channel crop: the NumPy oracle on B G R, and channel 0 of it on the alpha plane repeated three times."""
    from oracle import meshflow_oracle as mo
    c = mo.resize_linear_u8(np.ascontiguousarray(crop[..., :3]), ow, oh)
    a = mo.resize_linear_u8(rgb(crop[..., 3]), ow, oh)[..., :1]
    return np.concatenate([c, a], axis=-1)


def ref_crop(pixel, frames, rect):
    from oracle import meshflow_oracle as mo
    if pixel == 'u16c3':
        return m.crop_frames_u16(frames, rect)
    if pixel == 'u8c4':
        H, W = frames.shape[1:3]
        l, t, r, b = rect
        return np.stack([ref_resize_u8c4(f[t:b + 1, l:r + 1], W, H) for f in frames])
    return np.ascontiguousarray(np.stack(mo.crop_frames(list(rgb(frames)), rect))[..., 0])


def rects_of(rng, W, H):
    rects = {(0, 0, W - 1, H - 1), (0, 0, 0, 0), (W - 1, H - 1, W - 1, H - 1), (0, H - 1, W - 1, H - 1), (W - 1, 0, W - 1, H - 1)}
    for _ in range(3):
        l, r = sorted(rng.integers(0, W, size=2))
        t, b = sorted(rng.integers(0, H, size=2))
        rects.add((int(l), int(t), int(r), int(b)))
    return sorted(rects)


@pytest.mark.parametrize('pixel', PIXELS)
def test_crop_resize_corner_cases(dev, pixel):
    """test_gpu_parity.py::test_crop_resize_and_score_corner_cases (the crop-resize half) for the new pixel types: 1-300 columns, 1-40
    rows, 1 and 3 frames, one pixel / row / column, the whole frame and random rectangles; inputs and outputs at every offset the dtype
    allows (uint16: 0 and 2 mod 4; grey: 0-3; 4-channel: 0-3 and 8 / 12 mod 16).  The aligned input is an allocation of exactly the stack's bytes, so the last tile of
    every stack ends at the end of its allocation (resize8c1_kernel's staged / direct choice)."""
    from meshflow_amd import ops
    rng = np.random.default_rng(5)
    pairs = {'u16c3': ((None, None), (2, 2), (2, 0), (0, 2)), 'u8c1': ((None, None), (1, 3), (2, 1), (3, 2), (0, 1)),
             'u8c4': ((None, None), (1, 3), (2, 1), (3, 2), (0, 1), (8, 12))}[pixel]
    n = 0
    # (259-261 and 271-273: where tile 0 of the last rows of the last frame flips between staged and direct -- u8c4: 4 W against the staged
    # row's 1040 bytes, u8c1: W against 272)
    for W, H, nfr in itertools.product((1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 100, 255, 256, 257, 259, 260, 261, 271, 272, 273, 300),
                                       (1, 2, 3, 5, 8, 9, 17, 33, 40), (1, 3)):
        frames = rand_frames(pixel, rng, nfr, H, W)
        srcs = {off: put(frames, dev, off) for off in {p[0] for p in pairs}}
        dsts = {off: put(np.zeros_like(frames), dev, off) for off in {p[1] for p in pairs} if off is not None}
        for rect in rects_of(rng, W, H):
            n += 1
            want = ref_crop(pixel, frames, rect)
            for si, di in pairs:
                got = get(ops.crop_resize(srcs[si], rect, out=dsts.get(di)))
                assert np.array_equal(got, want), (W, H, nfr, rect, si, di)
    assert n > 1500


@pytest.mark.parametrize('W', [260, 261, 262, 263, 513, 1026, 1027, 1920])
def test_grey_crop_resize_wide_frames(dev, W):
    """resize8c1_kernel beyond one 256-column tile, every W & 3, stacks of 3 frames from each byte offset: the staged form (rows copied
    from the dword below the first byte) and the direct one (a span or stack end the copy must not reach) against the oracle."""
    from meshflow_amd import ops
    rng = np.random.default_rng(W)
    H = 37
    frames = rand_frames('u8c1', rng, 3, H, W)
    for rect in [(0, 0, W - 1, H - 1), (1, 2, W - 2, H - 1), (W // 3, 5, W - 4, 30), (W - 120, 0, W - 1, 7), (0, H - 9, 200, H - 1)] + rects_of(rng, W, H):
        want = ref_crop('u8c1', frames, rect)
        for off in (None, 0, 1, 2, 3):
            got = get(ops.crop_resize(put(frames, dev, off), rect))
            assert np.array_equal(got, want), (W, rect, off)


# ---- 7. random campaign ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('pixel', PIXELS)
def test_randomised_campaign(dev, pixel):
    """tests/fuzz_parity.py's geometries (warp incl. W % 4 != 0, borders, folded quads; crop + resize) on the new pixel types."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('fuzz_parity', os.path.join(os.path.dirname(os.path.abspath(__file__)), 'fuzz_parity.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    bad, stats = mod.run(190, 3, pixel=pixel)
    assert bad == 0 and stats['warp'] > 80 and stats['resize'] > 25 and stats['jacobi'] == 0


# ---- 8. path censuses -----------------------------------------------------------------------------------------------------------

GREY_PATHS = {'window160', 'window112', 'hot_window', 'pair_window', 'staged_narrow', 'border_region', 'w_mod4', 'unaligned'}


def test_grey_path_census(dev):
    """Every grey warp path is reached by a compared frame of the geometries above (plan and region words decoded by
    tests/plan_words.py): the grey window at pitch 160 and 112, HOT and PAIR through it, a staged footprint in a frame too narrow for
    it, a BORDER window, W % 4 != 0 and an unaligned stack.  A 1080p clip with a 16 x 16 mesh adds the config-2 geometry."""
    seen = set()
    for H, W, R, C in LIMITS + GREY_TALL:
        disp, stab = limit_case(H, W, R, C)
        seen |= check_warp(dev, 'u8c1', rand_frames('u8c1', np.random.default_rng(H * W), 2, H, W), R, C, disp, stab, (200,), what=(H, W))[1]
    for H, W, R, C, sigma, seed in STRESS:
        unstab, stab = stress_case(H, W, R, C, sigma, seed)
        seen |= check_warp(dev, 'u8c1', rand_frames('u8c1', np.random.default_rng(seed), 2, H, W), R, C, unstab, stab, (255,), (None, 1),
                           what=(H, W))[1]
    for F, H, W, R, C, jitter in ((3, 1080, 1920, 16, 16, 1.5), (3, 96, 64, 2, 2, 0.5)):
        disp, stab = clip(F, H, W, R, C, seed=W + F, jitter_sigma=jitter)
        seen |= check_warp(dev, 'u8c1', rand_frames('u8c1', np.random.default_rng(H), F, H, W), R, C, disp, stab, (77,), what=(H, W))[1]
    assert GREY_PATHS <= seen, sorted(GREY_PATHS - seen)


C4_PATHS = {'window', 'window_compact', 'hot_window', 'pair_window', 'window_clamped', 'border_region', 'w_mod4', 'unaligned', 'aligned4_not16'}
C4_CENSUS_CLIPS = [(3, 1080, 1920, 16, 16, 1.5), (3, 96, 64, 2, 2, 0.5), (3, 200, 84, 4, 2, 0.5), (3, 120, 60, 4, 2, 0.3), (3, 160, 76, 4, 2, 0.8),
                   (3, 120, 48, 2, 2, 0.3), (3, 96, 52, 2, 1, 0.5), (3, 200, 44, 4, 2, 0.2)]      # W < 56: see 'staged_narrow' below


def test_c4_path_census(dev):
    """Every 4-channel warp path is reached by a compared frame (plan and region words decoded by tests/plan_words.py): the 4-byte window
    cut from a wide and a COMPACT window, HOT and PAIR through it, its first column clamped to W - 56, a BORDER window, W % 4 != 0, an
    unaligned stack and one 4-byte but not 16-byte aligned.  'staged_narrow' is never reached: the plan stages footprints only in frames
    with W % 4 == 0 and 3 W >= 160 (cell_table.hip), that is W >= 56, so warp8c4_footprint's W >= MF_C4_COLS guard never declines a
    staged window -- the frames of 44-52 columns above check that it stays so."""
    seen = set()
    for H, W, R, C in LIMITS + C4_TALL:
        disp, stab = limit_case(H, W, R, C)
        seen |= check_warp(dev, 'u8c4', rand_frames('u8c4', np.random.default_rng(H * W), 2, H, W), R, C, disp, stab, (200, 1, 2, 3),
                           (None, 8), what=(H, W))[1]
    for H, W, R, C, sigma, seed in STRESS:
        unstab, stab = stress_case(H, W, R, C, sigma, seed)
        seen |= check_warp(dev, 'u8c4', rand_frames('u8c4', np.random.default_rng(seed), 2, H, W), R, C, unstab, stab, (255, 0, 0, 9),
                           (None, 1, 4), what=(H, W))[1]
    for F, H, W, R, C, jitter in C4_CENSUS_CLIPS:
        disp, stab = clip(F, H, W, R, C, seed=W + F, jitter_sigma=jitter)
        seen |= check_warp(dev, 'u8c4', rand_frames('u8c4', np.random.default_rng(H), F, H, W), R, C, disp, stab, (77, 78, 79, 80),
                           (None, 12), what=(H, W))[1]
    assert C4_PATHS <= seen, sorted(C4_PATHS - seen)
    assert 'staged_narrow' not in seen
