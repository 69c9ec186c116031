"""-m gpu: 4-channel uint8 frames -- mf_warp_u8c4 / mf_warp_bounds_u8c4 / mf_warp_clip_u8c4 / mf_crop_resize_u8c4 /
mf_crop_resize_to_u8c4 through `ops` and `stabilize_resident`.

cv2.remap's and cv2.resize's 8-bit paths work per channel, so the contract is: for frames X (n, H, W, 4) and border (b, g, r, a), the
result's channels 0-2 are byte for byte the u8c3 result of X[..., 0:3] with border (b, g, r), channel 3 is the u8c1 result of X[..., 3]
with border a, and the per-frame crop values, the clip rectangle and the degenerate-mesh status are the u8c3 call's.  A 3-component
border means a = 0 (cv::Scalar's padding)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def dev64(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)


def motion(F, H, W, R, C, seed, jitter, kind='jitter'):
    from meshflow_amd import synthetic
    from oracle import meshflow_oracle as mo
    if kind == 'shift':                            # large global translation: wide border rings, many uncovered pixels
        disp, hom = synthetic.motion(F, R, C, seed=seed, translation_sigma=12.0, jitter_sigma=jitter)
    else:
        disp, hom = synthetic.motion(F, R, C, seed=seed, jitter_sigma=jitter)
    stab = mo.stabilized_vertex_displacements(W, H, 0, disp, hom, 3, 10)
    return disp, hom, stab


def bgra(F, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (F, H, W, 4), dtype=np.uint8)


def split_reference(dev, fr, disp, stab, R, C, border):
    """The u8c3 warp of fr[..., :3] with border[:3] and the u8c1 warp of fr[..., 3] with border[3], interleaved: (frames, crop, rectangle)
    -- after checking that the two calls agree on crop values and rectangle."""
    from meshflow_amd import ops
    F, H, W, _ = fr.shape
    d = torch.from_numpy(fr).to(dev)
    t3 = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
    o3 = ops.warp(d[..., :3].contiguous(), t3, tuple(border[:3]))
    t1 = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
    o1 = ops.warp(d[..., 3].contiguous(), t1, (border[3],))
    torch.cuda.synchronize()
    t3.check()
    assert torch.equal(t3.crop, t1.crop) and torch.equal(t3.clip_bounds, t1.clip_bounds)
    want = torch.cat([o3, o1[..., None]], dim=-1).cpu().numpy()
    return want, t3.crop.cpu().numpy().copy(), t3.clip_bounds.cpu().numpy().copy()


GEOMS = [  # F, H, W, R, C, jitter, kind
    (2, 2, 2, 1, 1, 0.3, 'jitter'),              # the smallest frame
    (3, 2, 9, 1, 2, 0.3, 'jitter'),
    (3, 9, 2, 2, 1, 0.3, 'jitter'),
    (3, 131, 257, 5, 7, 1.0, 'jitter'),          # W % 4 != 0: no staged windows; W, H not multiples of 32 x 8
    (3, 75, 101, 6, 4, 2.0, 'shift'),
    (4, 72, 100, 3, 5, 6.0, 'jitter'),           # strong jitter: border taps and uncovered pixels
    (2, 60, 56, 2, 3, 1.0, 'jitter'),            # W = 56: the narrowest frame with a 4-byte window
    (4, 144, 256, 16, 16, 1.5, 'shift'),
    (2, 96, 128, 32, 32, 0.5, 'jitter'),
    (2, 97, 132, 8, 32, 0.8, 'jitter'),          # R != C
    (3, 1080, 1920, 16, 16, 1.5, 'jitter'),
    (2, 1080, 1920, 32, 32, 1.0, 'shift'),
]


@pytest.mark.parametrize('F,H,W,R,C,jitter,kind', GEOMS)
def test_warp_equals_u8c3_and_u8c1(dev, F, H, W, R, C, jitter, kind):
    from meshflow_amd import ops
    disp, _, stab = motion(F, H, W, R, C, seed=W + F, jitter=jitter, kind=kind)
    fr = bgra(F, H, W, seed=H)
    border = (11, 122, 233, 44)
    want, want_crop, want_bounds = split_reference(dev, fr, disp, stab, R, C, border)
    d = torch.from_numpy(fr).to(dev)
    table = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
    out = ops.warp(d, table, border)
    torch.cuda.synchronize()
    table.check()
    got = out.cpu().numpy()
    assert got.shape == (F, H, W, 4) and out.dtype == torch.uint8
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(table.crop.cpu().numpy(), want_crop)
    assert table.clip_bounds.cpu().numpy().tolist() == want_bounds.tolist()
    # mf_warp_bounds_u8c4: the rectangle in the caller's tensor
    bounds = torch.empty(4, dtype=torch.int32, device=dev)
    t2 = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C, bounds=bounds)
    out2 = ops.warp(d, t2, border, bounds=bounds)
    torch.cuda.synchronize()
    assert torch.equal(out2, out) and bounds.cpu().numpy().tolist() == want_bounds.tolist()


def test_small_clip_against_the_oracle(dev):
    """The C oracle per channel group: B G R through its u8c3 warp, alpha as a frame repeated three times (channel 0); the default
    3-component border gives alpha 0."""
    from meshflow_amd import ops
    from oracle import clib
    F, H, W, R, C = 4, 64, 96, 4, 4
    disp, _, stab = motion(F, H, W, R, C, seed=5, jitter=2.0)
    fr = bgra(F, H, W, seed=6)
    alpha3 = np.ascontiguousarray(np.repeat(fr[..., 3:], 3, axis=-1))
    want_c, crop, bad = clib.warp_clip(np.ascontiguousarray(fr[..., :3]), R, C, disp, stab, (0, 0, 255))
    assert bad == 0
    for border, a in (((0, 0, 255), 0), ((0, 0, 255, 77), 77)):
        want_a, crop_a, _ = clib.warp_clip(alpha3, R, C, disp, stab, (a, a, a))
        table = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
        out = ops.warp(torch.from_numpy(fr).to(dev), table, border).cpu().numpy()
        np.testing.assert_array_equal(out[..., :3], want_c)
        np.testing.assert_array_equal(out[..., 3], want_a[..., 0])
        np.testing.assert_array_equal(table.crop.cpu().numpy(), crop)
        np.testing.assert_array_equal(crop_a, crop)
    out = ops.warp(torch.from_numpy(fr).to(dev), ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)).cpu().numpy()
    np.testing.assert_array_equal(out[..., 3], clib.warp_clip(alpha3, R, C, disp, stab, (0, 0, 0))[0][..., 0])


@pytest.mark.parametrize('H,W,R,C,jitter,kind', [(72, 100, 3, 5, 6.0, 'jitter'), (144, 256, 8, 8, 2.0, 'shift'), (97, 131, 4, 6, 4.0, 'shift')])
def test_coverage_mask(dev, H, W, R, C, jitter, kind):
    """Input alpha 255, default border: output alpha is 0 on every pixel no cell owns or whose 2 x 2 footprint lies wholly outside the
    frame, 255 on every pixel whose four taps lie inside (both sets from the oracle's coordinate maps)."""
    from meshflow_amd import ops
    from oracle import clib
    F = 3
    disp, _, stab = motion(F, H, W, R, C, seed=H + R, jitter=jitter, kind=kind)
    fr = bgra(F, H, W, seed=W)
    fr[..., 3] = 255
    table = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
    alpha = ops.warp(torch.from_numpy(fr).to(dev), table)[..., 3].cpu().numpy()
    n_out = n_in = 0
    for f in range(F):
        tab, bad = clib.cell_table(W, H, R, C, disp[f], stab[f])
        assert bad == 0
        _, _, mx, my = clib.warp_frame(np.ascontiguousarray(fr[f, ..., :3]), R, C, tab, want_maps=True)
        ix = np.floor(np.rint(mx.astype(np.float64) * 32) / 32).astype(np.int64)
        iy = np.floor(np.rint(my.astype(np.float64) * 32) / 32).astype(np.int64)
        unowned = (mx == np.float32(W + 1)) & (my == np.float32(H + 1))
        outside = (ix >= W) | (ix + 1 < 0) | (iy >= H) | (iy + 1 < 0)
        inside = (ix >= 0) & (ix <= W - 2) & (iy >= 0) & (iy <= H - 2)
        assert np.all(alpha[f][unowned | outside] == 0)
        assert np.all(alpha[f][inside] == 255)
        n_out += int((unowned | outside).sum())
        n_in += int(inside.sum())
    assert n_out > 0 and n_in > 0


def test_staging_paths_and_frame_splits(dev, monkeypatch):
    """A 16-byte aligned stack (staged 4-byte windows), a 4-byte aligned one and one at a 1-byte offset (per-tap / global taps), and
    MF_WARP_FRAMES_PER_LAUNCH splits: all equal the u8c3 + u8c1 reference."""
    from meshflow_amd import ops
    F, H, W, R, C = 7, 144, 256, 8, 8
    disp, _, stab = motion(F, H, W, R, C, seed=9, jitter=1.5)
    fr = bgra(F, H, W, seed=10)
    border = (5, 6, 7, 8)
    want, want_crop, _ = split_reference(dev, fr, disp, stab, R, C, border)
    table = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
    aligned = torch.from_numpy(fr).to(dev)
    assert aligned.data_ptr() % 16 == 0
    np.testing.assert_array_equal(ops.warp(aligned, table, border).cpu().numpy(), want)
    for off in (1, 4):
        raw = torch.zeros(fr.size + off, dtype=torch.uint8, device=dev)
        raw[off:] = aligned.reshape(-1)
        view = raw[off:].view(F, H, W, 4)
        assert view.data_ptr() % 4 == off % 4
        t = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
        np.testing.assert_array_equal(ops.warp(view, t, border).cpu().numpy(), want)
        np.testing.assert_array_equal(t.crop.cpu().numpy(), want_crop)
    for per in ('1', '3'):
        monkeypatch.setenv('MF_WARP_FRAMES_PER_LAUNCH', per)
        np.testing.assert_array_equal(ops.warp(aligned, table, border).cpu().numpy(), want)


def test_more_than_65535_frames_in_one_call(dev):
    """70,000 frames of 6 x 5 pixels: launch_warp cuts the clip into launches of at most 65,535 frames."""
    from meshflow_amd import ops, synthetic
    F, H, W, R, C = 70000, 5, 6, 1, 1
    disp, _ = synthetic.motion(F, R, C, seed=61, jitter_sigma=0.3)
    stab = disp * 0.5
    fr = bgra(F, H, W, seed=62)
    want, want_crop, want_bounds = split_reference(dev, fr, disp, stab, R, C, (1, 2, 3, 4))
    table = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
    out = ops.warp(torch.from_numpy(fr).to(dev), table, (1, 2, 3, 4))
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want)
    assert np.array_equal(table.crop.cpu().numpy(), want_crop)
    assert table.clip_bounds.cpu().numpy().tolist() == want_bounds.tolist()


def test_stack_over_4_gib(dev):
    """530 frames of 1080p BGRA (4.4 GB): 64-bit frame offsets in the warp and the crop-resize; the last frames equal separate calls."""
    from meshflow_amd import ops
    F, H, W, R, C = 530, 1080, 1920, 4, 4
    disp, _, stab = motion(F, H, W, R, C, seed=31, jitter=1.0)
    base = torch.from_numpy(bgra(4, H, W, seed=32)).to(dev)
    fr = base.repeat(F // 4 + 1, 1, 1, 1)[:F].contiguous()
    assert fr.numel() > 2 ** 32
    d_un, d_st = dev64(disp, dev), dev64(stab, dev)
    table = ops.cell_table(d_un, d_st, W, H, R, C)
    out = ops.warp(fr, table, (1, 2, 3, 4))
    tail, crop = out[-3:].cpu(), table.crop[-3:].cpu()
    rect = (31, 17, 1890, 1060)
    cropped_tail = ops.crop_resize(out, rect)[-3:].cpu()
    del out
    torch.cuda.empty_cache()
    t2 = ops.cell_table(d_un[-3:].contiguous(), d_st[-3:].contiguous(), W, H, R, C)
    want = ops.warp(fr[-3:].contiguous(), t2, (1, 2, 3, 4))
    want_cropped = ops.crop_resize(want, rect)
    torch.cuda.synchronize()
    assert torch.equal(tail, want.cpu()) and torch.equal(crop, t2.crop.cpu())
    assert torch.equal(cropped_tail, want_cropped.cpu())
    del fr
    torch.cuda.empty_cache()


@pytest.mark.parametrize('chunks', [0, 3])
def test_warp_clip_equals_warp(dev, chunks):
    from meshflow_amd import ops
    F, H, W, R, C = 37, 72, 100, 4, 4
    disp, _, stab = motion(F, H, W, R, C, seed=21, jitter=1.5)
    fr = torch.from_numpy(bgra(F, H, W, seed=22)).to(dev)
    d_un, d_st = dev64(disp, dev), dev64(stab, dev)
    table = ops.cell_table(d_un, d_st, W, H, R, C)
    want = ops.warp(fr, table, (3, 4, 5, 6))
    want_bounds = ops.crop_reduce(table.crop, W, H)
    torch.cuda.synchronize()
    want_crop = table.crop.clone()
    t2 = ops.CellTable(F, W, H, R, C, dev)
    prep = torch.cuda.Stream(dev)
    out, bounds = ops.warp_clip(fr, d_un, d_st, t2, (3, 4, 5, 6), chunks=chunks, prep_stream=prep if chunks else None)
    torch.cuda.synchronize()
    t2.check()
    assert torch.equal(out, want)
    assert torch.equal(t2.crop, want_crop) and torch.equal(bounds, want_bounds)


def test_degenerate_mesh_same_error_as_u8c3(dev):
    from meshflow_amd import ops
    F, H, W, R, C = 2, 64, 64, 2, 2
    disp = np.zeros((F, R + 1, C + 1, 2))
    stab = np.zeros_like(disp)
    stab[1, 0, 1] = [-32.0, 0.0]                                         # vertex (0, 1) onto vertex (0, 0): no homography
    fr = bgra(F, H, W, seed=1)
    errs = []
    for frames in (torch.from_numpy(np.ascontiguousarray(fr[..., :3])).to(dev), torch.from_numpy(fr).to(dev)):
        table = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
        ops.warp(frames, table)
        t2 = ops.CellTable(F, W, H, R, C, dev)
        ops.warp_clip(frames, dev64(disp, dev), dev64(stab, dev), t2, chunks=0)
        torch.cuda.synchronize()
        for t in (table, t2):
            with pytest.raises(ValueError) as e:
                t.check()
            errs.append(str(e.value))
    assert errs[0] == errs[2] and errs[1] == errs[3]


# ---- crop-resize --------------------------------------------------------------------------------------------------------------------

RECTS = [(0, 0, 255, 143), (10, 5, 240, 130), (100, 0, 100, 143), (0, 70, 255, 70), (3, 3, 4, 140), (0, 0, 0, 0),
         (200, 1, 255, 9), (17, 29, 131, 77), (1, 1, 254, 142)]


def _split_resize(d, rect, size=None):
    from meshflow_amd import ops
    c3 = ops.crop_resize(d[..., :3].contiguous(), rect, size=size)
    c1 = ops.crop_resize(d[..., 3].contiguous(), rect, size=size)
    return torch.cat([c3, c1[..., None]], dim=-1)


@pytest.mark.parametrize('H,W', [(144, 256), (75, 101), (1080, 1920), (9, 3), (2, 2)])
def test_crop_resize_same_size(dev, H, W):
    from meshflow_amd import ops
    from oracle import meshflow_oracle as mo
    fr = bgra(3, H, W, seed=H + W)
    d = torch.from_numpy(fr).to(dev)
    raw = torch.zeros(fr.size + 1, dtype=torch.uint8, device=dev)           # a stack at an odd byte offset: the direct form
    raw[1:] = d.reshape(-1)
    odd = raw[1:].view(3, H, W, 4)
    for k, (l, t, r, b) in enumerate(RECTS):
        r, b = min(r, W - 1), min(b, H - 1)
        l, t = min(l, r), min(t, b)
        got = ops.crop_resize(d, (l, t, r, b))
        want = _split_resize(d, (l, t, r, b))
        torch.cuda.synchronize()
        assert got.shape == (3, H, W, 4)
        assert torch.equal(got, want), (l, t, r, b)
        assert torch.equal(ops.crop_resize(odd, (l, t, r, b)), want), (l, t, r, b)
        if k < 3 and H * W < 10 ** 5:
            g = got.cpu().numpy()
            np.testing.assert_array_equal(g[..., :3], np.stack(mo.crop_frames(list(fr[..., :3]), (l, t, r, b))))
            a3 = np.repeat(fr[..., 3:], 3, axis=-1)
            np.testing.assert_array_equal(g[..., 3], np.stack(mo.crop_frames(list(a3), (l, t, r, b)))[..., 0])


SIZES = [  # H, W, rect, (oW, oH): up, down, exactly 2x down, non-uniform, beyond the staged down span
    (144, 256, (10, 5, 240, 130), (400, 300)),
    (144, 256, (0, 0, 255, 143), (85, 47)),
    (144, 256, (0, 0, 255, 143), (128, 72)),
    (144, 256, (16, 8, 215, 107), (100, 50)),
    (75, 101, (3, 2, 90, 70), (200, 20)),
    (75, 101, (3, 2, 90, 70), (31, 140)),
    (1080, 1920, (0, 0, 1919, 1079), (640, 360)),
    (2160, 3840, (40, 22, 3799, 2137), (1920, 1080)),
    (2160, 3840, (0, 0, 3839, 2159), (1920, 1080)),
    (9, 3, (0, 0, 2, 8), (5, 1)),
]


@pytest.mark.parametrize('H,W,rect,size', SIZES)
def test_crop_resize_to_size(dev, H, W, rect, size):
    from meshflow_amd import ops
    from oracle import meshflow_oracle as mo
    F = 2
    fr = bgra(F, H, W, seed=W + size[0])
    d = torch.from_numpy(fr).to(dev)
    got = ops.crop_resize(d, rect, size=size)
    want = _split_resize(d, rect, size=size)
    torch.cuda.synchronize()
    assert got.shape == (F, size[1], size[0], 4)
    assert torch.equal(got, want)
    raw = torch.zeros(fr.size + 1, dtype=torch.uint8, device=dev)
    raw[1:] = d.reshape(-1)
    assert torch.equal(ops.crop_resize(raw[1:].view(F, H, W, 4), rect, size=size), want)
    out = torch.empty_like(got)
    assert ops.crop_resize(d, rect, size=size, out=out) is out and torch.equal(out, want)
    if H * W <= 144 * 256:
        l, t, r, b = rect
        g = got.cpu().numpy()
        for f in range(F):
            np.testing.assert_array_equal(g[f, ..., :3], mo.resize_linear_u8(fr[f, t:b + 1, l:r + 1, :3], *size))
            a3 = np.repeat(fr[f, t:b + 1, l:r + 1, 3:], 3, axis=-1)
            np.testing.assert_array_equal(g[f, ..., 3], mo.resize_linear_u8(a3, *size)[..., 0])
    if size == (W, H):
        assert torch.equal(got, ops.crop_resize(d, rect))


# ---- stabilize_resident -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('check', [True, 'deferred', 'never'])
@pytest.mark.parametrize('chunks', [0, 3])
def test_stabilize_resident(dev, check, chunks):
    from meshflow_amd import synthetic
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    F, H, W, R, C = 8, 72, 96, 4, 4
    disp, hom = synthetic.motion(F, R, C, seed=31, jitter_sigma=1.0)
    fr = bgra(F, H, W, seed=32)
    res = {}
    for name, frames in (('c3', fr[..., :3]), ('c1', fr[..., 3]), ('c4', fr)):
        s = MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, temporal_smoothing_radius=3, optimization_num_iterations=10,
                               device='cuda:0')
        s.resident_chunks = chunks
        d = torch.from_numpy(np.ascontiguousarray(frames)).to(dev)
        d_disp = dev64(disp, dev)
        full = s.stabilize_resident(d, d_disp, hom, check=check)
        lo, hi = 2, 5
        shard = s.stabilize_resident(d[lo:hi].contiguous(), d_disp, hom, check=check, frame_range=(lo, hi), collective=True)
        empty = s.stabilize_resident(d[:0], d_disp, hom, check=check, frame_range=(4, 4))
        s.finish()
        torch.cuda.synchronize()
        res[name] = (full, shard, empty)
    (o3, b3, s3), (sh3, sb3, ss3), (_, eb3, _) = res['c3']
    (o1, b1, s1), (sh1, sb1, _), _ = res['c1']
    (o4, b4, s4), (sh4, sb4, ss4), (e4, eb4, _) = res['c4']
    # the stabilizer's 3-component border (0, 0, 255): alpha border 0, the u8c1 call's border byte is 0 as well
    assert torch.equal(b3, b4) and torch.equal(b1, b4) and torch.equal(s3, s4) and torch.equal(sb3, sb4) and torch.equal(ss3, ss4)
    assert torch.equal(eb3, eb4) and torch.equal(sb1, sb4)
    assert o4.shape == (F, H, W, 4) and e4.shape == (0, H, W, 4)
    assert torch.equal(o4[..., :3], o3) and torch.equal(o4[..., 3], o1)
    assert torch.equal(sh4[..., :3], sh3) and torch.equal(sh4[..., 3], sh1)
    assert torch.equal(sh4, o4[2:5])
