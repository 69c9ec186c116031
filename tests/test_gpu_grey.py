"""-m gpu: single-channel uint8 frames -- mf_warp_u8c1 / mf_warp_bounds_u8c1 / mf_warp_clip_u8c1 / mf_crop_resize_u8c1, the u8c1 host
pipeline, `ops`, the drop-in methods and `stabilize_resident` on (H, W) / (n, H, W) frames.

cv2.remap's and cv2.resize's 8-bit paths work per channel, so the contract is: the grey result of `g` with border b is byte for byte
channel 0 of the u8c3 result of stack(g, g, g) with border (b, b, b) -- and channel c of every reference golden -- with the same
per-frame crop values and clip rectangle."""
import ctypes
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GOLDENS = sorted(f for f in os.listdir(GOLDEN) if f.startswith('warp_') and f.endswith('.npz'))


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


def grey(F, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (F, H, W), dtype=np.uint8)


def rgb(g):
    return np.ascontiguousarray(np.repeat(g[..., None], 3, axis=-1))


def colour_reference(dev, fr, disp, stab, R, C, b):
    """The u8c3 warp of the replicated frames with border (b, b, b): (channel 0, per-frame crop, rectangle)."""
    from meshflow_amd import ops
    F, H, W = fr.shape
    table = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
    out = ops.warp(torch.from_numpy(rgb(fr)).to(dev), table, (b, b, b))
    torch.cuda.synchronize()
    table.check()
    return out[..., 0].cpu().numpy(), table.crop.cpu().numpy().copy(), table.clip_bounds.cpu().numpy().copy()


# ---- the reference goldens, per channel ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', GOLDENS)
def test_goldens_per_channel_through_ops(dev, name):
    from meshflow_amd import ops
    g = np.load(os.path.join(GOLDEN, name))
    W, H, R, C = int(g['width']), int(g['height']), int(g['R']), int(g['C'])
    for c in range(3):
        fr = torch.from_numpy(np.ascontiguousarray(g['frames'][..., c])).to(dev)
        table = ops.cell_table(dev64(g['unstab'], dev), dev64(g['stab'], dev), W, H, R, C)
        out = ops.warp(fr, table, (int(g['border'][c]), 7, 9))
        torch.cuda.synchronize()
        table.check()
        assert out.shape == fr.shape and out.dtype == torch.uint8
        np.testing.assert_array_equal(out.cpu().numpy(), g['out'][..., c])
        assert table.clip_bounds.cpu().numpy().tolist() == g['bounds'].tolist()


@pytest.mark.parametrize('name', GOLDENS)
def test_goldens_per_channel_through_ctypes(dev, name):
    from meshflow_amd import _lib, ops
    lib = _lib.lib
    g = np.load(os.path.join(GOLDEN, name))
    W, H, R, C, F = int(g['width']), int(g['height']), int(g['R']), int(g['C']), int(g['F'])
    for c in range(3):
        fr = torch.from_numpy(np.ascontiguousarray(g['frames'][..., c])).to(dev)
        out = torch.empty_like(fr)
        table = ops.cell_table(dev64(g['unstab'], dev), dev64(g['stab'], dev), W, H, R, C)
        bounds = torch.empty(4, dtype=torch.int32, device=dev)
        d_un, d_st = dev64(g['unstab'], dev), dev64(g['stab'], dev)
        for chunks in (0, 2):
            _lib.check(lib.mf_warp_clip_u8c1(fr.data_ptr(), out.data_ptr(), d_un.data_ptr(), d_st.data_ptr(), F, W, H, R, C, int(g['border'][c]), table.buf.data_ptr(),
                                             table.crop.data_ptr(), bounds.data_ptr(), table.status.data_ptr(), chunks, None, None))
            torch.cuda.synchronize()
            np.testing.assert_array_equal(out.cpu().numpy(), g['out'][..., c])
            assert bounds.cpu().numpy().tolist() == g['bounds'].tolist()


# ---- seeded clips against the u8c3 kernels' channel 0 -----------------------------------------------------------------------------

GEOMS = [  # F, H, W, R, C, jitter, kind
    (3, 131, 257, 5, 7, 1.0, 'jitter'),        # W % 4 != 0: no staged windows
    (2, 2, 2, 1, 1, 0.3, 'jitter'),
    (3, 2, 9, 1, 2, 0.3, 'jitter'),
    (3, 9, 2, 2, 1, 0.3, 'jitter'),
    (3, 75, 101, 6, 4, 2.0, 'shift'),
    (2, 96, 128, 32, 32, 0.5, 'jitter'),
    (2, 130, 140, 64, 64, 0.3, 'jitter'),
    (4, 72, 100, 3, 5, 6.0, 'jitter'),          # strong jitter: border taps and uncovered pixels
    (4, 144, 256, 16, 16, 1.5, 'shift'),
    (3, 1080, 1920, 16, 16, 1.5, 'jitter'),
    (2, 1080, 1920, 32, 32, 1.0, 'shift'),
]


@pytest.mark.parametrize('F,H,W,R,C,jitter,kind', GEOMS)
def test_warp_equals_colour_channel0(dev, F, H, W, R, C, jitter, kind):
    from meshflow_amd import ops
    disp, _, stab = motion(F, H, W, R, C, seed=W + F, jitter=jitter, kind=kind)
    fr = grey(F, H, W, seed=H)
    b = 77
    want, want_crop, want_bounds = colour_reference(dev, fr, disp, stab, R, C, b)
    table = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
    out = ops.warp(torch.from_numpy(fr).to(dev), table, (b, 1, 2))
    torch.cuda.synchronize()
    table.check()
    got = out.cpu().numpy()
    assert got.shape == (F, H, W)
    assert np.array_equal(got, want), int((got != want).sum())
    assert np.array_equal(table.crop.cpu().numpy(), want_crop)
    assert table.clip_bounds.cpu().numpy().tolist() == want_bounds.tolist()


def test_small_clip_against_the_oracle(dev):
    from meshflow_amd import ops
    from oracle import clib
    F, H, W, R, C = 4, 64, 96, 4, 4
    disp, _, stab = motion(F, H, W, R, C, seed=5, jitter=2.0)
    fr = grey(F, H, W, seed=6)
    want, crop, bad = clib.warp_clip(rgb(fr), R, C, disp, stab, (0, 0, 0))
    assert bad == 0
    table = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
    out = ops.warp(torch.from_numpy(fr).to(dev), table)            # default border (0, 0, 255): byte 0
    torch.cuda.synchronize()
    np.testing.assert_array_equal(out.cpu().numpy(), want[..., 0])
    np.testing.assert_array_equal(table.crop.cpu().numpy(), crop)


def test_unaligned_stack_and_frame_splits(dev, monkeypatch):
    """A stack at an odd byte offset (no staged windows), and MF_WARP_FRAMES_PER_LAUNCH splits, equal the aligned single launch."""
    from meshflow_amd import ops
    F, H, W, R, C = 7, 144, 256, 8, 8
    disp, _, stab = motion(F, H, W, R, C, seed=9, jitter=1.5)
    fr = grey(F, H, W, seed=10)
    table = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
    want = ops.warp(torch.from_numpy(fr).to(dev), table, (5,)).cpu().numpy()
    raw = torch.zeros(F * H * W + 1, dtype=torch.uint8, device=dev)
    raw[1:] = torch.from_numpy(fr.reshape(-1)).to(dev)
    odd = raw[1:].view(F, H, W)
    assert odd.data_ptr() % 4 == 1
    np.testing.assert_array_equal(ops.warp(odd, table, (5,)).cpu().numpy(), want)
    for per in ('1', '3'):
        monkeypatch.setenv('MF_WARP_FRAMES_PER_LAUNCH', per)
        np.testing.assert_array_equal(ops.warp(torch.from_numpy(fr).to(dev), table, (5,)).cpu().numpy(), want)


@pytest.mark.parametrize('chunks', [0, 1, 4, 32])
def test_warp_clip_equals_warp(dev, chunks):
    from meshflow_amd import ops
    F, H, W, R, C = 37, 72, 100, 4, 4
    disp, _, stab = motion(F, H, W, R, C, seed=21, jitter=1.5)
    fr = torch.from_numpy(grey(F, H, W, seed=22)).to(dev)
    d_un, d_st = dev64(disp, dev), dev64(stab, dev)
    table = ops.cell_table(d_un, d_st, W, H, R, C)
    want = ops.warp(fr, table, (3,))
    want_bounds = ops.crop_reduce(table.crop, W, H)
    t2 = ops.cell_table(d_un, d_st, W, H, R, C)
    prep = torch.cuda.Stream(dev)
    out, bounds = ops.warp_clip(fr, d_un, d_st, t2, (3,), chunks=chunks, prep_stream=prep if chunks else None)
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    assert bounds.tolist() == want_bounds.tolist()


def test_resident_stack_over_4_gib(dev):
    """2,100 frames of 1080p grey (4.35 GB): 64-bit frame offsets; the last frames equal a separate call on them."""
    from meshflow_amd import ops
    F, H, W, R, C = 2100, 1080, 1920, 4, 4
    disp, _, stab = motion(F, H, W, R, C, seed=31, jitter=1.0)
    base = torch.from_numpy(grey(4, H, W, seed=32)).to(dev)
    fr = base.repeat(F // 4 + 1, 1, 1)[:F].contiguous()
    d_un, d_st = dev64(disp, dev), dev64(stab, dev)
    table = ops.cell_table(d_un, d_st, W, H, R, C)
    out = ops.warp(fr, table, (9,))
    tail = out[-3:].cpu()
    crop = table.crop[-3:].cpu()
    del out
    t2 = ops.cell_table(d_un[-3:].contiguous(), d_st[-3:].contiguous(), W, H, R, C)
    want = ops.warp(fr[-3:].contiguous(), t2, (9,))
    torch.cuda.synchronize()
    assert torch.equal(tail, want.cpu())
    assert torch.equal(crop, t2.crop.cpu())


# ---- crop-resize --------------------------------------------------------------------------------------------------------------------

RECTS = [(0, 0, 255, 143), (10, 5, 240, 130), (100, 0, 100, 143), (0, 70, 255, 70), (3, 3, 4, 140), (0, 0, 0, 0),
         (200, 1, 255, 9), (17, 29, 131, 77), (1, 1, 254, 142)]


@pytest.mark.parametrize('H,W', [(144, 256), (75, 101), (1080, 1920), (9, 3)])
def test_crop_resize_equals_colour_channel0(dev, H, W):
    from meshflow_amd import ops
    fr = grey(3, H, W, seed=H + W)
    d = torch.from_numpy(fr).to(dev)
    d3 = torch.from_numpy(rgb(fr)).to(dev)
    for l, t, r, b in RECTS:
        r, b = min(r, W - 1), min(b, H - 1)
        l, t = min(l, r), min(t, b)
        got = ops.crop_resize(d, (l, t, r, b))
        want = ops.crop_resize(d3, (l, t, r, b))[..., 0]
        torch.cuda.synchronize()
        assert got.shape == (3, H, W)
        assert torch.equal(got, want), (l, t, r, b)
    raw = torch.zeros(3 * H * W + 3, dtype=torch.uint8, device=dev)          # a stack at an odd byte offset
    raw[3:] = d.reshape(-1)
    assert torch.equal(ops.crop_resize(raw[3:].view(3, H, W), (0, 0, W // 2, H // 2)),
                       ops.crop_resize(d3, (0, 0, W // 2, H // 2))[..., 0])


# ---- host paths -------------------------------------------------------------------------------------------------------------------

def stabilizer(R, C, dev='cuda:0'):
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    return MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, temporal_smoothing_radius=3, optimization_num_iterations=10, device=dev)


@pytest.fixture(scope='module')
def host_case(dev):
    from meshflow_amd import ops
    F, H, W, R, C = 17, 144, 256, 4, 4
    disp, hom, _ = motion(F, H, W, R, C, seed=41, jitter=2.0)
    fr = grey(F, H, W, seed=42)
    s = stabilizer(R, C)
    stab = s._get_stabilized_vertex_displacements(F, list(fr), 0, disp, hom)
    b = 0                                          # color_outside_image_area_bgr = (0, 0, 255): byte 0
    table = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
    out = ops.warp(torch.from_numpy(fr).to(dev), table)
    bounds = tuple(int(v) for v in ops.crop_reduce(table.crop, W, H).tolist())
    cropped = ops.crop_resize(out, bounds)
    torch.cuda.synchronize()
    col = s.stabilize_clip(list(rgb(fr)), disp, hom, crop=True)
    return dict(F=F, H=H, W=W, R=R, C=C, disp=disp, hom=hom, fr=fr, stab=stab, s=s, out=out.cpu().numpy(), bounds=bounds,
                cropped=cropped.cpu().numpy(), col=col, b=b)


def _check_clip_result(case, res, crop):
    out, bounds, stab = res[0], res[1], res[2]
    assert tuple(int(v) for v in bounds) == case['bounds'] == tuple(int(v) for v in case['col'][1])
    np.testing.assert_array_equal(stab, case['stab'])
    if out is not None:
        assert len(out) == case['F'] and out[0].shape == (case['H'], case['W'])
        np.testing.assert_array_equal(np.stack(out), case['out'])
        np.testing.assert_array_equal(np.stack(out), np.stack(case['col'][0])[..., 0])
    if crop:
        assert res[4][0].shape == (case['H'], case['W'])
        np.testing.assert_array_equal(np.stack(res[4]), case['cropped'])
        np.testing.assert_array_equal(np.stack(res[4]), np.stack(case['col'][4])[..., 0])


def _inputs(fr):
    F, H, W = fr.shape
    buf = np.zeros(F * H * W + 3, np.uint8)
    buf[3:] = fr.reshape(-1)
    odd = buf[3:].reshape(F, H, W)
    wide = np.ascontiguousarray(np.stack([fr, 255 - fr], axis=-1))
    ro = [np.frombuffer(f.tobytes(), np.uint8).reshape(H, W) for f in fr]
    return {'list': list(fr), 'array': fr, 'odd_views': list(odd), 'odd_array': odd, 'channel_slices': [f[..., 0] for f in wide],
            'read_only': ro}


@pytest.mark.parametrize('chunk', [None, '1', '5'])
def test_host_paths_equal_resident_and_colour(dev, host_case, monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv('MF_PIPE_CHUNK', chunk)
    s, case = host_case['s'], host_case
    for name, frames in _inputs(case['fr']).items():
        for crop, keep in ((False, True), (True, True), (True, False)):
            res = s.stabilize_clip(frames, case['disp'], case['hom'], crop=crop, keep_uncropped=keep)
            _check_clip_result(case, res, crop)
            if crop and not keep:
                assert res[0] is None
        out, bounds = s._get_stabilized_frames_and_crop_boundaries(case['F'], frames, case['disp'], case['stab'])
        assert isinstance(out, list) and out[0].shape == (case['H'], case['W']), name
        np.testing.assert_array_equal(np.stack(out), case['out'])
        assert tuple(int(v) for v in bounds) == case['bounds']
        cropped = s._crop_frames(frames, case['bounds'])
        assert isinstance(cropped, list) and cropped[0].shape == (case['H'], case['W'])
        from meshflow_amd import ops
        want = ops.crop_resize(torch.from_numpy(np.ascontiguousarray(np.stack(frames))).to(dev), case['bounds']).cpu().numpy()
        np.testing.assert_array_equal(np.stack(cropped), want)


def test_host_one_frame_object_repeated(dev, host_case):
    case = host_case
    f0 = case['fr'][0]
    res = case['s'].stabilize_clip([f0] * case['F'], case['disp'], case['hom'], crop=True)
    from meshflow_amd import ops
    table = ops.cell_table(dev64(case['disp'], dev), dev64(res[2], dev), case['W'], case['H'], case['R'], case['C'])
    want = ops.warp(torch.from_numpy(np.stack([f0] * case['F'])).to(dev), table).cpu().numpy()
    np.testing.assert_array_equal(np.stack(res[0]), want)


def test_host_clip_larger_than_the_ring(dev):
    """200 frames of 4K grey (1.66 GB, more than the 720 MB ring per direction): equal to the resident result."""
    from meshflow_amd import ops
    F, H, W, R, C = 200, 2160, 3840, 8, 8
    disp, hom, _ = motion(F, H, W, R, C, seed=51, jitter=1.0)
    base = grey(2, H, W, seed=52)
    fr = np.ascontiguousarray(np.concatenate([base] * (F // 2)))
    s = stabilizer(R, C)
    out, bounds, stab, _, cropped = s.stabilize_clip(fr, disp, hom, crop=True)
    d_fr = torch.from_numpy(fr).to(dev)
    table = ops.cell_table(dev64(disp, dev), dev64(stab, dev), W, H, R, C)
    want = ops.warp(d_fr, table)
    del d_fr
    want_bounds = tuple(int(v) for v in ops.crop_reduce(table.crop, W, H).tolist())
    assert tuple(int(v) for v in bounds) == want_bounds
    for i in (0, 1, 99, 198, 199):
        np.testing.assert_array_equal(out[i], want[i].cpu().numpy())
    want_c = ops.crop_resize(want[-4:].contiguous(), want_bounds).cpu().numpy()
    np.testing.assert_array_equal(np.stack(cropped[-4:]), want_c)


def test_methods_borrowed_by_a_foreign_class(dev):
    """INTEGRATION.md section 1 with grey frames: a class that only has the reference's attributes borrows the drop-in pair."""
    import meshflow_amd as amd
    from oracle import clib

    class RefLike:
        def __init__(self):
            self.mesh_row_count = self.mesh_col_count = 4
            self.temporal_smoothing_radius, self.optimization_num_iterations = 3, 8
            self.color_outside_image_area_bgr = (0, 0, 255)

    class Stabilizer(RefLike):
        _get_stabilized_vertex_displacements = amd.MeshFlowStabilizer._get_stabilized_vertex_displacements
        _get_stabilized_frames_and_crop_boundaries = amd.MeshFlowStabilizer._get_stabilized_frames_and_crop_boundaries
        _check_mesh_shape = amd.MeshFlowStabilizer._check_mesh_shape
        _torch_device = amd.MeshFlowStabilizer._torch_device
        _jacobi_coefficients_device = amd.MeshFlowStabilizer._jacobi_coefficients_device
        _stabilized_vertex_displacements_device = amd.MeshFlowStabilizer._stabilized_vertex_displacements_device
        _crop_frames = amd.MeshFlowStabilizer._crop_frames
        device = None

    F, H, W = 10, 64, 96
    disp, hom, _ = motion(F, H, W, 4, 4, seed=6, jitter=1.0)
    fr = grey(F, H, W, seed=7)
    s = Stabilizer()
    stab = s._get_stabilized_vertex_displacements(F, list(fr), 0, disp, hom)
    out, bounds = s._get_stabilized_frames_and_crop_boundaries(F, list(fr), disp, stab)
    want, crop, _ = clib.warp_clip(rgb(fr), 4, 4, disp, stab, (0, 0, 0))
    assert out[0].shape == (H, W)
    np.testing.assert_array_equal(np.stack(out), want[..., 0])
    assert tuple(int(v) for v in bounds) == (crop[:, 0].max(), crop[:, 1].max(), crop[:, 2].min(), crop[:, 3].min())
    cropped = s._crop_frames(out, bounds)
    assert len(cropped) == F and cropped[0].shape == (H, W)


# ---- refusals and bad arguments -----------------------------------------------------------------------------------------------------

def test_refusals_keep_their_errors(dev):
    from meshflow_amd import ops
    F, H, W, R, C = 6, 48, 64, 2, 2
    disp, hom, _ = motion(F, H, W, R, C, seed=3, jitter=0.5)
    s = stabilizer(R, C)
    g = list(grey(F, H, W, seed=4))
    colour = list(rgb(grey(F, H, W, seed=4)))
    for bad in ([f[..., None] for f in g], np.stack(g)[..., None], colour[:3] + [g[3]] + colour[4:], g[:3] + [colour[3]] + g[4:],
                [np.zeros((H, W, 4), np.uint8)] * F, g[:3] + [np.zeros((H, W + 1), np.uint8)] + g[4:]):
        with pytest.raises(ValueError):
            s.stabilize_clip(bad, disp, hom)
    for bad in ([f.astype(np.uint16) for f in g], [f.astype(np.float32) for f in g], np.stack(g).astype(np.uint16)):
        with pytest.raises(TypeError):
            s.stabilize_clip(bad, disp, hom)
        with pytest.raises(TypeError):
            s._crop_frames(bad, (0, 0, W - 1, H - 1))
    d16 = torch.zeros((F, H, W), dtype=torch.uint16, device=dev)
    table = ops.cell_table(dev64(disp, dev), dev64(disp, dev), W, H, R, C)
    for fn in (lambda: ops.warp(d16, table), lambda: ops.crop_resize(d16, (0, 0, W - 1, H - 1)),
               lambda: s.stabilize_resident(d16, dev64(disp, dev), hom)):
        with pytest.raises(ValueError, match='uint16'):
            fn()
    with pytest.raises(ValueError):
        ops.warp(torch.zeros((F, H, W, 1), dtype=torch.uint8, device=dev), table)


def test_abi_bad_arguments(dev):
    from meshflow_amd import _lib, ops
    lib = _lib.lib
    F, H, W, R, C = 2, 64, 64, 2, 2
    disp = np.zeros((F, R + 1, C + 1, 2))
    d_un = dev64(disp, dev)
    table = ops.cell_table(d_un, d_un, W, H, R, C)
    fr = torch.zeros((F, H, W), dtype=torch.uint8, device=dev)
    out = torch.full((F, H, W), 0xA5, dtype=torch.uint8, device=dev)
    bounds = torch.empty(4, dtype=torch.int32, device=dev)
    work = torch.empty(lib.mf_crop_resize_workspace_bytes(W, H), dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()              # noqa: E731
    t, cr, st = table.buf, table.crop, table.status
    calls = [
        lambda: lib.mf_warp_u8c1(None, p(out), p(t), F, W, H, R, C, 0, p(cr), None),
        lambda: lib.mf_warp_u8c1(p(fr), p(fr), p(t), F, W, H, R, C, 0, p(cr), None),
        lambda: lib.mf_warp_u8c1(p(fr), p(out), p(t), 0, W, H, R, C, 0, p(cr), None),
        lambda: lib.mf_warp_u8c1(p(fr), p(out), p(t), F, 1, H, R, C, 0, p(cr), None),
        lambda: lib.mf_warp_u8c1(p(fr), p(out), p(t), F, W, 40000, R, C, 0, p(cr), None),
        lambda: lib.mf_warp_u8c1(p(fr), p(out), p(t), F, W, H, 65, C, 0, p(cr), None),
        lambda: lib.mf_warp_bounds_u8c1(p(fr), p(out), p(t), F, W, H, R, C, 0, p(cr), None, None),
        lambda: lib.mf_warp_clip_u8c1(p(fr), p(out), p(d_un), None, F, W, H, R, C, 0, p(t), p(cr), p(bounds), p(st), 0, None, None),
        lambda: lib.mf_warp_clip_u8c1(p(fr), p(out), p(d_un), p(d_un), F, W, H, R, 65, 0, p(t), p(cr), p(bounds), p(st), 0, None, None),
        lambda: lib.mf_warp_clip_u8c1(p(fr), p(out), p(d_un), p(d_un), F, 1, H, R, C, 0, p(t), p(cr), p(bounds), p(st), 2, None, None),
        lambda: lib.mf_crop_resize_u8c1(p(fr), p(out), F, W, H, 0, 0, W, H - 1, p(work), None),
        lambda: lib.mf_crop_resize_u8c1(p(fr), p(out), F, W, H, 5, 0, 4, H - 1, p(work), None),
        lambda: lib.mf_crop_resize_u8c1(p(fr), None, F, W, H, 0, 0, 1, 1, p(work), None),
        lambda: lib.mf_crop_resize_u8c1(p(fr), p(out), 0, W, H, 0, 0, 1, 1, p(work), None),
        lambda: lib.mf_warp_u8c1_host_frames(None, None, None, None, F, W, H, R, C, 0, None, None),
        lambda: lib.mf_warp_crop_u8c1_host_frames(None, None, None, None, None, F, W, H, R, C, 0, None, None, None),
        lambda: lib.mf_crop_resize_u8c1_host_frames(None, None, F, W, H, 0, 0, 1, 1, None),
    ]
    for i, call in enumerate(calls):
        assert call() == _lib.MF_ERR_INVALID_ARG, i
        assert lib.mf_last_error(), i
    hf = [np.zeros((H, W), np.uint8) for _ in range(F)]
    ho = [np.zeros((H, W), np.uint8) for _ in range(F)]
    pin = (ctypes.c_void_p * F)(*[f.ctypes.data for f in hf])
    pout = (ctypes.c_void_p * F)(*[f.ctypes.data for f in ho])
    assert lib.mf_crop_resize_u8c1_host_frames(pin, pout, F, W, H, 3, 0, 2, H - 1, None) == _lib.MF_ERR_INVALID_ARG
    assert lib.mf_crop_resize_u8c1_host_frames(pin, pin, F, W, H, 0, 0, W - 1, H - 1, None) == _lib.MF_ERR_INVALID_ARG
    torch.cuda.synchronize()
    assert (out == 0xA5).all().item()                  # nothing was written
    assert torch.equal(ops.warp(fr, table), torch.zeros_like(fr))    # the device still answers


def test_degenerate_mesh_leaves_outputs_untouched(dev):
    from meshflow_amd import _lib
    F, H, W, R, C = 2, 64, 64, 2, 2
    disp = np.zeros((F, R + 1, C + 1, 2))
    stab = np.zeros_like(disp)
    stab[1, 0, 1] = [-32.0, 0.0]                                         # vertex (0, 1) onto vertex (0, 0): no homography
    s = stabilizer(R, C)
    fr = grey(F, H, W, seed=1)
    with pytest.raises(ValueError, match='degenerate'):
        s._get_stabilized_frames_and_crop_boundaries(F, list(fr), disp, stab)
    lib = _lib.lib
    out = [np.full((H, W), 0xA5, np.uint8) for _ in range(F)]
    crp = [np.full((H, W), 0x5A, np.uint8) for _ in range(F)]
    pin = (ctypes.c_void_p * F)(*[f.ctypes.data for f in fr])
    pout = (ctypes.c_void_p * F)(*[f.ctypes.data for f in out])
    pcrop = (ctypes.c_void_p * F)(*[f.ctypes.data for f in crp])
    crop = np.zeros((F, 4), np.int32)
    rect = (ctypes.c_int32 * 4)()
    rc = lib.mf_warp_crop_u8c1_host_frames(pin, pout, pcrop, disp.ctypes.data, stab.ctypes.data, F, W, H, R, C, 0, crop.ctypes.data, rect, None)
    assert rc == _lib.MF_ERR_DEGENERATE
    assert all((o == 0xA5).all() for o in out) and all((c == 0x5A).all() for c in crp)


# ---- stabilize_resident -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('check', [True, 'deferred', 'never'])
@pytest.mark.parametrize('chunks', [0, 3])
def test_stabilize_resident(dev, check, chunks):
    from meshflow_amd import ops
    F, H, W, R, C = 24, 96, 128, 4, 4
    disp, hom, _ = motion(F, H, W, R, C, seed=61, jitter=1.5)
    fr = grey(F, H, W, seed=62)
    s = stabilizer(R, C)
    s.resident_chunks = chunks
    d_fr, d_disp = torch.from_numpy(fr).to(dev), dev64(disp, dev)
    out, bounds, d_stab = s.stabilize_resident(d_fr, d_disp, hom, check=check)
    s.finish()
    torch.cuda.synchronize()
    assert out.shape == (F, H, W) and out.dtype == torch.uint8
    c_out, c_bounds, _ = s.stabilize_resident(torch.from_numpy(rgb(fr)).to(dev), d_disp, hom, check=check)
    s.finish()
    torch.cuda.synchronize()
    assert torch.equal(out, c_out[..., 0]) and bounds.tolist() == c_bounds.tolist()
    table = ops.cell_table(d_disp, d_stab, W, H, R, C)
    assert torch.equal(out, ops.warp(d_fr, table))
    # a frame-range shard equals the unsharded slice
    lo, hi = 7, 19
    sh_out, sh_bounds, _ = s.stabilize_resident(d_fr[lo:hi].contiguous(), d_disp, hom, frame_range=(lo, hi), check=check)
    s.finish()
    torch.cuda.synchronize()
    assert torch.equal(sh_out, out[lo:hi])
    want = table.crop[lo:hi].cpu().numpy()
    assert sh_bounds.tolist() == [int(want[:, 0].max()), int(want[:, 1].max()), int(want[:, 2].min()), int(want[:, 3].min())]
