"""-m gpu: a THIRD-PARTY second opinion on the restated OpenCV calls, with what the GPU box has: torch.

No OpenCV exists in the build image or on the GPU box, so the five cv2 calls on the path (findHomography, warpPerspective,
perspectiveTransform, remap: mfs.py:1041-1069; resize: mfs.py:1150) are restated from OpenCV's published algorithms and the
NumPy oracle, the C oracle and the HIP kernels all share that reading ("parity unpinned").  These tests
compare the HIP path with implementations that share NOTHING with it:

  * the warp with `torch.nn.functional.grid_sample(mode='bilinear', padding_mode='zeros', align_corners=True)` fed a coordinate
    map computed here in float64 -- pixel centres at integers, the map read as "output pixel -> source position", taps outside
    the frame replaced by the (black) border colour;
  * `_crop_frames` with `torch.nn.functional.interpolate(mode='bilinear', align_corners=False, antialias=False)` on the crop --
    half-pixel centres.

cv2.remap quantises coordinates to 1/32 pixel and cv2.resize its weights to 11 bits, so the comparison allows 1 LSB (north_star's
own bar) around the envelope of the float64 result over a 1/32-pixel neighbourhood; identity and integer shifts must be exact.
It pins nothing (parity stays "partial": tests/test_cv2_crosscheck.py is the door to "green"), but a wrong reading of pixel
centres, map direction, mesh-motion sign or border handling cannot pass it.

The helpers live in tests/second_opinion.py.  The tests of the second half judge all four formats and crop_resize(size=...) with that
module's judge and constants, which were fixed on the CPU against the models (tests/test_second_opinion_models.py); none is defined here.
The last part does the same for the NV12 and P010 calls, chroma included, and registers chroma on luma with a ramp."""
import numpy as np
import pytest

import second_opinion as so

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')
F_ = torch.nn.functional


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def _grid(W, H, R, C):
    return so.grid(W, H, R, C)


def _smooth_frames(dev, n, H, W, seed=0):
    """Band-limited frames (sums of sinusoids, gradients of a few grey levels per pixel): uint8 (n, H, W, 3) on the device."""
    return so.smooth_planes('u8c3', n, H, W, seed, dev).to(torch.uint8)


def _sample(frames, u, v):
    """grid_sample of uint8 frames (n, H, W, 3) at float64 source positions u, v (n, H, W) in PIXEL units -> float64 (n, H, W, 3)."""
    return so.sample(frames.to(torch.float64), u, v)


_assert_within_envelope = so.legacy_assert_within_envelope


def _hip_warp(dev, d_frames, R, C, unstab, stab, border=(0, 0, 0)):
    from meshflow_amd import ops
    n, H, W = d_frames.shape[:3]
    table = ops.cell_table(torch.from_numpy(np.ascontiguousarray(unstab)).to(dev), torch.from_numpy(np.ascontiguousarray(stab)).to(dev), W, H, R, C)
    out = ops.warp(d_frames, table, border)
    torch.cuda.synchronize()
    table.check()
    return out, table.crop.cpu().numpy()


def _pixels(dev, n, H, W):
    return so.pixels(n, H, W, dev)


@pytest.mark.parametrize('H,W,R,C', [(360, 640, 16, 16), (270, 484, 5, 7), (1080, 1920, 16, 16)])
def test_identity_and_integer_shifts_are_exact(dev, H, W, R, C):
    """No motion: the frame itself.  Stabilized = unstabilized + (dx, dy): the content moves by exactly (+dx, +dy) (content at grid
    vertex v moves to v + (P - C), mfs.py:964-967), the uncovered band is the border colour -- grid_sample with the map
    (x - dx, y - dy) says the same, byte for byte."""
    n = 2
    frames = _smooth_frames(dev, n, H, W)
    z = np.zeros((n, R + 1, C + 1, 2))
    out, crop = _hip_warp(dev, frames, R, C, z, z)
    assert torch.equal(out, frames)
    xs, ys = _pixels(dev, n, H, W)
    for dx, dy in ((5, -3), (-4, 6)):
        s = z.copy(); s[..., 0] = dx; s[..., 1] = dy
        out, crop = _hip_warp(dev, frames, R, C, z, s)
        want = _sample(frames, xs - dx, ys - dy)                         # integer positions: weights 0 / 1
        # one ring of pixels next to the uncovered band: cv2.warpPerspective's bilinear mask reaches one pixel beyond the mesh
        # (those pixels sample column -1 / W: black either way) -- equal as well
        # (grid_sample goes through normalised coordinates: an integer position comes back as integer +- 1e-13, the weights as
        # 1 - 1e-13 and 1e-13 -- "exact" is |difference| < 1e-6 grey levels on every byte)
        assert float((out.to(torch.float64) - want).abs().max()) < 1e-6
        assert crop.tolist() == [[max(dx, 0), max(dy, 0), W - 1 + min(dx, 0), H - 1 + min(dy, 0)]] * n


@pytest.mark.parametrize('H,W,R,C,seed', [(360, 640, 16, 16, 1), (270, 484, 5, 7, 2), (1080, 1920, 16, 16, 3), (1080, 1920, 32, 32, 4)])
def test_global_homography_vs_grid_sample(dev, H, W, R, C, seed):
    """Every vertex moved by ONE global homography G (rotation, shear, perspective, sub-pixel shift): every cell's 4-point
    homography is G, whichever cell owns a pixel, so the whole frame is out(x) = src(G^-1 x) -- computed here in float64 with
    torch.linalg, sampled by grid_sample.  Pixel centres, map direction, the sign of the mesh motion and the constant border all
    have to agree; the only licence is cv2.remap's 1/32-pixel coordinate bucket + 1 LSB."""
    rng = np.random.RandomState(seed)
    n = 2
    frames = _smooth_frames(dev, n, H, W, seed)
    gx, gy = _grid(W, H, R, C)
    unstab = np.zeros((n, R + 1, C + 1, 2))
    stab = np.zeros_like(unstab)
    Gs = []
    for f in range(n):
        a = rng.uniform(-0.01, 0.01)
        G = np.array([[np.cos(a) * (1 + rng.uniform(-0.01, 0.01)), -np.sin(a) + rng.uniform(-0.004, 0.004), rng.uniform(-6, 6)],
                      [np.sin(a), np.cos(a) * (1 + rng.uniform(-0.01, 0.01)), rng.uniform(-6, 6)],
                      [rng.uniform(-4e-6, 4e-6), rng.uniform(-4e-6, 4e-6), 1.0]])
        Gs.append(G)
        X, Y = np.meshgrid(gx, gy)                                       # (R+1, C+1)
        w = G[2, 0] * X + G[2, 1] * Y + G[2, 2]
        stab[f, :, :, 0] = (G[0, 0] * X + G[0, 1] * Y + G[0, 2]) / w - X
        stab[f, :, :, 1] = (G[1, 0] * X + G[1, 1] * Y + G[1, 2]) / w - Y
    out, _ = _hip_warp(dev, frames, R, C, unstab, stab)
    xs, ys = _pixels(dev, n, H, W)
    Gi = torch.linalg.inv(torch.from_numpy(np.stack(Gs)).to(dev))      # (n, 3, 3) float64
    g = lambda i, j: Gi[:, i, j][:, None, None]
    w = g(2, 0) * xs + g(2, 1) * ys + g(2, 2)
    u = (g(0, 0) * xs + g(0, 1) * ys + g(0, 2)) / w
    v = (g(1, 0) * xs + g(1, 1) * ys + g(1, 2)) / w
    # Outside the warped mesh the reference paints the border colour where grid_sample still blends the frame's edge pixels with
    # black over one pixel: skip the ring of output pixels whose source lies within 1.5 pixels outside the frame
    ring = ((u < 0) & (u > -1.5)) | ((u > W - 1) & (u < W + 0.5)) | ((v < 0) & (v > -1.5)) | ((v > H - 1) & (v < H + 0.5))
    # (the vertices are float32 when cv2.findHomography sees them, mfs.py:1041: 1e-4 px at these coordinates -- inside the envelope)
    mean_abs = _assert_within_envelope(out, frames, u, v, allow=1.0, skip=ring)
    assert mean_abs < 0.6                                                # typical distance from the float64 value: rounding + bucket
    far = (u < -2) | (u > W + 1) | (v < -2) | (v > H + 1)                # well outside the frame: the border colour (black)
    assert bool((out[far] == 0).all())


def test_mesh_motion_vs_grid_sample_on_cell_interiors(dev):
    """Real mesh motion (every cell its own homography): per cell the exact 4-point homography is solved here with
    torch.linalg.solve (stabilized corners -> grid corners), and every output pixel that lies INSIDE the stabilized quad of
    exactly one cell, two pixels away from its edges, must be that cell's map sampled by grid_sample.  (Pixels near cell borders
    are owned by the painter order of mfs.py:1031-1061 -- pinned by the goldens, not judged here.)"""
    from meshflow_amd import synthetic
    H, W, R, C, n = 360, 640, 8, 8, 2
    frames = _smooth_frames(dev, n, H, W, 5)
    disp, hom = synthetic.motion(n + 6, R, C, seed=7, translation_sigma=2.0, field_sigma=1.5)
    unstab = disp[3:3 + n]
    stab = unstab + 0.6 * (disp[5:5 + n] - unstab)                       # some smooth per-vertex motion
    out, _ = _hip_warp(dev, frames, R, C, unstab, stab)
    gx, gy = _grid(W, H, R, C)
    xs, ys = _pixels(dev, 1, H, W)
    xs, ys = xs[0], ys[0]
    for f in range(n):
        u = torch.full((H, W), float('nan'), dtype=torch.float64, device=dev)
        v = torch.full_like(u, float('nan'))
        owners = torch.zeros((H, W), dtype=torch.int32, device=dev)
        P = np.stack(np.meshgrid(gx, gy), axis=-1) + (stab[f] - unstab[f])          # stabilized vertex positions (R+1, C+1, 2)
        for r in range(R):
            for c in range(C):
                src = np.array([P[r, c], P[r, c + 1], P[r + 1, c], P[r + 1, c + 1]]).astype(np.float32).astype(np.float64)
                dst = np.array([[gx[c], gy[r]], [gx[c + 1], gy[r]], [gx[c], gy[r + 1]], [gx[c + 1], gy[r + 1]]])
                A, b = [], []
                for (x, y), (X, Y) in zip(src, dst):                     # h maps (x, y) -> (X, Y), h22 = 1
                    A.append([x, y, 1, 0, 0, 0, -X * x, -X * y]); b.append(X)
                    A.append([0, 0, 0, x, y, 1, -Y * x, -Y * y]); b.append(Y)
                h = torch.linalg.solve(torch.tensor(A, dtype=torch.float64), torch.tensor(b, dtype=torch.float64))
                h = [float(t) for t in h] + [1.0]
                w = h[6] * xs + h[7] * ys + h[8]
                uu = (h[0] * xs + h[1] * ys + h[2]) / w
                vv = (h[3] * xs + h[4] * ys + h[5]) / w
                inside = (uu > gx[c] + 2) & (uu < gx[c + 1] - 2) & (vv > gy[r] + 2) & (vv < gy[r + 1] - 2)
                loose = (uu > gx[c] - 2) & (uu < gx[c + 1] + 2) & (vv > gy[r] - 2) & (vv < gy[r + 1] + 2)
                owners += loose.to(torch.int32)
                u = torch.where(inside, uu, u)
                v = torch.where(inside, vv, v)
        sure = ~torch.isnan(u) & (owners == 1)
        assert float(sure.double().mean()) > 0.6                          # most of the frame is judged
        u = torch.where(sure, u, torch.zeros_like(u)); v = torch.where(sure, v, torch.zeros_like(v))
        _assert_within_envelope(out[f:f + 1], frames[f:f + 1], u[None], v[None], allow=1.0, skip=~sure[None])


@pytest.mark.parametrize('H,W,rect', [(360, 640, (13, 11, 629, 350)), (1080, 1920, (17, 9, 1899, 1071)), (270, 484, (0, 0, 483, 269)),
                                      (270, 484, (40, 30, 443, 239))])
def test_crop_resize_vs_interpolate(dev, H, W, rect):
    """_crop_frames (mfs.py:1111-1157: crop to the inclusive rectangle, cv2.resize back to (W, H), INTER_LINEAR) against
    torch's bilinear interpolate with half-pixel centres (align_corners=False), float64: within 1 LSB (cv2 quantises the
    weights to 11 bits and truncates twice); the full-frame rectangle is the identity."""
    from meshflow_amd import ops
    frames = _smooth_frames(dev, 2, H, W, 9)
    left, top, right, bottom = rect
    got = ops.crop_resize(frames, rect)
    crop = frames[:, top:bottom + 1, left:right + 1].permute(0, 3, 1, 2).to(torch.float64)
    want = F_.interpolate(crop, size=(H, W), mode='bilinear', align_corners=False, antialias=False).permute(0, 2, 3, 1)
    diff = (got.to(torch.float64) - want).abs()
    assert float(diff.max()) <= 1.0 + 1e-9, float(diff.max())
    assert float(diff.mean()) < 0.35
    if rect == (0, 0, W - 1, H - 1):
        assert torch.equal(got, frames)
    # and on noise (worst case for interpolation): still within 1 LSB of the float64 result + its rounding
    noise = torch.randint(0, 256, (1, H, W, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(device=dev).manual_seed(3))
    got = ops.crop_resize(noise, rect)
    crop = noise[:, top:bottom + 1, left:right + 1].permute(0, 3, 1, 2).to(torch.float64)
    want = F_.interpolate(crop, size=(H, W), mode='bilinear', align_corners=False, antialias=False).permute(0, 2, 3, 1)
    assert float((got.to(torch.float64) - want).abs().max()) <= 1.0 + 1e-9


# ---- the four formats and resize-to, judged by tests/second_opinion.py with its constants -------------------------------------------------
# Every bound below lives in second_opinion.py and was fixed on the CPU against the models (tests/test_second_opinion_models.py).

PLANES = {'smooth': so.smooth_planes, 'noise': so.noise_planes}
SMALL_WARP = [c for c in so.WARP_CASES if c.kind != 'far']
LARGE_WARP = so.WARP_CASES_1080P


def _to_dev(fmt, planes, dev):
    """float64 planes -> the device stack `ops` takes (uint16 moved as bytes)."""
    a = np.ascontiguousarray(so.to_numpy(fmt, planes))
    t = torch.from_numpy(a.view(np.uint8)).to(dev)
    return t.view(torch.uint16) if a.dtype == np.uint16 else t


def _to_planes(t, dev):
    a = t.contiguous().view(torch.uint8).cpu().numpy().view(np.uint16) if t.dtype == torch.uint16 else t.cpu().numpy()
    return so.to_planes(a, dev)


def _kernel_warp(dev, fmt, planes, R, C, unstab, stab, border):
    out, _ = _hip_warp(dev, _to_dev(fmt, planes, dev), R, C, unstab, stab, border)
    return _to_planes(out, dev)


def _kernel_warp_findings(dev, fmt, case, kind, border=(0, 0, 0), with_model=False):
    """Like test_second_opinion_models.warp_case_findings with the kernel in the model's place; with_model: the model through the same
    judge must give the same numbers."""
    planes = PLANES[kind](fmt, case.n, case.H, case.W, case.seed, dev)
    found = []
    for setup in so.warp_setups(case, dev):
        got = _kernel_warp(dev, fmt, planes, case.R, case.C, setup.unstab, setup.stab, border)
        f = so.warp_findings(fmt, got, planes, setup, border)
        found.append((f, so.warp_violations(fmt, f, setup, kind == 'smooth')))
        if with_model:
            import test_second_opinion_models as models
            want = so.to_planes(models.model_warp(fmt, so.to_numpy(fmt, planes), case.R, case.C, setup.unstab, setup.stab, border), dev)
            assert so.warp_findings(fmt, want, planes, setup, border) == f
    return found


@pytest.mark.parametrize('kind', ['smooth', 'noise'])
@pytest.mark.parametrize('fmt', so.FORMATS)
@pytest.mark.parametrize('case', SMALL_WARP + LARGE_WARP, ids=lambda c: f'{c.kind}-{c.H}x{c.W}-{c.R}')
def test_warp_formats_vs_grid_sample(dev, case, fmt, kind):
    """ops.warp in each format: identity and integer shifts exact, a global homography and real mesh motion inside the envelope, the mean
    signed difference of uint16 within its bound; on the CPU-sized cases the model gives the same numbers."""
    found = _kernel_warp_findings(dev, fmt, case, kind, with_model=case in SMALL_WARP)
    assert not [v for _, vs in found for v in vs], found


@pytest.mark.parametrize('fmt', so.FORMATS)
def test_warp_borders_vs_grid_sample(dev, fmt):
    """A non-black border per format: exactly the border far outside the mesh (uint16 (0, 0, 255) -> 255; u8c4 alpha 0 from 3 components,
    the given alpha from 4), blended into the pixels next to the ring as the float64 sampler blends it."""
    far = next(c for c in so.WARP_CASES if c.kind == 'far')
    hom = next(c for c in so.WARP_CASES if c.kind == 'homography')
    borders = [so.BORDERS[fmt]] + ([so.BORDERS['u8c4'][:3]] if fmt == 'u8c4' else [])
    for border in borders:
        for case in (far, hom):
            found = _kernel_warp_findings(dev, fmt, case, 'smooth', border, with_model=True)
            assert not [v for _, vs in found for v in vs], found


def _kernel_resize_findings(dev, fmt, case, kind, same_size=False, with_model=False):
    from meshflow_amd import ops
    n, H, W, rect, (ow, oh) = case
    planes = PLANES[kind](fmt, n, H, W, 9, dev)
    frames = _to_dev(fmt, planes, dev)
    out = ops.crop_resize(frames, rect) if same_size else ops.crop_resize(frames, rect, size=(ow, oh))
    torch.cuda.synchronize()
    got = _to_planes(out, dev)
    assert tuple(got.shape[:3]) == (n, oh, ow)
    f = so.resize_findings(fmt, got, planes, rect, ow, oh)
    if with_model:
        import test_second_opinion_models as models
        want = so.to_planes(models.model_resize(fmt, so.to_numpy(fmt, planes), rect, ow, oh), dev)
        assert so.resize_findings(fmt, want, planes, rect, ow, oh) == f
    return f, so.resize_violations(fmt, f, rect, ow, oh, kind == 'smooth')


@pytest.mark.parametrize('kind', ['smooth', 'noise'])
@pytest.mark.parametrize('fmt', so.FORMATS)
@pytest.mark.parametrize('case', range(len(so.RESIZE_CASES) + len(so.RESIZE_CASES_1080P)))
def test_crop_resize_to_vs_interpolate(dev, case, fmt, kind):
    """ops.crop_resize(size=...) in each format over the device suite's case list and 1080p downscales on both sides of every staged /
    direct cut-over, against float64 `interpolate` of the crop."""
    small = case < len(so.RESIZE_CASES)
    f, violations = _kernel_resize_findings(dev, fmt, (so.RESIZE_CASES + so.RESIZE_CASES_1080P)[case], kind, with_model=small)
    assert not violations, (f, violations)


@pytest.mark.parametrize('fmt', so.FORMATS)
def test_crop_resize_same_size_formats_vs_interpolate(dev, fmt):
    """The call without `size` (back to the frame size) in each format, 1080p included."""
    for n, H, W, rect in so.SAME_SIZE_CASES + so.SAME_SIZE_CASES_1080P:
        for kind in ('smooth', 'noise'):
            f, violations = _kernel_resize_findings(dev, fmt, (n, H, W, rect, (W, H)), kind, same_size=True, with_model=H < 1080)
            assert not violations, (f, violations)


# ---- NV12 and P010: the pair judged whole, chroma by the chroma rows of tests/second_opinion.py ----------------------------------------------
# Luma as u8c1 / as a one-channel 16-bit plane with u16c3's constants; chroma as the two-channel plane at the even luma pixels' positions
# halved (warp) or at the absolute float64 positions (crop-resize).  Proven on the CPU models first, like everything above.

WARP_420 = so.WARP_CASES_420 + [so.WARP_CASES_1080P[0]]
RESIZE_420 = so.RESIZE_CASES_420 + so.RESIZE_CASES_1080P


def _pair_to_dev(fmt, y, uv, dev):
    return _to_dev(so.LUMA_OF[fmt], y, dev), _to_dev(so.CHROMA_OF[fmt], uv, dev)


def _kernel_warp_420(dev, fmt, y, uv, case, setup, border):
    """(out_y, out_uv) of ops.warp_nv12 / ops.warp_p010 as device tensors."""
    from meshflow_amd import ops
    d_y, d_uv = _pair_to_dev(fmt, y, uv, dev)
    table = ops.cell_table(torch.from_numpy(np.ascontiguousarray(setup.unstab)).to(dev), torch.from_numpy(np.ascontiguousarray(setup.stab)).to(dev),
                           case.W, case.H, case.R, case.C)
    out_y, out_uv = {'nv12': ops.warp_nv12, 'p010': ops.warp_p010}[fmt](d_y, d_uv, table, border)
    torch.cuda.synchronize()
    table.check()
    return out_y, out_uv


def _same_bits(t, a):
    got = t.contiguous().view(torch.uint8).cpu().numpy().view(a.dtype).reshape(a.shape)
    return np.array_equal(got, a), (int((got != a).sum()), np.argwhere(got != a)[:5].tolist())


def _warp_420_findings(dev, fmt, case, kind, with_model, planes=None):
    """[(luma findings, chroma findings, violations)] per setup; with_model: the model's planes equal the kernel's bit for bit and go
    through the judge to the same numbers."""
    import test_second_opinion_models as models
    border = so.BORDERS_YUV[fmt]
    y, uv = planes or so.planes_420(fmt, kind, case.n, case.H, case.W, case.seed, dev)
    found = []
    for setup in so.warp_setups(case, dev):
        out_y, out_uv = _kernel_warp_420(dev, fmt, y, uv, case, setup, border)
        f = so.warp_findings_420(fmt, _to_planes(out_y, dev), _to_planes(out_uv, dev), y, uv, setup, border, kind == 'smooth')
        print(fmt, case.kind, f'{case.H}x{case.W}', kind, 'luma', {k: f[0][k] for k in ('label', 'worst', 'share')}, 'chroma',
              {k: f[1][k] for k in ('worst', 'share', 'mean_signed', 'far_bad', 'far_pixels')})
        found.append(f)
        if with_model:
            want_y, want_uv = models.model_warp_420(fmt, so.to_numpy(so.LUMA_OF[fmt], y), so.to_numpy(so.CHROMA_OF[fmt], uv), case, setup, border)
            same_y, same_uv = _same_bits(out_y, want_y), _same_bits(out_uv, want_uv)
            assert same_y[0] and same_uv[0], (setup.label, 'luma', same_y[1], 'chroma', same_uv[1])
            assert so.warp_findings_420(fmt, so.to_planes(want_y, dev), so.to_planes(want_uv, dev), y, uv, setup, border, kind == 'smooth') == f
    return found


@pytest.mark.parametrize('kind', ['smooth', 'noise'])
@pytest.mark.parametrize('fmt', so.FORMATS_420)
@pytest.mark.parametrize('case', WARP_420, ids=lambda c: f'{c.kind}-{c.H}x{c.W}-{c.R}')
def test_warp_420_vs_grid_sample(dev, case, fmt, kind):
    """ops.warp_nv12 / ops.warp_p010 with a (Y, U, V) border whose components all differ: luma and chroma exact under identity and even
    shifts, inside their envelopes otherwise, exactly the border far outside, the P010 chroma mean within its bound; up to 360 x 640 the
    kernel's planes are the model's bit for bit."""
    found = _warp_420_findings(dev, fmt, case, kind, with_model=case.H < 1080)
    assert not [v for _, _, vs in found for v in vs], found
    if case.kind == 'far':
        assert found[0][1]['far_pixels'] > 250


@pytest.mark.parametrize('fmt', so.FORMATS_420)
def test_warp_420_is_the_model_at_1080p(dev, fmt):
    """One 1080p noise frame under a homography: both planes bit for bit the model's."""
    case = so.WARP_CASES_1080P[0]
    found = _warp_420_findings(dev, fmt, case, 'noise', with_model=True)
    assert not [v for _, _, vs in found for v in vs], found


def _resize_420_findings(dev, fmt, case, kind, same_size=False, planes=None):
    """(luma findings, chroma findings, violations), the kernel's planes bit for bit the model's and the model judged to the same numbers."""
    from meshflow_amd import ops
    import test_second_opinion_models as models
    n, H, W, rect, (ow, oh) = case
    y, uv = planes or so.planes_420(fmt, kind, n, H, W, 9, dev)
    d_y, d_uv = _pair_to_dev(fmt, y, uv, dev)
    call = {'nv12': ops.crop_resize_nv12, 'p010': ops.crop_resize_p010}[fmt]
    out_y, out_uv = call(d_y, d_uv, rect) if same_size else call(d_y, d_uv, rect, size=(ow, oh))
    torch.cuda.synchronize()
    assert tuple(out_y.shape) == (n, oh, ow) and tuple(out_uv.shape) == (n, oh // 2, ow // 2, 2)
    f = so.resize_findings_420(fmt, _to_planes(out_y, dev), _to_planes(out_uv, dev), y, uv, rect, ow, oh)
    print(fmt, f'{H}x{W}', rect, (ow, oh), kind, 'luma', f[0]['worst'], 'chroma', f[1]['worst'])
    want_y, want_uv = models.model_resize_420(fmt, so.to_numpy(so.LUMA_OF[fmt], y), so.to_numpy(so.CHROMA_OF[fmt], uv), rect, (ow, oh))
    same_y, same_uv = _same_bits(out_y, want_y), _same_bits(out_uv, want_uv)
    assert same_y[0] and same_uv[0], ('luma', same_y[1], 'chroma', same_uv[1])
    assert so.resize_findings_420(fmt, so.to_planes(want_y, dev), so.to_planes(want_uv, dev), y, uv, rect, ow, oh) == f
    return (out_y, out_uv), f


@pytest.mark.parametrize('kind', ['smooth', 'noise'])
@pytest.mark.parametrize('fmt', so.FORMATS_420)
@pytest.mark.parametrize('case', range(len(RESIZE_420)))
def test_crop_resize_420_vs_float64_positions(dev, case, fmt, kind):
    """ops.crop_resize_nv12 / ops.crop_resize_p010 over the 4:2:0 table (every parity of every edge, one-pixel crops) and the 1080p
    downscales on both sides of every staged / direct cut-over: luma against `interpolate` of the crop, chroma against the whole chroma
    plane sampled at the absolute float64 positions; bit for bit the model at every size."""
    _, f = _resize_420_findings(dev, fmt, RESIZE_420[case], kind)
    assert not f[2], f


@pytest.mark.parametrize('fmt', so.FORMATS_420)
def test_crop_resize_420_same_size_vs_float64_positions(dev, fmt):
    """The call without `size`, 1080p included."""
    for n, H, W, rect in so.SAME_SIZE_CASES + so.SAME_SIZE_CASES_1080P:
        _, f = _resize_420_findings(dev, fmt, (n, H, W, rect, (W, H)), 'noise', same_size=True)
        assert not f[2], f


@pytest.mark.parametrize('fmt', so.FORMATS_420)
def test_ramp_registration_of_the_kernels(dev, fmt):
    """Chroma registered on luma without a model of siting: on a linear ramp out_uv[cy, cx] is out_y[2 cy, 2 cx] (less the channel's
    offset) within the bound derived in second_opinion.registration_warp / registration_resize, under a homography and under a crop with
    an odd left and top.  Chroma sited at the odd luma sample is off by sx + sy LSB, several times the bound."""
    case = so.REGISTRATION_WARP[fmt]
    y, uv = so.ramp_420(fmt, case.n, case.H, case.W, dev)
    setup = next(so.warp_setups(case, dev))
    out_y, out_uv = _kernel_warp_420(dev, fmt, y, uv, case, setup, so.BORDERS_YUV[fmt])
    worst, compared, bound = so.registration_warp(fmt, _to_planes(out_y, dev), _to_planes(out_uv, dev), setup)
    print(fmt, 'warp', worst, compared, bound)
    assert worst <= bound and compared > 0.8 * case.n * case.H * case.W / 4
    assert so.RAMP[fmt]['sx'] + so.RAMP[fmt]['sy'] > 3 * bound
    n, H, W, rect, (ow, oh) = so.REGISTRATION_RESIZE[fmt]
    planes = so.ramp_420(fmt, n, H, W, dev)
    (out_y, out_uv), _ = _resize_420_findings(dev, fmt, so.REGISTRATION_RESIZE[fmt], 'ramp', planes=planes)
    worst, compared, bound = so.registration_resize(fmt, _to_planes(out_y, dev), _to_planes(out_uv, dev), H, W, rect, ow, oh)
    print(fmt, 'resize', worst, compared, bound)
    assert worst <= bound and compared >= n * (ow // 2 - 2) * (oh // 2 - 2)
