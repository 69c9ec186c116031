"""-m gpu: the NV16 crop-resize -- `ops.crop_resize_nv16` with a host rectangle and with one that stays on the device,
`ops.crop_resize_packed_422`, `MeshFlowStabilizer.stabilized_nv16_cropped` and `stabilized_packed_422_cropped`.

Every equality is byte for byte.  Both planes are compared with tests/nv16_crop_model.py; luma also with `ops.crop_resize` /
`ops.crop_resize_resident` of y (the grey crop-resize, itself proven against the oracle); the host path with the device path.  The case table
(tests/nv16_crop_cases.py) is checked on the CPU to hold low-clamped, high-clamped and interior chroma samples in x and in y before a kernel
result is looked at."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nv16_crop_cases as cases  # noqa: E402
import nv16_crop_model as model  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def put(a, dev):
    return torch.from_numpy(np.array(a, copy=True)).to(dev)             # (a writable copy: the cases' arrays are read-only)


def differing(got, want):
    d = got != want
    return int(d.sum()), np.argwhere(d)[:5].tolist()


@pytest.mark.parametrize('name', cases.NAMES)
def test_crop_resize_nv16_equals_the_model_and_the_grey_crop(dev, name):
    from meshflow_amd import ops
    counts = cases.class_counts()                                       # from the model alone, before any kernel result
    for axis in ('x', 'y'):
        assert min(counts[axis]) > 0, counts
    c = cases.frame(name)
    print(name, len(c['cases']), 'cases; classes of the table (low, high, interior):', counts)
    y, uv = put(c['y'], dev), put(c['uv'], dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    for rect, size in c['cases']:
        want_y, want_uv = cases.want(name, rect, size)
        arg = None if size == (c['W'], c['H']) and rect[0] % 2 == 0 else size          # (the default size, taken now and then)
        got_y, got_uv = ops.crop_resize_nv16(y, uv, rect, size=arg)
        bounds = torch.tensor(rect, dtype=torch.int32, device=dev)
        dev_y, dev_uv, st = ops.crop_resize_nv16(y, uv, bounds, size=arg, status=status)
        grey = ops.crop_resize(y, rect, size=size)
        grey_dev, _ = ops.crop_resize_resident(y, bounds, size=size)
        assert st is status
        assert tuple(got_y.shape) == want_y.shape and tuple(got_uv.shape) == want_uv.shape == (c['n'], size[1], size[0] // 2, 2), (rect, size)
        assert torch.equal(got_y, grey) and torch.equal(dev_y, grey_dev), (rect, size)
        g = got_y.cpu().numpy()
        assert np.array_equal(g, want_y), (rect, size, differing(g, want_y))
        g = got_uv.cpu().numpy()
        assert np.array_equal(g, want_uv), (rect, size, differing(g, want_uv))
        assert torch.equal(dev_y, got_y) and torch.equal(dev_uv, got_uv), (rect, size)
    assert int(status.item()) == 0
    assert np.array_equal(y.cpu().numpy(), c['y']) and np.array_equal(uv.cpu().numpy(), c['uv'])


def test_at_x_identity_the_y_axis_is_the_grey_kernel_s(dev):
    """left even and oW == cw: U planted into the even columns of a grey plane; out_u[:, cx] is then `ops.crop_resize(grey)[:, 2 cx]` -- the
    grey KERNEL's bytes, not the model's."""
    from meshflow_amd import ops
    c = cases.frame('100x71')
    W, H = c['W'], c['H']
    grey = np.array(c['y'], copy=True)
    grey[:, :, 0::2] = c['uv'][..., 0]
    y, uv, d_grey = put(c['y'], dev), put(c['uv'], dev), put(grey, dev)
    for rect in ((0, 0, W - 1, H - 1), (2, 3, W - 3, H - 4), (4, 1, W - 1, H - 1), (6, 5, 9, 5)):
        cw, ch = rect[2] - rect[0] + 1, rect[3] - rect[1] + 1
        for oH in (H, 2 * ch + 1, max(2, ch // 2), max(2, ch // 5), 3):
            _, got_uv = ops.crop_resize_nv16(y, uv, rect, size=(cw, oH))
            lum = ops.crop_resize(d_grey, rect, size=(cw, oH))
            assert torch.equal(got_uv[..., 0], lum[:, :, 0::2]), (rect, oH)


def offset(a, off, dev, pad=48):
    """`a` in a sentinel-filled buffer, `off` bytes past a 16-byte boundary: (buffer, lead, the view)."""
    raw = np.array(a, copy=True).reshape(-1)
    buf = torch.full((raw.size + pad,), 0xA5, dtype=torch.uint8, device=dev)
    lead = (-buf.data_ptr()) % 16 + off
    t = buf[lead:lead + raw.size]
    t.copy_(torch.from_numpy(raw).to(dev))
    return buf, lead, t.view(a.shape)


def test_odd_addresses_and_canaries_around_every_buffer(dev):
    """`out=`: the pair comes back; luma at odd addresses and chroma 2, 6 and 14 bytes past a 16-byte boundary, inputs and outputs alike, gives
    the same bytes and leaves the sentinel around all four buffers alone."""
    from meshflow_amd import ops
    name = '66x49'
    c = cases.frame(name)
    for rect, size in (((3, 3, 62, 46), (92, 73)), ((2, 1, 65, 48), (64, 48)), ((3, 2, 65, 48), (14, 9))):
        want_y, want_uv = cases.want(name, rect, size)
        bounds = torch.tensor(rect, dtype=torch.int32, device=dev)
        for y_off, uv_off in ((0, 0), (1, 2), (3, 6), (1, 14)):
            iy = offset(c['y'], y_off, dev)
            iuv = offset(c['uv'], uv_off, dev)
            for b in (rect, bounds):
                oy = offset(np.full_like(want_y, 0xA5), y_off, dev)
                ouv = offset(np.full_like(want_uv, 0xA5), uv_off, dev)
                res = ops.crop_resize_nv16(iy[2], iuv[2], b, size=size, out=(oy[2], ouv[2]))
                assert res[0].data_ptr() == oy[2].data_ptr() and res[1].data_ptr() == ouv[2].data_ptr()
                assert np.array_equal(oy[2].cpu().numpy(), want_y) and np.array_equal(ouv[2].cpu().numpy(), want_uv), (rect, size, y_off, uv_off)
                for buf, lead, t in (oy, ouv, iy, iuv):
                    assert bool((buf[:lead] == 0xA5).all()) and bool((buf[lead + t.numel():] == 0xA5).all()), (rect, size, y_off, uv_off)
            assert np.array_equal(iy[2].cpu().numpy(), c['y']) and np.array_equal(iuv[2].cpu().numpy(), c['uv'])


def at_the_end(a, lead, dev):
    """`a` as the LAST bytes of a device tensor of its own, `lead` bytes into it: the stack's last sample is the last byte the tensor holds."""
    raw = np.array(a, copy=True).reshape(-1)
    buf = torch.empty((lead + raw.size,), dtype=torch.uint8, device=dev)
    t = buf[lead:]
    t.copy_(torch.from_numpy(raw).to(dev))
    assert t.data_ptr() + t.numel() == buf.data_ptr() + buf.numel()
    return t.view(a.shape)


def test_the_last_sample_of_the_stack_at_the_end_of_its_allocation(dev):
    """The stacks end where their tensors' bytes end (nothing of theirs behind them), luma at an odd address and chroma at a 2-byte one, and
    the rectangles reach the last column and row of the last frame: where s == c1 only the 2-byte sample is read, so the call reads nothing
    behind the stack -- and gives the model's bytes."""
    from meshflow_amd import ops
    for name in ('66x49', '2x35', '2x2'):
        c = cases.frame(name)
        W, H = c['W'], c['H']
        y, uv = at_the_end(c['y'], 33, dev), at_the_end(c['uv'], 34, dev)
        for rect in ((0, 0, W - 1, H - 1), (W - 1, H - 1, W - 1, H - 1), (1, 1, W - 1, H - 1)):
            for size in ((W, H), (2 * W + 2, 2 * H + 1), (2, 3)):
                want_y, want_uv = model.crop_resize_clip(c['y'], c['uv'], rect, size)
                got_y, got_uv = ops.crop_resize_nv16(y, uv, rect, size=size)
                dev_y, dev_uv, st = ops.crop_resize_nv16(y, uv, torch.tensor(rect, dtype=torch.int32, device=dev), size=size)
                assert int(st.item()) == 0
                for g, w in ((got_y, want_y), (dev_y, want_y), (got_uv, want_uv), (dev_uv, want_uv)):
                    assert np.array_equal(g.cpu().numpy(), w), (name, rect, size)


@pytest.mark.parametrize('name,rect,size', [('100x71', (3, 3, 96, 67), (100, 71)), ('100x71', (5, 7, 5, 7), (20, 13)),
                                            ('66x49', (2, 3, 63, 45), (30, 9)), ('64x48', (63, 47, 63, 47), (64, 48))])
def test_nothing_outside_the_crop_influences_the_result(dev, name, rect, size):
    """Every chroma sample outside columns c0 .. c1 x rows top .. bottom and every luma pixel outside the rectangle re-randomised: the same
    bytes."""
    from meshflow_amd import ops
    c = cases.frame(name)
    left, top, right, bottom = rect
    c0, c1 = model.axis_range(left, right)
    rng = np.random.default_rng(77)
    y2 = rng.integers(0, 256, c['y'].shape, dtype=np.uint8)
    uv2 = rng.integers(0, 256, c['uv'].shape, dtype=np.uint8)
    y2[:, top:bottom + 1, left:right + 1] = c['y'][:, top:bottom + 1, left:right + 1]
    uv2[:, top:bottom + 1, c0:c1 + 1] = c['uv'][:, top:bottom + 1, c0:c1 + 1]
    assert not np.array_equal(uv2, c['uv']) and not np.array_equal(y2, c['y'])
    want_y, want_uv = model.crop_resize_clip(c['y'], c['uv'], rect, size)
    bounds = torch.tensor(rect, dtype=torch.int32, device=dev)
    for yy, uu in ((c['y'], c['uv']), (y2, uv2)):
        got_y, got_uv = ops.crop_resize_nv16(put(yy, dev), put(uu, dev), rect, size=size)
        dev_y, dev_uv, _ = ops.crop_resize_nv16(put(yy, dev), put(uu, dev), bounds, size=size)
        for g, w in ((got_y, want_y), (dev_y, want_y), (got_uv, want_uv), (dev_uv, want_uv)):
            assert np.array_equal(g.cpu().numpy(), w)


def test_unusable_device_rectangles(dev):
    """Empty, negative, outside the frame: the status rises by exactly 1 per call and accumulates, the sentinel-filled outputs, the planes AND
    the workspace stay untouched (the C call, on a workspace of the test's own), and a usable call afterwards is correct."""
    import ctypes
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
        oy = torch.full((n, size[1], size[0]), 0x5A, dtype=torch.uint8, device=dev)
        ouv = torch.full((n, size[1], size[0] // 2, 2), 0x5A, dtype=torch.uint8, device=dev)
        work = torch.full((_lib.lib.mf_crop_resize_nv16_workspace_bytes(*size),), 0x3C, dtype=torch.uint8, device=dev)
        before = int(status.item())
        for k, rect in enumerate(bad):
            bounds = torch.tensor(rect, dtype=torch.int32, device=dev)
            if k % 2:
                _, _, st = ops.crop_resize_nv16(y, uv, bounds, size=size, out=(oy, ouv), status=status)
                assert st is status
            else:
                _lib.check(_lib.lib.mf_crop_resize_dev_nv16(vp(y.data_ptr()), vp(uv.data_ptr()), vp(oy.data_ptr()), vp(ouv.data_ptr()), n, W, H,
                                                            vp(bounds.data_ptr()), size[0], size[1], vp(work.data_ptr()), vp(status.data_ptr()),
                                                            vp(stream)))
            assert int(status.item()) == before + k + 1, (rect, size)
        assert bool((oy == 0x5A).all()) and bool((ouv == 0x5A).all()) and bool((work == 0x3C).all()), size
        rect = (3, 3, 62, 46)
        bounds = torch.tensor(rect, dtype=torch.int32, device=dev)
        ops.crop_resize_nv16(y, uv, bounds, size=size, out=(oy, ouv), status=status)
        assert int(status.item()) == before + len(bad)
        want_y, want_uv = model.crop_resize_clip(c['y'], c['uv'], rect, size)
        assert np.array_equal(oy.cpu().numpy(), want_y) and np.array_equal(ouv.cpu().numpy(), want_uv), size
    _, _, fresh = ops.crop_resize_nv16(y, uv, torch.tensor(bad[0], dtype=torch.int32, device=dev))
    assert int(fresh.item()) == 1                                       # a status of the call's own starts at zero
    assert np.array_equal(y.cpu().numpy(), c['y']) and np.array_equal(uv.cpu().numpy(), c['uv'])


@pytest.fixture(scope='module')
def shaky(dev):
    """An 8-frame NV16 clip of 96 x 65 with synthetic motion, its stabilizer, and `stabilized_nv16`'s uncropped result."""
    from meshflow_amd import synthetic
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    F, H, W, R, C = 8, 65, 96, 3, 4
    disp, hom = synthetic.motion(F, R, C, seed=71, jitter_sigma=2.0)
    s = MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, temporal_smoothing_radius=4, optimization_num_iterations=15, device='cuda:0')
    rng = np.random.default_rng(8)
    y = put(rng.integers(0, 256, (F, H, W), dtype=np.uint8), dev)
    uv = put(rng.integers(0, 256, (F, H, W // 2, 2), dtype=np.uint8), dev)
    d_disp = torch.from_numpy(np.ascontiguousarray(disp, dtype=np.float64)).to(dev)
    plain_y, plain_uv, b = s.stabilized_nv16(y, uv, d_disp, hom, (60, 100, 200))
    rect = tuple(b.tolist())
    assert rect != (0, 0, W - 1, H - 1) and 0 <= rect[0] <= rect[2] < W and 0 <= rect[1] <= rect[3] < H
    return dict(s=s, F=F, H=H, W=W, y=y, uv=uv, d_disp=d_disp, hom=hom, border=(60, 100, 200), plain=(plain_y, plain_uv), bounds=b, rect=rect)


def test_stabilized_nv16_cropped(dev, shaky):
    """Equals `ops.crop_resize_nv16` of `stabilized_nv16`'s result with the returned bounds, from the device and from the host rectangle, and
    the model on one frame; `out=` names the cropped pair."""
    from meshflow_amd import ops
    k = shaky
    s, y, uv, d_disp, hom, border, (plain_y, plain_uv), b, rect = (k[x] for x in ('s', 'y', 'uv', 'd_disp', 'hom', 'border', 'plain', 'bounds', 'rect'))
    for size in (None, (128, 91), (48, 33)):
        got_y, got_uv, gb = s.stabilized_nv16_cropped(y, uv, d_disp, hom, border, output_size=size)
        want_y, want_uv, st = ops.crop_resize_nv16(plain_y, plain_uv, b, size=size)
        host_y, host_uv = ops.crop_resize_nv16(plain_y, plain_uv, rect, size=size)
        assert int(st.item()) == 0 and torch.equal(gb, b)
        assert torch.equal(got_y, want_y) and torch.equal(got_uv, want_uv) and torch.equal(got_y, host_y) and torch.equal(got_uv, host_uv), size
        my, muv = model.crop_resize_frame(plain_y[3].cpu().numpy(), plain_uv[3].cpu().numpy(), rect, size)
        assert np.array_equal(got_y[3].cpu().numpy(), my) and np.array_equal(got_uv[3].cpu().numpy(), muv), size
    oy = torch.empty((k['F'], 33, 48), dtype=torch.uint8, device=dev)
    ouv = torch.empty((k['F'], 33, 24, 2), dtype=torch.uint8, device=dev)
    r_y, r_uv, _ = s.stabilized_nv16_cropped(y, uv, d_disp, hom, border, out=(oy, ouv), output_size=(48, 33))
    assert r_y.data_ptr() == oy.data_ptr() and r_uv.data_ptr() == ouv.data_ptr() and torch.equal(oy, got_y) and torch.equal(ouv, got_uv)
    with pytest.raises(ValueError):
        s.stabilized_nv16_cropped(y, uv, d_disp, hom, border, output_size=(47, 32))
    with pytest.raises(ValueError):
        s.stabilized_nv16_cropped(y, uv, d_disp, hom, border, out=(plain_y, plain_uv), output_size=(48, 33))


@pytest.mark.parametrize('order', ['yuyv', 'uyvy'])
def test_the_packed_calls_are_their_definitions(dev, shaky, order):
    """`crop_resize_packed_422` is unpack, `crop_resize_nv16`, pack; `stabilized_packed_422_cropped` is unpack, the warp, the crop-resize, pack."""
    from meshflow_amd import ops
    k = shaky
    s, y, uv, d_disp, hom, border, b, rect = (k[x] for x in ('s', 'y', 'uv', 'd_disp', 'hom', 'border', 'bounds', 'rect'))
    packed = ops.pack_422(y, uv, order)
    keep = packed.clone()
    for size in (None, (128, 91), (48, 33)):
        ny, nuv = ops.crop_resize_nv16(y, uv, rect, size=size)
        want = ops.pack_422(ny, nuv, order)
        got = ops.crop_resize_packed_422(packed, rect, order, size=size)
        got_dev, st = ops.crop_resize_packed_422(packed, b, order, size=size)
        assert int(st.item()) == 0 and torch.equal(got, want) and torch.equal(got_dev, want), (order, size)
        assert tuple(got.shape) == (k['F'],) + ((k['H'], k['W']) if size is None else (size[1], size[0])) + (2,)
        sy, suv, sb = s.stabilized_nv16_cropped(y, uv, d_disp, hom, border, output_size=size)
        out, ob = s.stabilized_packed_422_cropped(packed, d_disp, hom, order, border, output_size=size)
        assert torch.equal(ob, sb) and torch.equal(out, ops.pack_422(sy, suv, order)), (order, size)
    buf = torch.full((k['F'], 33, 48, 2), 0xA5, dtype=torch.uint8, device=dev)
    assert ops.crop_resize_packed_422(packed, rect, order, size=(48, 33), out=buf).data_ptr() == buf.data_ptr() and torch.equal(buf, got)
    buf.fill_(0xA5)
    r, _ = s.stabilized_packed_422_cropped(packed, d_disp, hom, order, border, out=buf, output_size=(48, 33))
    assert r.data_ptr() == buf.data_ptr() and torch.equal(buf, out)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    _, st = ops.crop_resize_packed_422(packed, torch.tensor((5, 3, 4, 40), dtype=torch.int32, device=dev), order, status=status)
    assert st is status and int(status.item()) == 1
    assert torch.equal(packed, keep)
