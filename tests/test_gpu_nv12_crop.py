"""-m gpu: the NV12 crop-resize -- `ops.crop_resize_nv12` with a host rectangle and with one that stays on the device, and
`MeshFlowStabilizer.stabilized_nv12(crop=True)`.

Every equality is byte for byte.  Both planes are compared with tests/nv12_crop_model.py; luma also with `ops.crop_resize` /
`ops.crop_resize_resident` of y (the grey crop-resize, itself proven against the oracle); the host path with the device path.  The case table
(tests/nv12_crop_cases.py) is checked on the CPU to hold low-clamped, high-clamped and interior chroma samples in x and in y before a kernel
result is looked at."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nv12_crop_cases as cases  # noqa: E402
import nv12_crop_model as model  # noqa: E402


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
def test_crop_resize_nv12_equals_the_model_and_the_grey_crop(dev, name):
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
        got_y, got_uv = ops.crop_resize_nv12(y, uv, rect, size=arg)
        bounds = torch.tensor(rect, dtype=torch.int32, device=dev)
        dev_y, dev_uv, st = ops.crop_resize_nv12(y, uv, bounds, size=arg, status=status)
        grey = ops.crop_resize(y, rect, size=size)
        grey_dev, _ = ops.crop_resize_resident(y, bounds, size=size)
        assert st is status
        assert tuple(got_y.shape) == want_y.shape and tuple(got_uv.shape) == want_uv.shape, (rect, size)
        assert torch.equal(got_y, grey) and torch.equal(dev_y, grey_dev), (rect, size)
        g = got_y.cpu().numpy()
        assert np.array_equal(g, want_y), (rect, size, differing(g, want_y))
        g = got_uv.cpu().numpy()
        assert np.array_equal(g, want_uv), (rect, size, differing(g, want_uv))
        assert torch.equal(dev_y, got_y) and torch.equal(dev_uv, got_uv), (rect, size)
    assert int(status.item()) == 0
    assert np.array_equal(y.cpu().numpy(), c['y']) and np.array_equal(uv.cpu().numpy(), c['uv'])


def test_out_pair_is_filled_and_nothing_around_it(dev):
    """`out=`: the pair comes back; chroma 2, 6 and 14 bytes past a 16-byte boundary, inputs and outputs alike, gives the same bytes and leaves
    the sentinel around the outputs alone."""
    from meshflow_amd import ops
    name, rect, size = '66x50', (3, 3, 62, 47), (92, 74)
    c = cases.frame(name)
    want_y, want_uv = cases.want(name, rect, size)

    def offset(a, off):
        raw = np.array(a, copy=True).reshape(-1)
        buf = torch.full((raw.size + 48,), 0xA5, dtype=torch.uint8, device=dev)
        lead = (-buf.data_ptr()) % 16 + off
        t = buf[lead:lead + raw.size]
        t.copy_(torch.from_numpy(raw).to(dev))
        return buf, lead, t.view(a.shape)

    for y_off, uv_off in ((0, 0), (1, 2), (3, 6), (1, 14)):
        _, _, y = offset(c['y'], y_off)
        _, _, uv = offset(c['uv'], uv_off)
        by, ly, oy = offset(np.full_like(want_y, 0xA5), y_off)
        buv, luv, ouv = offset(np.full_like(want_uv, 0xA5), uv_off)
        ry, ruv = ops.crop_resize_nv12(y, uv, rect, size=size, out=(oy, ouv))
        assert ry.data_ptr() == oy.data_ptr() and ruv.data_ptr() == ouv.data_ptr()
        assert np.array_equal(oy.cpu().numpy(), want_y) and np.array_equal(ouv.cpu().numpy(), want_uv), (y_off, uv_off)
        for buf, lead, t in ((by, ly, oy), (buv, luv, ouv)):
            assert bool((buf[:lead] == 0xA5).all()) and bool((buf[lead + t.numel():] == 0xA5).all()), (y_off, uv_off)


@pytest.mark.parametrize('name,rect,size', [('100x72', (3, 3, 96, 68), (100, 72)), ('100x72', (5, 7, 5, 7), (20, 12)),
                                            ('66x50', (2, 3, 63, 46), (30, 8)), ('64x48', (63, 47, 63, 47), (64, 48))])
def test_nothing_outside_the_crop_influences_the_result(dev, name, rect, size):
    """Every chroma sample outside columns c0 .. c1 and rows r0 .. r1 and every luma pixel outside the rectangle re-randomised: the same bytes."""
    from meshflow_amd import ops
    c = cases.frame(name)
    left, top, right, bottom = rect
    (c0, c1), (r0, r1) = model.axis_range(left, right), model.axis_range(top, bottom)
    rng = np.random.default_rng(77)
    y2 = rng.integers(0, 256, c['y'].shape, dtype=np.uint8)
    uv2 = rng.integers(0, 256, c['uv'].shape, dtype=np.uint8)
    y2[:, top:bottom + 1, left:right + 1] = c['y'][:, top:bottom + 1, left:right + 1]
    uv2[:, r0:r1 + 1, c0:c1 + 1] = c['uv'][:, r0:r1 + 1, c0:c1 + 1]
    assert not np.array_equal(uv2, c['uv']) and not np.array_equal(y2, c['y'])
    want_y, want_uv = cases.want(name, rect, size)
    bounds = torch.tensor(rect, dtype=torch.int32, device=dev)
    for yy, uu in ((c['y'], c['uv']), (y2, uv2)):
        got_y, got_uv = ops.crop_resize_nv12(put(yy, dev), put(uu, dev), rect, size=size)
        dev_y, dev_uv, _ = ops.crop_resize_nv12(put(yy, dev), put(uu, dev), bounds, size=size)
        for g, w in ((got_y, want_y), (dev_y, want_y), (got_uv, want_uv), (dev_uv, want_uv)):
            assert np.array_equal(g.cpu().numpy(), w)


def test_unusable_device_rectangles(dev):
    """Empty, negative, outside the frame: the status rises by exactly 1 per call and accumulates, the sentinel-filled outputs and the planes
    stay untouched, and a usable call afterwards is correct."""
    from meshflow_amd import ops
    name = '66x50'
    c = cases.frame(name)
    W, H = c['W'], c['H']
    y, uv = put(c['y'], dev), put(c['uv'], dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    bad = [(5, 3, 4, 40), (2, 9, 60, 8), (-1, 3, 60, 40), (2, -2, 60, 40), (2, 3, W, 40), (2, 3, 60, H), (W, H, W + 4, H + 4),
           (-2 ** 31, -2 ** 31, 2 ** 31 - 1, 2 ** 31 - 1), (2 ** 31 - 1, 0, -2 ** 31, 5)]
    for size in ((W, H), (92, 74), (30, 8)):
        oy = torch.full((c['n'], size[1], size[0]), 0x5A, dtype=torch.uint8, device=dev)
        ouv = torch.full((c['n'], size[1] // 2, size[0] // 2, 2), 0x5A, dtype=torch.uint8, device=dev)
        before = int(status.item())
        for k, rect in enumerate(bad):
            bounds = torch.tensor(rect, dtype=torch.int32, device=dev)
            _, _, st = ops.crop_resize_nv12(y, uv, bounds, size=size, out=(oy, ouv), status=status)
            assert st is status and int(status.item()) == before + k + 1, (rect, size)
        assert bool((oy == 0x5A).all()) and bool((ouv == 0x5A).all()), size
        rect = (3, 3, 62, 47)
        bounds = torch.tensor(rect, dtype=torch.int32, device=dev)
        ops.crop_resize_nv12(y, uv, bounds, size=size, out=(oy, ouv), status=status)
        assert int(status.item()) == before + len(bad)
        want_y, want_uv = model.crop_resize_clip(c['y'], c['uv'], rect, size)
        assert np.array_equal(oy.cpu().numpy(), want_y) and np.array_equal(ouv.cpu().numpy(), want_uv), size
    _, _, fresh = ops.crop_resize_nv12(y, uv, torch.tensor(bad[0], dtype=torch.int32, device=dev))
    assert int(fresh.item()) == 1                                       # a status of the call's own starts at zero
    assert np.array_equal(y.cpu().numpy(), c['y']) and np.array_equal(uv.cpu().numpy(), c['uv'])


def test_stabilized_nv12_crop(dev):
    """crop=True equals `ops.crop_resize_nv12` of the crop=False result with the returned bounds; crop=False is the call as it was: the warp of
    the clip's table (`ops.warp_nv12`), which is what it returned before it had a crop option."""
    from meshflow_amd import ops, synthetic
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    F, H, W, R, C = 8, 64, 96, 3, 4
    border = (60, 100, 200)
    disp, hom = synthetic.motion(F, R, C, seed=71, jitter_sigma=2.0)
    s = MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, temporal_smoothing_radius=4, optimization_num_iterations=15, device='cuda:0')
    rng = np.random.default_rng(8)
    y = put(rng.integers(0, 256, (F, H, W), dtype=np.uint8), dev)
    uv = put(rng.integers(0, 256, (F, H // 2, W // 2, 2), dtype=np.uint8), dev)
    d_disp = torch.from_numpy(np.ascontiguousarray(disp, dtype=np.float64)).to(dev)
    stab = s._get_stabilized_vertex_displacements(F, [np.zeros((H, W, 3), np.uint8)] * F, s.ADAPTIVE_WEIGHTS_DEFINITION_ORIGINAL, disp, hom)
    table = ops.cell_table(d_disp, torch.from_numpy(np.ascontiguousarray(stab, dtype=np.float64)).to(dev), W, H, R, C)
    parent_y, parent_uv = ops.warp_nv12(y, uv, table, border)
    plain_y, plain_uv, b = s.stabilized_nv12(y, uv, d_disp, hom, border)
    also_y, also_uv, b2 = s.stabilized_nv12(y, uv, d_disp, hom, border, crop=False)
    assert torch.equal(plain_y, parent_y) and torch.equal(plain_uv, parent_uv) and torch.equal(b, table.clip_bounds)
    assert torch.equal(also_y, parent_y) and torch.equal(also_uv, parent_uv) and torch.equal(b2, b)
    rect = tuple(b.tolist())
    assert rect != (0, 0, W - 1, H - 1) and 0 <= rect[0] <= rect[2] < W and 0 <= rect[1] <= rect[3] < H
    for size in (None, (128, 90), (48, 32)):
        got_y, got_uv, gb = s.stabilized_nv12(y, uv, d_disp, hom, border, crop=True, output_size=size)
        want_y, want_uv, st = ops.crop_resize_nv12(plain_y, plain_uv, b, size=size)
        host_y, host_uv = ops.crop_resize_nv12(plain_y, plain_uv, rect, size=size)
        assert int(st.item()) == 0 and torch.equal(gb, b)
        assert torch.equal(got_y, want_y) and torch.equal(got_uv, want_uv) and torch.equal(got_y, host_y) and torch.equal(got_uv, host_uv), size
        my, muv = model.crop_resize_frame(plain_y[3].cpu().numpy(), plain_uv[3].cpu().numpy(), rect, size)
        assert np.array_equal(got_y[3].cpu().numpy(), my) and np.array_equal(got_uv[3].cpu().numpy(), muv), size
    # out= names the cropped pair
    oy = torch.empty((F, 32, 48), dtype=torch.uint8, device=dev)
    ouv = torch.empty((F, 16, 24, 2), dtype=torch.uint8, device=dev)
    r_y, r_uv, _ = s.stabilized_nv12(y, uv, d_disp, hom, border, out=(oy, ouv), crop=True, output_size=(48, 32))
    assert r_y.data_ptr() == oy.data_ptr() and r_uv.data_ptr() == ouv.data_ptr() and torch.equal(oy, got_y) and torch.equal(ouv, got_uv)
    with pytest.raises(ValueError, match='output_size belongs to crop=True'):
        s.stabilized_nv12(y, uv, d_disp, hom, border, output_size=(48, 32))
    with pytest.raises(ValueError):
        s.stabilized_nv12(y, uv, d_disp, hom, border, crop=True, output_size=(47, 32))
    with pytest.raises(ValueError):
        s.stabilized_nv12(y, uv, d_disp, hom, border, crop=True, out=(plain_y, plain_uv), output_size=(48, 32))
