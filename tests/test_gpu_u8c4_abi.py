"""-m gpu: the five u8c4 entries of the C ABI answer every tuple of test_gpu_abi_misuse.py's argument grids (and the crop-resize-to grid of
output sizes, null pointers, aliasing) with the u8c3 entry's status, and write nothing when they refuse; `ops` refuses what it should
(wrong dtype, five channels, a mismatched `out`, a non-contiguous stack) before anything is launched."""
import ctypes
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def test_scalar_grids_answer_like_u8c3(dev):
    from meshflow_amd import _lib
    L = _lib.lib
    a, b, c = (torch.zeros(64 << 20, dtype=torch.uint8, device=dev) for _ in range(3))
    p, q, r = a.data_ptr(), b.data_ptr(), c.data_ptr()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    b3 = (ctypes.c_uint8 * 3)(1, 2, 3)
    b4 = (ctypes.c_uint8 * 4)(1, 2, 3, 4)
    twins = twins_ok = 0

    def twin(name3, name4, args3, args4):
        nonlocal twins, twins_ok
        rc3 = getattr(L, name3)(*args3)
        rc4 = getattr(L, name4)(*args4)
        twins += 1
        twins_ok += rc4 == 0
        assert rc4 == rc3, (name4, args4, rc4, rc3)
        if rc4 != 0:
            assert L.mf_last_error()

    for n, W, H, R, C in itertools.product((-1, 0, 1), (-1, 0, 1, 2, 8, 32768), (-1, 1, 2, 8, 32768), (-1, 0, 1, 65), (0, 1, 65)):
        if W > 0 and H > 0 and W * H * 3 * max(n, 1) > (32 << 20):
            continue
        twin('mf_warp_u8c3', 'mf_warp_u8c4', (p, q, r, n, W, H, R, C, b3, r, st), (p, q, r, n, W, H, R, C, b4, r, st))
        twin('mf_warp_bounds_u8c3', 'mf_warp_bounds_u8c4', (p, q, r, n, W, H, R, C, b3, r, r, st), (p, q, r, n, W, H, R, C, b4, r, r, st))
        if n <= 0 or R <= 0 or C <= 0 or W < 2 or H < 2 or R > 64 or C > 64 or W > 32767 or H > 32767:   # (only refusals: no cell table)
            twin('mf_warp_clip_u8c3', 'mf_warp_clip_u8c4', (p, q, p, p, n, W, H, R, C, b3, r, r, r, r, 0, None, st),
                 (p, q, p, p, n, W, H, R, C, b4, r, r, r, r, 0, None, st))
    for n, W, H in itertools.product((-1, 0, 1), (-1, 0, 1, 5, 32768), (-1, 0, 1, 5, 32768)):
        for rect in ((0, 0, 0, 0), (-1, 0, 3, 3), (2, 2, 1, 1), (0, 0, W, H), (0, 0, max(W, 1) - 1, max(H, 1) - 1), (2147483647, 0, 2147483647, 0)):
            if W > 0 and H > 0 and W * H * 3 > (32 << 20):
                continue
            twin('mf_crop_resize_u8c3', 'mf_crop_resize_u8c4', (p, q, n, W, H, *rect, r, st), (p, q, n, W, H, *rect, r, st))
            for oW, oH in ((-1, 5), (0, 1), (1, 0), (5, 32768), (32768, 5), (7, 3)):
                twin('mf_crop_resize_to_u8c3', 'mf_crop_resize_to_u8c4', (p, q, n, W, H, *rect, oW, oH, r, st),
                     (p, q, n, W, H, *rect, oW, oH, r, st))
    torch.cuda.synchronize()
    assert twins > 2000 and 0 < twins_ok < twins
    assert int(torch.arange(8, device=dev).sum().item()) == 28      # the device still answers


def test_refusals_write_nothing(dev):
    from meshflow_amd import _lib, ops
    L = _lib.lib
    F, H, W, R, C = 2, 64, 64, 2, 2
    disp = torch.zeros((F, R + 1, C + 1, 2), dtype=torch.float64, device=dev)
    table = ops.cell_table(disp, disp, W, H, R, C)
    fr = torch.zeros((F, H, W, 4), dtype=torch.uint8, device=dev)
    out = torch.full((F, H, W, 4), 0xA5, dtype=torch.uint8, device=dev)
    crop = torch.full((F, 4), -7, dtype=torch.int32, device=dev)
    bounds = torch.full((4,), -7, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    work = torch.empty(L.mf_crop_resize_workspace_bytes(W, H), dtype=torch.uint8, device=dev)
    p = lambda t: t.data_ptr()              # noqa: E731
    b4 = (ctypes.c_uint8 * 4)(1, 2, 3, 4)
    t = table.buf
    calls = [
        lambda: L.mf_warp_u8c4(None, p(out), p(t), F, W, H, R, C, b4, p(crop), None),
        lambda: L.mf_warp_u8c4(p(fr), p(out), p(t), F, W, H, R, C, None, p(crop), None),
        lambda: L.mf_warp_u8c4(p(fr), p(fr), p(t), F, W, H, R, C, b4, p(crop), None),
        lambda: L.mf_warp_u8c4(p(fr), p(out), p(t), F, W, H, 65, C, b4, p(crop), None),
        lambda: L.mf_warp_u8c4(p(fr), p(out), p(t), F, 1, H, R, C, b4, p(crop), None),
        lambda: L.mf_warp_bounds_u8c4(p(fr), p(out), p(t), F, W, H, R, C, b4, p(crop), None, None),
        lambda: L.mf_warp_bounds_u8c4(p(fr), p(out), p(t), 0, W, H, R, C, b4, p(crop), p(bounds), None),
        lambda: L.mf_warp_clip_u8c4(p(fr), p(out), p(disp), p(disp), F, W, H, R, C, b4, p(t), p(crop), p(bounds), None, 0, None, None),
        lambda: L.mf_warp_clip_u8c4(p(fr), p(fr), p(disp), p(disp), F, W, H, R, C, b4, p(t), p(crop), p(bounds), p(status), 0, None, None),
        lambda: L.mf_warp_clip_u8c4(p(fr), p(out), p(disp), p(disp), F, W, H, R, 65, b4, p(t), p(crop), p(bounds), p(status), 3, None, None),
        lambda: L.mf_warp_clip_u8c4(p(fr), p(out), p(disp), p(disp), F, 40000, H, R, C, b4, p(t), p(crop), p(bounds), p(status), 0, None, None),
        lambda: L.mf_crop_resize_u8c4(p(fr), p(out), F, W, H, 5, 0, 4, 7, p(work), None),
        lambda: L.mf_crop_resize_u8c4(p(fr), p(out), F, W, H, 0, 0, W, H - 1, p(work), None),
        lambda: L.mf_crop_resize_u8c4(p(fr), p(fr), F, W, H, 0, 0, 7, 7, p(work), None),
        lambda: L.mf_crop_resize_u8c4(p(fr), p(out), F, W, H, 0, 0, 7, 7, None, None),
        lambda: L.mf_crop_resize_to_u8c4(p(fr), p(out), F, W, H, 0, 0, 7, 7, 0, 5, p(work), None),
        lambda: L.mf_crop_resize_to_u8c4(p(fr), p(out), F, W, H, 0, 0, 7, 7, 5, 32768, p(work), None),
        lambda: L.mf_crop_resize_to_u8c4(p(fr), p(out), F, W, H, 3, 0, 2, 7, 5, 5, p(work), None),
        lambda: L.mf_crop_resize_to_u8c4(None, p(out), F, W, H, 0, 0, 7, 7, 5, 5, p(work), None),
        lambda: L.mf_crop_resize_to_u8c4(p(fr), p(out), -1, W, H, 0, 0, 7, 7, 5, 5, p(work), None),
    ]
    for call in calls:
        assert call() == -1, L.mf_last_error()
        assert L.mf_last_error()
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and bool((crop == -7).all()) and bool((bounds == -7).all()) and int(status.item()) == 0


def test_ops_refusals(dev):
    from meshflow_amd import ops
    F, H, W, R, C = 2, 16, 32, 1, 1
    disp = torch.zeros((F, R + 1, C + 1, 2), dtype=torch.float64, device=dev)
    table = ops.cell_table(disp, disp, W, H, R, C)
    for dt in (torch.uint16, torch.float32, torch.int32):
        bad = torch.zeros((F, H, W, 4), dtype=dt, device=dev)
        for fn in (lambda: ops.warp(bad, table), lambda: ops.warp_clip(bad, disp, disp, table),
                   lambda: ops.crop_resize(bad, (0, 0, 7, 7)), lambda: ops.crop_resize(bad, (0, 0, 7, 7), size=(4, 4))):
            with pytest.raises(ValueError, match=str(dt).split('.')[-1]):
                fn()
    with pytest.raises(ValueError):
        ops.warp(torch.zeros((F, H, W, 5), dtype=torch.uint8, device=dev), table)
    with pytest.raises(ValueError):
        ops.crop_resize(torch.zeros((F, H, W, 5), dtype=torch.uint8, device=dev), (0, 0, 7, 7))
    fr = torch.zeros((F, H, W, 4), dtype=torch.uint8, device=dev)
    sentinel = torch.full((F, H, W, 3), 0x5A, dtype=torch.uint8, device=dev)
    for fn in (lambda: ops.warp(fr, table, out=sentinel), lambda: ops.crop_resize(fr, (0, 0, 7, 7), out=sentinel),
               lambda: ops.crop_resize(fr, (0, 0, 7, 7), size=(8, 8), out=torch.empty((F, 8, 8, 3), dtype=torch.uint8, device=dev)),
               lambda: ops.warp(fr, table, out=torch.empty((F, H, W, 4), dtype=torch.uint16, device=dev))):
        with pytest.raises(ValueError):
            fn()
    strided = torch.zeros((F, H, 2 * W, 4), dtype=torch.uint8, device=dev)[:, :, ::2]
    assert strided.shape == (F, H, W, 4) and not strided.is_contiguous()
    for fn in (lambda: ops.warp(strided, table), lambda: ops.crop_resize(strided, (0, 0, 7, 7))):
        with pytest.raises(ValueError, match='contiguous'):
            fn()
    torch.cuda.synchronize()
    assert bool((sentinel == 0x5A).all())
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    s = MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, temporal_smoothing_radius=1, optimization_num_iterations=0, device='cuda:0')
    with pytest.raises(ValueError, match='uint16'):
        s.stabilize_resident(torch.zeros((F, H, W, 4), dtype=torch.uint16, device=dev), disp, np.tile(np.eye(3), (F, 1, 1)))
    assert ops.pixel_format(torch.uint8, (F, H, W, 4)).channels == 4
