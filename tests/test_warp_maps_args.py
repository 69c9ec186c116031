"""No GPU: the coordinate-map calls in the header, the ctypes table and the built library; `ops.maps_to_grid` on CPU tensors against
`torch.nn.functional.grid_sample`; and the argument refusals of `ops.warp_maps` that are decided before the library is called."""
import os
import sys
import types

import numpy as np
import pytest

torch = pytest.importorskip('torch')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import second_opinion  # noqa: E402


def test_library_exports_the_maps_calls():
    from meshflow_amd import _lib
    for name, nargs in (('mf_warp_maps_f32', 11), ('mf_warp_maps_bounds_f32', 12)):
        assert name in _lib.SIGNATURES, name
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == nargs
        assert hasattr(_lib.lib, name), name
    assert _lib.lib.mf_abi_version() == 1


def test_refusals_of_the_c_calls_need_no_gpu():
    """Null pointers, bad sizes and frame ranges outside the table are refused before anything touches a device."""
    import ctypes
    from meshflow_amd import _lib
    L = _lib.lib
    buf = (ctypes.c_uint8 * 128)()
    base = (ctypes.addressof(buf) + 15) & ~15
    p = ctypes.c_void_p(base)
    E = _lib.MF_ERR_INVALID_ARG
    assert L.mf_warp_maps_f32(None, p, 4, 64, 64, 4, 4, 0, 4, p, None) == E
    assert L.mf_warp_maps_f32(p, None, 4, 64, 64, 4, 4, 0, 4, p, None) == E
    assert L.mf_warp_maps_f32(p, p, 4, 64, 64, 4, 4, 0, 4, None, None) == E
    assert L.mf_warp_maps_bounds_f32(p, p, 4, 64, 64, 4, 4, 0, 4, p, None, None) == E
    assert L.mf_warp_maps_f32(p, p, 0, 64, 64, 4, 4, 0, 0, p, None) == E
    for first, count in ((-1, 1), (0, -1), (0, 5), (4, 1), (5, 0), (2, 3), (2**31 - 1, 2**31 - 1)):
        assert L.mf_warp_maps_f32(p, p, 4, 64, 64, 4, 4, first, count, p, None) == E, (first, count)
        assert b'first' in L.mf_last_error()
    assert L.mf_warp_maps_f32(p, ctypes.c_void_p(base + 4), 4, 64, 64, 4, 4, 0, 1, p, None) == E
    assert b'aligned' in L.mf_last_error()
    # count == 0 is a no-op, at either end of the table, with or without a map pointer
    assert L.mf_warp_maps_f32(p, p, 4, 64, 64, 4, 4, 0, 0, p, None) == _lib.MF_OK
    assert L.mf_warp_maps_f32(p, None, 4, 64, 64, 4, 4, 4, 0, p, None) == _lib.MF_OK
    assert L.mf_warp_maps_bounds_f32(p, None, 4, 64, 64, 4, 4, 2, 0, p, p, None) == _lib.MF_OK


def _identity_maps(H, W, dtype=torch.float64):
    ys, xs = torch.meshgrid(torch.arange(H, dtype=dtype), torch.arange(W, dtype=dtype), indexing='ij')
    return torch.stack([xs, ys], dim=-1)[None]


def test_maps_to_grid_corners_and_unowned():
    from meshflow_amd import ops
    H, W = 5, 9
    m = _identity_maps(H, W, torch.float32)
    g = ops.maps_to_grid(m)
    assert g.dtype == torch.float32 and g.shape == (1, H, W, 2)
    assert g[0, 0, 0].tolist() == [-1.0, -1.0] and g[0, H - 1, W - 1].tolist() == [1.0, 1.0]
    h = ops.maps_to_grid(m, align_corners=False)
    assert h.dtype == torch.float32
    want = torch.stack([(2 * m[..., 0] + 1) / W - 1, (2 * m[..., 1] + 1) / H - 1], dim=-1)
    assert torch.allclose(h, want, rtol=0, atol=1e-6)
    assert abs(h[0, 0, 0, 0].item() - (1.0 / W - 1)) < 1e-6 and abs(h[0, H - 1, W - 1, 1].item() - (1 - 1.0 / H)) < 1e-6
    unowned = torch.tensor([[[[W + 1.0, H + 1.0]]]], dtype=torch.float32).expand(1, H, W, 2)
    for ac in (True, False):
        assert bool((ops.maps_to_grid(unowned, align_corners=ac) > 1).all())
    with pytest.raises(ValueError):
        ops.maps_to_grid(torch.zeros(1, 4, 4, 3))
    with pytest.raises(ValueError):
        ops.maps_to_grid(torch.zeros(1, 4, 4, 2, dtype=torch.int32))


@pytest.mark.parametrize('align_corners', [True, False])
def test_grid_sample_through_identity_and_shift_maps(align_corners):
    from meshflow_amd import ops
    H, W = 13, 18
    frame = torch.from_numpy(np.random.default_rng(3).random((1, 2, H, W)))
    m = _identity_maps(H, W)
    got = torch.nn.functional.grid_sample(frame, ops.maps_to_grid(m, align_corners), mode='bilinear', padding_mode='zeros', align_corners=align_corners)
    assert float((got - frame).abs().max()) <= second_opinion.EXACT
    for dx, dy in ((3, -2), (-5, 4)):
        # output (x, y) samples (x - dx, y - dy): the frame moves by (dx, dy), zeros where the source lies outside
        shifted = m - torch.tensor([float(dx), float(dy)], dtype=torch.float64)
        got = torch.nn.functional.grid_sample(frame, ops.maps_to_grid(shifted, align_corners), mode='bilinear', padding_mode='zeros',
                                              align_corners=align_corners)
        want = torch.zeros_like(frame)
        ys, yd = (slice(0, H - dy), slice(dy, H)) if dy >= 0 else (slice(-dy, H), slice(0, H + dy))
        xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
        want[..., yd, xd] = frame[..., ys, xs]
        assert float((got - want).abs().max()) <= second_opinion.EXACT
        assert float(want.abs().sum()) > 0 and bool((want == 0).any())
    # unowned pixels stay empty
    far = torch.full((1, H, W, 2), 0.0, dtype=torch.float64) + torch.tensor([W + 1.0, H + 1.0], dtype=torch.float64)
    got = torch.nn.functional.grid_sample(frame, ops.maps_to_grid(far, align_corners), mode='bilinear', padding_mode='zeros', align_corners=align_corners)
    assert float(got.abs().max()) == 0.0


def test_warp_maps_refuses_bad_ranges_and_out_before_the_library():
    """The range and `out` checks come first: a stand-in table without device memory is enough to reach them."""
    from meshflow_amd import ops
    table = types.SimpleNamespace(n=4, W=32, H=16, R=2, C=2, device=torch.device('cpu'), buf=None, crop=None)
    for first, count in ((-1, 1), (5, None), (0, 5), (3, 2), (0, -1), (1.5, 1), (0, 2.0), (True, 1)):
        with pytest.raises(ValueError):
            ops.warp_maps(table, first=first, count=count)
    good = (2, 16, 32, 2)
    for out in (torch.zeros(good, dtype=torch.float64), torch.zeros((2, 16, 32, 3)), torch.zeros((3, 16, 32, 2)),
                torch.zeros((2, 16, 32, 4))[..., ::2], np.zeros(good, dtype=np.float32)):
        with pytest.raises(ValueError):
            ops.warp_maps(table, first=1, count=2, out=out)
    with pytest.raises(ValueError):
        ops.warp_maps(table, first=0, count=2, out=torch.zeros(good), bounds=torch.zeros(3, dtype=torch.int32))
