"""-m gpu: one packed 4:2:2 clip end to end, as a capture card delivers it -- ten 128 x 96 UYVY frames (tests/online_clips.py's grey clip as
luma, seeded chroma) through `estimate_motion` on the unpacked luma and `MeshFlowStabilizer.stabilized_packed_422`.  The output's luma bytes
are `stabilize_resident`'s uncropped grey warp of that luma, its chroma is tests/nv16_model.py at `stabilization_maps`, and the clip
rectangle is the grey call's.  Byte for byte."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nv16_model  # noqa: E402
import online_clips  # noqa: E402
import tracker_clip  # noqa: E402

ORDER = 'uyvy'
BORDER_UV = (203, 77)


def test_packed_clip_end_to_end():
    from meshflow_amd import ops
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    dev = torch.device('cuda:0')
    luma = online_clips.grey_clip()
    F, H, W = luma.shape
    assert (F, H, W) == (10, 96, 128)
    uv = np.random.default_rng(422).integers(0, 256, (F, H, W // 2, 2), dtype=np.uint8)
    packed_np = nv16_model.pack(luma, uv, ORDER)
    d_packed = torch.from_numpy(packed_np).to(dev)
    s = tracker_clip.stabilizer(dev)
    d_y = ops.unpack_422(d_packed, ORDER)[0]                            # the plane the tracker takes
    assert np.array_equal(d_y.cpu().numpy(), luma)
    d_disp, hom = s.estimate_motion(d_y, outliers='device', fit='device', max_per_subframe=tracker_clip.MAX_PER)
    # the grey call: the warp of the luma alone, uncropped, and its rectangle; its border byte is color_outside_image_area_bgr[0]
    grey, grey_bounds, _ = s.stabilize_resident(d_y, d_disp, hom)
    border = (s.color_outside_image_area_bgr[0],) + BORDER_UV
    out, bounds = s.stabilized_packed_422(d_packed, d_disp, hom, order=ORDER, border_yuv=border)
    maps, maps_bounds = s.stabilization_maps(d_disp, hom, W, H)
    torch.cuda.synchronize()
    assert out.dtype == torch.uint8 and tuple(out.shape) == (F, H, W, 2)
    got_y, got_uv = nv16_model.unpack(out.cpu().numpy(), ORDER)
    assert np.array_equal(got_y, grey.cpu().numpy())
    m = maps.cpu().numpy()
    cmx, cmy = nv16_model.chroma_maps(m[..., 0], m[..., 1])
    want_uv = np.stack([nv16_model.remap_chroma(uv[f], cmx[f], cmy[f], BORDER_UV) for f in range(F)])
    assert np.array_equal(got_uv, want_uv), (int((got_uv != want_uv).sum()), np.argwhere(got_uv != want_uv)[:5].tolist())
    assert not np.array_equal(want_uv, uv) and (want_uv == np.asarray(BORDER_UV, np.uint8)).all(axis=-1).any()      # the clip moved
    assert bounds.dtype == torch.int32 and torch.equal(bounds, grey_bounds) and torch.equal(bounds, maps_bounds)
    assert tuple(bounds.tolist()) != (0, 0, W - 1, H - 1)
    assert np.array_equal(d_packed.cpu().numpy(), packed_np)
    # out=, and the NV16 call on the unpacked pair gives the same planes
    d_uv = torch.from_numpy(uv).to(dev)
    o_y, o_uv, b2 = s.stabilized_nv16(d_y, d_uv, d_disp, hom, border_yuv=border)
    filled = torch.empty_like(d_packed)
    r, _ = s.stabilized_packed_422(d_packed, d_disp, hom, ORDER, border, out=filled)
    assert r.data_ptr() == filled.data_ptr() and torch.equal(filled, out) and torch.equal(ops.pack_422(o_y, o_uv, ORDER), out)
    assert torch.equal(b2, bounds)
    with pytest.raises(ValueError, match='order'):
        s.stabilized_packed_422(d_packed, d_disp, hom, order='yvyu')
    with pytest.raises(TypeError):
        s.stabilized_packed_422(d_packed, d_disp, hom, output_size=(64, 48))       # no crop-resize of 4:2:2 clips
