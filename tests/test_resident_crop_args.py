"""CPU: the argument rules of `stabilize_resident(crop=True, output_size=..., cropped_out=...)` that need no GPU, and the clip that
tests/test_gpu_resident_crop.py uses for an unusable rectangle: by the CPU oracle its clip-level rectangle is empty and none of its mesh
cells is degenerate."""
import inspect

import numpy as np
import pytest

torch = pytest.importorskip('torch')


def empty_rectangle_clip(F=12, H=64, W=96, R=4, C=4):
    """(frames, displacements, homographies): every vertex of even frames 70 px right of, of odd frames 70 px left of its place -- the
    displacement recipe of the empty-rectangle case of tests/test_gpu_capi_host.py moved in front of the smoothing.  The smoothed paths lie
    in between, so consecutive frames are warped more than 30 px in opposite directions: the largest left bound passes the smallest right
    bound.  Pure translations: every cell keeps its homography."""
    from meshflow_amd import synthetic
    disp = np.zeros((F, R + 1, C + 1, 2))
    disp[0::2, ..., 0] = 70.0
    disp[1::2, ..., 0] = -70.0
    return synthetic.frames_numpy(F, H, W, seed=1), disp, np.tile(np.identity(3), (F, 1, 1))


def test_the_empty_rectangle_clip_is_empty_and_not_degenerate_by_the_oracle():
    from oracle import clib, meshflow_oracle as mo
    F, H, W, R, C = 12, 64, 96, 4, 4
    frames, disp, hom = empty_rectangle_clip(F, H, W, R, C)
    stab = mo.stabilized_vertex_displacements(W, H, 0, disp, hom, 3, 10)       # radius 3, 10 iterations: what the GPU test's stabilizer runs
    _, crop, bad = clib.warp_clip(frames, R, C, disp, stab, use_bbox=True)
    assert bad == 0
    left, top, right, bottom = int(crop[:, 0].max()), int(crop[:, 1].max()), int(crop[:, 2].min()), int(crop[:, 3].min())
    assert left > right and top <= bottom, (left, top, right, bottom)
    assert 0 <= left < W and 0 <= right < W                                     # empty, not out of the frame


def test_argument_rules():
    from meshflow_amd import DegenerateMeshError, MeshFlowStabilizer, UnusableCropError
    s = MeshFlowStabilizer(mesh_row_count=4, mesh_col_count=4)
    frames, disp = torch.zeros((2, 8, 8, 3), dtype=torch.uint8), torch.zeros((2, 5, 5, 2), dtype=torch.float64)
    hom = np.tile(np.identity(3), (2, 1, 1))
    with pytest.raises(ValueError, match='output_size needs crop=True: it is the size of the cropped frames'):
        s.stabilize_resident(frames, disp, hom, output_size=(8, 8))
    with pytest.raises(ValueError, match='output_size needs crop=True'):
        s.stabilize_resident(frames, disp, hom, crop=False, output_size=(8, 8))
    with pytest.raises(ValueError, match='cropped_out needs crop=True'):
        s.stabilize_resident(frames, disp, hom, cropped_out=torch.zeros_like(frames))
    for size in ((0, 5), (5, 0), (32768, 5), (5.0, 5), (5,), 'ab', (True, 5), (5, 5, 5)):
        with pytest.raises(ValueError, match='output_size'):
            s.stabilize_resident(frames, disp, hom, crop=True, output_size=size)
    p = inspect.signature(s.stabilize_resident).parameters
    assert p['crop'].default is False and p['output_size'].default is None and p['cropped_out'].default is None
    e = UnusableCropError(7)
    assert isinstance(e, ValueError) and not isinstance(e, DegenerateMeshError) and e.clip_serial == 7 and '#7' in str(e)


def test_ops_refuses_without_a_device_tensor():
    from meshflow_amd import ops
    frames = torch.zeros((2, 8, 8, 3), dtype=torch.uint8)
    with pytest.raises(ValueError):
        ops.crop_resize_resident(frames, torch.zeros(4, dtype=torch.int32))
    assert ops.check_output_size((3, 4)) == (3, 4)
