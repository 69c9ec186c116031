"""CPU: the output_size argument of MeshFlowStabilizer.stabilize_clip / _crop_frames and the size of ops.crop_resize are checked before
any device work -- two positive ints up to 32,767 in cv2's (width, height) order, and stabilize_clip only with crop=True."""
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

BAD = [(0, 5), (5, 0), (-1, 5), (32768, 10), (10, 32768), (5.0, 5), (5, 2.5), (True, 5), (5,), (5, 5, 5), 'ab', 7]


def test_check_output_size():
    from meshflow_amd import ops
    assert ops.check_output_size((1920, 1080)) == (1920, 1080)
    assert ops.check_output_size([1, 32767]) == (1, 32767)
    assert ops.check_output_size((np.int64(3), np.int32(4))) == (3, 4)
    for bad in BAD:
        with pytest.raises(ValueError):
            ops.check_output_size(bad)


def test_stabilizer_refuses_before_device_work():
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    s = MeshFlowStabilizer(mesh_row_count=2, mesh_col_count=2, device='cuda:0')
    F, H, W = 3, 8, 10
    frames = [np.zeros((H, W, 3), np.uint8)] * F
    disp = np.zeros((F, 3, 3, 2))
    hom = np.tile(np.eye(3), (F, 1, 1))
    with pytest.raises(ValueError, match='crop=True'):
        s.stabilize_clip(frames, disp, hom, output_size=(4, 4))
    for bad in BAD:
        with pytest.raises(ValueError):
            s.stabilize_clip(frames, disp, hom, crop=True, output_size=bad)
        with pytest.raises(ValueError):
            s._crop_frames(frames, (0, 0, 5, 5), output_size=bad)
