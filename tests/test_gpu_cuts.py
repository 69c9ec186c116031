"""`ops.frame_signatures` and `ops.cut_distances` against tests/cuts_model.py, bit for bit: every shape at which the kernel takes another
path -- one pixel, frames narrower than the tiles, odd widths that move every row against the 16-byte grid, rows of several hundred blocks,
tiles cut into several strips, more frames than a tile has pixels --, content that lands in one counter (constants at the bin edges, one flat
tile) as well as noise, a source that starts at any byte, and an output that was full of something else."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuts_model as cm  # noqa: E402
import luma_clip  # noqa: E402
from tracker_clip import same_bits  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 5, 3), (2, 7, 9), (2, 96, 128), (2, 97, 131), (1, 8, 4099), (1, 4099, 8), (70, 8, 8)]
CONSTANTS = (0, 255, 15, 16, 239, 240)                                  # the bin edges
FILL = 0x7f7f7f7f


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def noise(shape, seed):
    return luma_clip._noise(shape, 256, seed).astype(np.uint8)


def one_flat_tile(shape, seed):
    """Noise with tile (1, 2) of every frame constant."""
    stack = noise(shape, seed)
    rows, cols = cm.tile_edges(shape[1]), cm.tile_edges(shape[2])
    stack[:, rows[1]:rows[2], cols[2]:cols[3]] = 0x9c
    return stack


def signatures_at(stack, dev, offset):
    """`ops.frame_signatures` of the stack placed `offset` bytes into a larger buffer."""
    import torch
    from meshflow_amd import ops
    room = torch.zeros(stack.size + 64, dtype=torch.uint8, device=dev)
    assert room.data_ptr() % 16 == 0
    held = room[offset:offset + stack.size].view(stack.shape)
    held.copy_(torch.from_numpy(stack).to(dev))
    assert held.data_ptr() % 16 == offset % 16 and held.is_contiguous()
    return ops.frame_signatures(held)


@pytest.mark.parametrize('shape', SHAPES)
def test_signatures_equal_the_model(dev, shape):
    import torch
    stacks = [('noise', noise(shape, 41)), ('one flat tile', one_flat_tile(shape, 42))] + [(f'constant {v}', np.full(shape, v, np.uint8)) for v in CONSTANTS]
    for what, stack in stacks:
        want = cm.signatures(stack)
        for offset in ((0, 1, 2, 3) if what in ('noise', 'constant 255') else (0,)):
            got = signatures_at(stack, dev, offset)
            assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (shape[0], 256)
            same_bits(got.cpu().numpy(), want, (shape, what, offset))
            assert int(got.sum().item()) == stack.size


@pytest.mark.parametrize('shape', [(3, 5, 3), (2, 97, 131), (1, 8, 4099)])
def test_the_output_is_overwritten(dev, shape):
    """The C call on a d_sig full of 0x7f7f7f7f, twice: the same bytes as the model's both times."""
    import ctypes
    import torch
    from meshflow_amd import _lib
    n, H, W = shape
    stack = noise(shape, 43)
    d_luma = torch.from_numpy(stack).to(dev)
    sig = torch.full((n + 1, 256), FILL, dtype=torch.int32, device=dev)
    for _ in range(2):
        _lib.check(_lib.lib.mf_frame_signature_u8(ctypes.c_void_p(d_luma.data_ptr()), n, W, H, ctypes.c_void_p(sig.data_ptr()),
                                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
        got = sig.cpu().numpy()
        same_bits(got[:n], cm.signatures(stack), shape)
        assert (got[n] == FILL).all()                                   # (and nothing behind the n signatures is touched)


def test_distances_equal_the_model(dev):
    import torch
    from meshflow_amd import ops
    stack = np.concatenate([noise((3, 97, 131), 44), noise((2, 97, 131), 45) >> 2, np.zeros((1, 97, 131), np.uint8), np.full((1, 97, 131), 255, np.uint8)])
    sigs = cm.signatures(stack)
    d_sig = ops.frame_signatures(torch.from_numpy(stack).to(dev))
    got = ops.cut_distances(d_sig)
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == (7,)
    same_bits(got.cpu().numpy(), cm.distances(sigs), 'no d_prev')
    assert int(got[0].item()) == 0 and int(got[6].item()) == 2 * 97 * 131         # black to white: the extreme
    prev = cm.signature(noise((97, 131), 46))
    same_bits(ops.cut_distances(d_sig, torch.from_numpy(prev).to(dev)).cpu().numpy(), cm.distances(sigs, prev), 'd_prev')
    # one signature: 0 without d_prev, the distance from it with one -- the extreme from a white frame to the black one
    one = d_sig[5:6]
    assert ops.cut_distances(one).cpu().numpy().tolist() == [0]
    assert ops.cut_distances(one, d_sig[6]).cpu().numpy().tolist() == [2 * 97 * 131]
    same_bits(ops.cut_distances(d_sig[2:3], d_sig[1]).cpu().numpy(), cm.distances(sigs[2:3], sigs[1]), 'n = 1')
    # the output is overwritten
    filled = torch.full((7,), FILL, dtype=torch.int32, device=dev)
    import ctypes
    from meshflow_amd import _lib
    _lib.check(_lib.lib.mf_cut_distance_i32(None, ctypes.c_void_p(d_sig.data_ptr()), 7, ctypes.c_void_p(filled.data_ptr()),
                                            ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    same_bits(filled.cpu().numpy(), cm.distances(sigs), 'overwritten')


def test_find_cuts_equals_the_model(dev):
    import torch
    from meshflow_amd import ops
    stack = np.concatenate([noise((3, 40, 52), 47) >> 1, 128 + (noise((4, 40, 52), 48) >> 1)])
    d_luma = torch.from_numpy(stack).to(dev)
    for threshold in (0.30, 0.0, 1.0, 0.02):
        want_cuts, want_dist, want_sig = cm.find_cuts(stack, threshold)
        cuts, dist, sig = ops.find_cuts(d_luma, threshold)
        assert cuts == want_cuts and isinstance(dist, np.ndarray), threshold
        same_bits(dist, want_dist, threshold)
        assert sig.is_cuda and sig.dtype == torch.int32
        same_bits(sig.cpu().numpy(), want_sig, threshold)
    assert ops.find_cuts(d_luma)[0] == [3]
    # in blocks, the last signature carried over: the cut at the head of a block is found from d_prev
    _, _, carried = ops.find_cuts(d_luma[:3])
    cuts, dist, _ = ops.find_cuts(d_luma[3:], d_prev=carried)
    assert cuts == [0] and dist.tolist() == cm.distances(cm.signatures(stack))[3:].tolist()
    for bad, match in ((d_luma[:, :, ::2], 'contiguous'), (d_luma[0], r'shape \(n, H, W\)'), (d_luma.to(torch.int8), 'dtype'), (d_luma[:0], 'n >= 1')):
        with pytest.raises(ValueError, match=match):
            ops.frame_signatures(bad)
    d_sig = ops.frame_signatures(d_luma)
    for bad, prev, match in ((d_sig[:, :255].contiguous(), None, r'shape \(n, 256\)'), (d_sig, d_sig[:2], r'd_prev must have shape \(256,\)'),
                             (d_sig, d_sig[0].cpu(), 'd_prev must be a CUDA/HIP'), (d_sig.long(), None, 'dtype')):
        with pytest.raises(ValueError, match=match):
            ops.cut_distances(bad, prev)
