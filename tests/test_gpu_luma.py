"""`ops.luma` against its specification, tests/luma_model.py, bit for bit: every source format in both channel orders on shapes whose pixel
counts leave the kernel's head, 16-pixel runs and tail each empty, partial and full; sources and destinations that start at odd bytes of a
larger buffer, with canaries around the destination; every level of every channel, the 16-bit values where the high byte turns, hashed noise
and P010-style samples with low bits set; and one clip of 2^28 + 32,768 pixels, longer than a launch takes.  The small cases go through views
of byte buffers, so the source is compared with what was uploaded as well."""
import itertools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import luma_model as lm  # noqa: E402

pytestmark = pytest.mark.gpu

# name -> (dtype, channels; 1 = a plane without a channel axis, whether red_first applies)
FORMATS = {'u8c3': (np.uint8, 3, True), 'u8c4': (np.uint8, 4, True), 'u16c3': (np.uint16, 3, True), 'u16c1': (np.uint16, 1, False)}
SHAPES = tuple(itertools.product((1, 3), (1, 2, 5), (1, 3, 4, 5, 15, 16, 17, 61, 64, 67, 253)))
U8_OFFSETS = (0, 1, 2, 3, 5, 8, 15)
U16_SOURCE_OFFSETS = (0, 2, 6, 14)
CANARY, FRONT = 0xA5, 32          # FRONT bytes in front of the destination keep its misalignment what the test asks for


@pytest.fixture(scope='module')
def dev():
    torch = pytest.importorskip('torch')
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def noise(shape, dtype, seed):
    from meshflow_amd import synthetic
    return (synthetic.hash32(np.arange(int(np.prod(shape))), seed) % (np.iinfo(dtype).max + 1)).astype(dtype).reshape(shape)


def frames_of(name, shape, seed):
    dtype, channels, _ = FORMATS[name]
    return noise(shape + ((channels,) if channels > 1 else ()), dtype, seed)


def orders(name):
    return (False, True) if FORMATS[name][2] else (False,)


def device_luma(dev, frames, red_first=False, source_offset=0, dest_offset=0):
    """`ops.luma` of `frames` placed source_offset bytes into one byte buffer, into a view dest_offset bytes past a 16-byte boundary of
    another that is filled with canaries.  Checks the canaries, the untouched source and that `out` came back; returns the result."""
    import torch
    from meshflow_amd import ops
    raw = np.frombuffer(frames.tobytes(), np.uint8)
    total = int(np.prod(frames.shape[:3]))
    d_bytes = torch.zeros(source_offset + raw.size + 16, dtype=torch.uint8, device=dev)
    assert d_bytes.data_ptr() % 16 == 0
    d_bytes[source_offset:source_offset + raw.size] = torch.from_numpy(raw.copy()).to(dev)
    d_src = d_bytes[source_offset:source_offset + raw.size]
    if frames.dtype == np.uint16:
        d_src = d_src.view(torch.uint16)
    d_src = d_src.view(frames.shape)
    assert d_src.is_contiguous() and d_src.data_ptr() % 16 == source_offset % 16
    d_room = torch.full((FRONT + dest_offset + total + FRONT,), CANARY, dtype=torch.uint8, device=dev)
    assert d_room.data_ptr() % 16 == 0
    d_out = d_room[FRONT + dest_offset:FRONT + dest_offset + total].view(frames.shape[:3])
    kw = {'red_first': red_first} if red_first else {}
    got = ops.luma(d_src, out=d_out, **kw)
    assert got is d_out
    room = d_room.cpu().numpy()
    assert (room[:FRONT + dest_offset] == CANARY).all() and (room[FRONT + dest_offset + total:] == CANARY).all(), 'a byte outside the destination changed'
    assert np.array_equal(d_bytes.cpu().numpy()[source_offset:source_offset + raw.size], raw), 'the source changed'
    return room[FRONT + dest_offset:FRONT + dest_offset + total].reshape(frames.shape[:3])


def same(got, want, what):
    assert got.dtype == np.uint8 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (what, len(bad), bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


@pytest.mark.parametrize('name', sorted(FORMATS))
def test_every_shape_equals_the_model(dev, name):
    for k, shape in enumerate(SHAPES):
        frames = frames_of(name, shape, 100 + k)
        for red_first in orders(name):
            same(device_luma(dev, frames, red_first), lm.luma(frames, red_first), (name, shape, red_first))


@pytest.mark.parametrize('name', ['u8c3', 'u8c4'])
def test_misaligned_u8_sources_and_destinations(dev, name):
    """(3, 2, 61) = 366 pixels: a head of up to 15, 21 or 22 runs and a tail; (1, 1, 5): a clip that ends inside its head."""
    for shape in ((3, 2, 61), (1, 1, 5)):
        frames = frames_of(name, shape, 7)
        want = {r: lm.luma(frames, r) for r in (False, True)}
        for k, (s_off, d_off) in enumerate(itertools.product(U8_OFFSETS, U8_OFFSETS)):
            red_first = bool(k & 1)
            same(device_luma(dev, frames, red_first, s_off, d_off), want[red_first], (name, shape, s_off, d_off, red_first))


@pytest.mark.parametrize('name', ['u16c3', 'u16c1'])
def test_misaligned_u16_sources_and_destinations(dev, name):
    for shape in ((3, 2, 61), (1, 1, 5)):
        frames = frames_of(name, shape, 9)
        want = {r: lm.luma(frames, r) for r in orders(name)}
        for k, (s_off, d_off) in enumerate(itertools.product(U16_SOURCE_OFFSETS, U8_OFFSETS)):
            red_first = bool(k & 1) and FORMATS[name][2]
            same(device_luma(dev, frames, red_first, s_off, d_off), want[red_first], (name, shape, s_off, d_off, red_first))


def test_every_level_of_every_channel(dev):
    """Channel c at 0 .. 255 with the other two at 0 and at 255: 3 x 2 x 256 pixels, BGR and BGRA (noise alpha)."""
    px = np.zeros((3, 2, 256, 3), np.uint8)
    for c in range(3):
        for k, other in enumerate((0, 255)):
            px[c, k] = other
            px[c, k, :, c] = np.arange(256)
    bgra = np.concatenate([px, noise((3, 2, 256, 1), np.uint8, 11)], axis=3)
    for red_first in (False, True):
        want = lm.luma(px, red_first)
        same(device_luma(dev, px, red_first), want, ('u8c3 levels', red_first))
        same(device_luma(dev, bgra, red_first), want, ('u8c4 levels', red_first))
    assert lm.luma(px)[:, 0, 255].tolist() == [29, 150, 76]


def test_sixteen_bit_values_where_the_high_byte_turns(dev):
    edge = np.array([0, 255, 256, 32767, 32768, 65535], np.uint16)
    bgr = np.array(list(itertools.product(edge, edge, edge)), np.uint16).reshape(1, 6, 36, 3)
    for red_first in (False, True):
        same(device_luma(dev, bgr, red_first), lm.luma(bgr, red_first), ('u16c3 edges', red_first))
    # each channel over the whole range in steps of 251 and 256 with the others at the edges
    ramp = np.concatenate([np.arange(0, 65536, 251), np.arange(255, 65536, 256), np.arange(0, 65536, 256)]).astype(np.uint16)
    px = np.zeros((3, len(edge), len(ramp), 3), np.uint16)
    for c in range(3):
        px[c] = edge[:, None, None]
        px[c, :, :, c] = ramp
    for red_first in (False, True):
        same(device_luma(dev, px, red_first), lm.luma(px, red_first), ('u16c3 ramps', red_first))
    plane = np.concatenate([edge, ramp]).reshape(1, 1, -1)
    same(device_luma(dev, plane), (plane >> 8).astype(np.uint8), 'u16c1 edges')


def test_p010_samples_with_low_bits_set(dev):
    """10-bit levels in the high bits, the six low bits anything: only the high byte counts."""
    levels = noise((2, 9, 37), np.uint16, 13) & 0xFFC0
    low = noise((2, 9, 37), np.uint16, 14) & 0x3F
    assert low.any()
    got, clean = device_luma(dev, levels | low), device_luma(dev, levels)
    same(got, lm.luma(levels | low), 'p010 with low bits')
    same(got, clean, 'the low bits do not matter')
    same(got, (levels >> 8).astype(np.uint8), 'the high byte')


def test_a_new_tensor_when_no_out_is_given(dev):
    import torch
    from meshflow_amd import ops
    for name in sorted(FORMATS):
        frames = frames_of(name, (2, 5, 67), 17)
        d_src = torch.from_numpy(frames).to(dev)
        for red_first in orders(name):
            got = ops.luma(d_src, red_first)
            assert got.dtype == torch.uint8 and tuple(got.shape) == (2, 5, 67) and got.device == d_src.device and got.is_contiguous()
            same(got.cpu().numpy(), lm.luma(frames, red_first), (name, red_first))
        assert np.array_equal(d_src.cpu().numpy(), frames)


@pytest.mark.parametrize('name', ['u8c3', 'u16c1'])
def test_a_clip_longer_than_one_launch(dev, name):
    """(4, 8192, 8193) = 2^28 + 32,768 pixels: a launch takes 2^28, so the library's stride over the rest runs once.  Noise made on the device;
    the whole result against the same arithmetic in torch, and the model on the first and last pixels and on both sides of the seam."""
    import torch
    from meshflow_amd import ops
    shape = (4, 8192, 8193)
    total = shape[0] * shape[1] * shape[2]
    assert (1 << 28) < total < (1 << 28) + (1 << 16)
    if name == 'u8c3':
        d_src = torch.randint(0, 256, shape + (3,), dtype=torch.uint8, device=dev)
    else:
        d_src = torch.randint(0, 256, (2 * total,), dtype=torch.uint8, device=dev).view(torch.uint16).view(shape)
    d_out = torch.full((total + 64,), CANARY, dtype=torch.uint8, device=dev)
    got = ops.luma(d_src, out=d_out[32:32 + total].view(shape))
    if name == 'u8c3':
        b, g, r = (d_src[..., i].to(torch.int32) for i in range(3))
        want = ((b * 3735 + g * 19235 + r * 9798 + 16384) >> 15).to(torch.uint8)
        del b, g, r
    else:
        want = (d_src.to(torch.int32) >> 8).to(torch.uint8)
    assert torch.equal(got, want)
    assert bool((d_out[:32] == CANARY).all()) and bool((d_out[32 + total:] == CANARY).all())
    flat_src = d_src.view(total, -1)
    for lo, hi in ((0, 4096), ((1 << 28) - 4096, (1 << 28) + 4096), (total - 4096, total)):
        part = flat_src[lo:hi].cpu().numpy()
        part = part.reshape(1, 1, hi - lo, 3) if name == 'u8c3' else part.reshape(1, 1, hi - lo)
        same(got.view(-1)[lo:hi].cpu().numpy().reshape(1, 1, -1), lm.luma(part), (name, lo, hi))


def test_more_runs_than_one_workgroup_takes(dev):
    """(2, 67, 253) = 33,902 pixels: 2,118 runs, nine workgroups of 256 lanes."""
    for name in sorted(FORMATS):
        frames = frames_of(name, (2, 67, 253), 19)
        same(device_luma(dev, frames, FORMATS[name][2], 0, 3), lm.luma(frames, FORMATS[name][2]), name)
