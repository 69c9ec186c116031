"""-m gpu: packed 4:2:2 against the NV16 pair -- `ops.unpack_422` and `ops.pack_422` (pack422.hip) in both byte orders, byte for byte
tests/nv16_model.py's slicing.

The shapes walk the kernels' cut of the word stream: one word, a head alone, head and tail without a full run (45 words), and clips of
several runs with and without a tail.  The source and the destinations are views into sentinel-filled buffers at byte offsets from a 16-byte
boundary chosen so that every choice of access width occurs: everything aligned (dwordx4 loads, 16-byte stores), only the packed side
misaligned (dword loads / a cut that leaves the planes off), `y` and `uv` out of phase with each other (2-byte accesses), and planes in phase
but off the boundary, with and without the packed side in step (a head in front of wide runs).  Around every output not a byte changes."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import nv16_model  # noqa: E402

SHAPES = [(1, 1, 2), (1, 1, 6), (3, 5, 6), (2, 7, 34), (1, 16, 64), (2, 33, 130)]         # (n, H, W)
# (packed, y, uv) byte offsets past a 16-byte boundary: packed 4-byte aligned, the planes 2-byte aligned
LAYOUTS = [(0, 0, 0),                       # all aligned: the wide path
           (4, 0, 0), (12, 0, 0),           # only the packed side misaligned
           (0, 0, 2), (0, 6, 14), (4, 2, 10),   # y and uv out of phase
           (12, 6, 6),                      # in phase, off the boundary: unpack's head of 5 words brings all three to a boundary
           (4, 10, 10),                     # ... and pack's head of 3 words does
           (8, 2, 2)]                       # in phase, the packed side never in step with them
GUARD = 48


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def place(dev, shape, offset, data=None):
    """A contiguous uint8 view of `shape`, `offset` bytes past a 16-byte boundary inside a buffer of 0xA5; `data` copied in, if given.
    Returns (view, buffer, lead)."""
    nbytes = int(np.prod(shape))
    buf = torch.full((nbytes + 2 * GUARD + 16,), 0xA5, dtype=torch.uint8, device=dev)
    lead = GUARD + (-(buf.data_ptr() + GUARD)) % 16 + offset
    view = buf[lead:lead + nbytes]
    assert view.data_ptr() % 16 == offset
    if data is not None:
        view.copy_(torch.from_numpy(np.array(data, copy=True).reshape(-1)).to(dev))       # (a writable copy: the clips are read-only)
    return view.view(shape), buf, lead


def guards_intact(t, buf, lead):
    return bool((buf[:lead] == 0xA5).all()) and bool((buf[lead + t.numel():] == 0xA5).all())


@pytest.fixture(scope='module')
def clips():
    """{shape: the packed clip (n, H, W, 2)}, seeded, read-only; no byte equal to the sentinel, so that an unwritten output byte shows."""
    out = {}
    for i, (n, H, W) in enumerate(SHAPES):
        a = np.random.default_rng(4220 + i).integers(0, 0xA5, (n, H, W, 2), dtype=np.uint8)
        a.setflags(write=False)
        out[(n, H, W)] = a
    return out


@pytest.mark.parametrize('order', nv16_model.ORDERS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: '%dx%dx%d' % s)
def test_unpack_and_pack_equal_the_model(dev, clips, shape, order):
    from meshflow_amd import ops
    n, H, W = shape
    packed_np = clips[shape]
    want_y, want_uv = nv16_model.unpack(packed_np, order)
    assert np.array_equal(nv16_model.pack(want_y, want_uv, order), packed_np)
    for p_off, y_off, uv_off in LAYOUTS:
        where = (shape, order, p_off, y_off, uv_off)
        # unpack: packed in, the pair out
        src, sbuf, slead = place(dev, (n, H, W, 2), p_off, packed_np)
        oy, ybuf, ylead = place(dev, (n, H, W), y_off)
        ouv, cbuf, clead = place(dev, (n, H, W // 2, 2), uv_off)
        got_y, got_uv = ops.unpack_422(src, order, out=(oy, ouv))
        torch.cuda.synchronize()
        assert got_y.data_ptr() == oy.data_ptr() and got_uv.data_ptr() == ouv.data_ptr()
        assert np.array_equal(oy.cpu().numpy(), want_y), where
        assert np.array_equal(ouv.cpu().numpy(), want_uv), where
        assert guards_intact(oy, ybuf, ylead) and guards_intact(ouv, cbuf, clead), where
        assert np.array_equal(src.cpu().numpy(), packed_np) and guards_intact(src, sbuf, slead), where
        # pack: that pair in (where unpack left it), packed out
        back, bbuf, blead = place(dev, (n, H, W, 2), p_off)
        got = ops.pack_422(oy, ouv, order, out=back)
        torch.cuda.synchronize()
        assert got.data_ptr() == back.data_ptr()
        assert np.array_equal(back.cpu().numpy(), packed_np), where                       # pack(unpack(x)) == x, and the model's pack
        assert guards_intact(back, bbuf, blead), where
        assert np.array_equal(oy.cpu().numpy(), want_y) and np.array_equal(ouv.cpu().numpy(), want_uv), where
        assert guards_intact(oy, ybuf, ylead) and guards_intact(ouv, cbuf, clead), where


@pytest.mark.parametrize('order', nv16_model.ORDERS)
def test_allocations_of_their_own(dev, clips, order):
    """Without `out`: new tensors of the right shapes, and the other order gives other bytes."""
    from meshflow_amd import ops
    shape = (2, 33, 130)
    n, H, W = shape
    packed = torch.from_numpy(np.array(clips[shape], copy=True)).to(dev)
    y, uv = ops.unpack_422(packed, order)
    assert tuple(y.shape) == (n, H, W) and tuple(uv.shape) == (n, H, W // 2, 2) and y.dtype == torch.uint8 and uv.dtype == torch.uint8
    want_y, want_uv = nv16_model.unpack(clips[shape], order)
    assert np.array_equal(y.cpu().numpy(), want_y) and np.array_equal(uv.cpu().numpy(), want_uv)
    again = ops.pack_422(y, uv, order)
    assert tuple(again.shape) == (n, H, W, 2) and torch.equal(again, packed)
    other = [o for o in nv16_model.ORDERS if o != order][0]
    swapped = ops.pack_422(y, uv, other)
    assert np.array_equal(swapped.cpu().numpy(), nv16_model.pack(want_y, want_uv, other)) and not torch.equal(swapped, packed)
    if order == 'yuyv':
        assert torch.equal(ops.unpack_422(packed)[0], y) and torch.equal(ops.pack_422(y, uv), packed)       # the default order


def test_refused_views_leave_the_outputs_untouched(dev, clips):
    """What the library refuses -- a packed view that is only 2-byte aligned, planes at odd addresses -- comes back as ValueError, nothing
    written."""
    from meshflow_amd import ops
    shape = (3, 5, 6)
    n, H, W = shape
    for p_off, y_off, uv_off, match in ((2, 0, 0, '4-byte aligned'), (0, 1, 0, '2-byte aligned'), (0, 0, 3, '2-byte aligned')):
        src, _, _ = place(dev, (n, H, W, 2), p_off, clips[shape])
        oy, ybuf, ylead = place(dev, (n, H, W), y_off)
        ouv, cbuf, clead = place(dev, (n, H, W // 2, 2), uv_off)
        with pytest.raises(ValueError, match=match):
            ops.unpack_422(src, 'uyvy', out=(oy, ouv))
        back, bbuf, blead = place(dev, (n, H, W, 2), p_off)
        with pytest.raises(ValueError, match=match):
            ops.pack_422(oy, ouv, 'uyvy', out=back)
        torch.cuda.synchronize()
        for t, buf in ((oy, ybuf), (ouv, cbuf), (back, bbuf)):
            assert bool((buf == 0xA5).all())
