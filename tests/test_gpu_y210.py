"""-m gpu: packed Y210 / Y216 against the P210 pair -- `ops.unpack_y210` and `ops.pack_y210` (pack_y210.hip), bit for bit
tests/p210_model.py's slicing -- and one packed clip end to end through `MeshFlowStabilizer.stabilized_y210_cropped`.

The word counts walk the kernels' cut of the word stream: every count from 1 (an empty clip is refused) through two full runs past the
longest head and tail (3 + 3 + 2 x 4 = 14, and on to 16), so that a head alone, head and tail without a run, and runs with and without a
tail all occur.  The planes are views into sentinel-filled buffers at EVERY residue mod 16 in 2-byte steps, `uv` in phase with `y` and out of
phase, and the packed side at both residues its contract allows (0 and 8): everything aligned (dwordx4 loads, 16-byte stores), the packed side
out of step (dwordx2 loads), planes 4-byte aligned off the boundary (a head in front of wide runs), planes 2-byte aligned only (2-byte
accesses throughout).  Around every output not a byte changes."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import p210_model  # noqa: E402

WORDS = list(range(1, 17))
GUARD = 48


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def place(dev, shape, offset, data=None):
    """A contiguous uint16 view of `shape`, `offset` bytes (even) past a 16-byte boundary inside a buffer of 0xA5 bytes; `data` copied in, if
    given.  Returns (view, buffer, lead, bytes)."""
    nbytes = 2 * int(np.prod(shape))
    buf = torch.full((nbytes + 2 * GUARD + 16,), 0xA5, dtype=torch.uint8, device=dev)
    lead = GUARD + (-(buf.data_ptr() + GUARD)) % 16 + offset
    view = buf[lead:lead + nbytes]
    assert view.data_ptr() % 16 == offset
    if data is not None:
        view.copy_(torch.from_numpy(np.array(data, dtype=np.uint16, copy=True).reshape(-1).view(np.uint8)).to(dev))
    return view.view(torch.uint16).view(shape), buf, lead, nbytes


def guards_intact(placed):
    _, buf, lead, nbytes = placed
    return bool((buf[:lead] == 0xA5).all()) and bool((buf[lead + nbytes:] == 0xA5).all())


def get(t):
    return t.cpu().numpy()


def clip(shape, seed):
    """A packed clip (n, H, W, 2) whose samples never hold the sentinel byte, so that an unwritten output byte shows."""
    a = np.random.default_rng(seed).integers(0, 0xA5, shape + (2,), dtype=np.uint16)
    a = (a | (np.random.default_rng(seed + 1).integers(0, 0xA5, shape + (2,), dtype=np.uint16) << 8)).astype(np.uint16)
    a.setflags(write=False)
    return a


@pytest.mark.parametrize('words', WORDS)
def test_unpack_and_pack_equal_slicing_at_every_residue(dev, words):
    from meshflow_amd import ops
    shape = (1, 1, 2 * words)
    n, H, W = shape
    packed_np = clip(shape, 2100 + words)
    want_y, want_uv = p210_model.unpack_y210(packed_np)
    assert np.array_equal(p210_model.pack_y210(want_y, want_uv), packed_np)
    for p_off in (0, 8):                                                # wide and narrow source layouts follow from p_off and the head
        for y_off in range(0, 16, 2):
            for uv_off in (y_off, (y_off + 6) % 16):
                where = (words, p_off, y_off, uv_off)
                # unpack: packed in, the pair out
                src = place(dev, (n, H, W, 2), p_off, packed_np)
                oy, ouv = place(dev, (n, H, W), y_off), place(dev, (n, H, W // 2, 2), uv_off)
                got_y, got_uv = ops.unpack_y210(src[0], out=(oy[0], ouv[0]))
                assert got_y.data_ptr() == oy[0].data_ptr() and got_uv.data_ptr() == ouv[0].data_ptr()
                assert np.array_equal(get(oy[0]), want_y) and np.array_equal(get(ouv[0]), want_uv), where
                assert guards_intact(oy) and guards_intact(ouv) and guards_intact(src), where
                assert np.array_equal(get(src[0]), packed_np), where
                # pack: that pair in (where unpack left it), packed out
                back = place(dev, (n, H, W, 2), p_off)
                got = ops.pack_y210(oy[0], ouv[0], out=back[0])
                assert got.data_ptr() == back[0].data_ptr()
                assert np.array_equal(get(back[0]), packed_np), where
                assert guards_intact(back) and guards_intact(oy) and guards_intact(ouv), where
                assert np.array_equal(get(oy[0]), want_y) and np.array_equal(get(ouv[0]), want_uv), where


@pytest.mark.parametrize('shape', [(3, 5, 6), (2, 33, 130), (1, 16, 64)], ids=lambda s: '%dx%dx%d' % s)
def test_clips_of_many_runs(dev, shape):
    """Rows and frames do not matter to the kernels: whole clips, more than one workgroup of runs, on allocations of their own and at
    offsets."""
    from meshflow_amd import ops
    n, H, W = shape
    packed_np = clip(shape, 4210)
    want_y, want_uv = p210_model.unpack_y210(packed_np)
    packed = torch.from_numpy(np.array(packed_np, copy=True)).to(dev)
    y, uv = ops.unpack_y210(packed)
    assert tuple(y.shape) == (n, H, W) and tuple(uv.shape) == (n, H, W // 2, 2) and y.dtype == torch.uint16 and uv.dtype == torch.uint16
    assert np.array_equal(get(y), want_y) and np.array_equal(get(uv), want_uv)
    again = ops.pack_y210(y, uv)
    assert tuple(again.shape) == (n, H, W, 2) and np.array_equal(get(again), packed_np)
    for p_off, y_off, uv_off in ((8, 4, 4), (0, 12, 12), (8, 2, 10), (0, 0, 8), (8, 6, 6)):
        src = place(dev, (n, H, W, 2), p_off, packed_np)
        oy, ouv = place(dev, (n, H, W), y_off), place(dev, (n, H, W // 2, 2), uv_off)
        ops.unpack_y210(src[0], out=(oy[0], ouv[0]))
        back = place(dev, (n, H, W, 2), p_off)
        ops.pack_y210(oy[0], ouv[0], out=back[0])
        assert np.array_equal(get(oy[0]), want_y) and np.array_equal(get(ouv[0]), want_uv) and np.array_equal(get(back[0]), packed_np)
        assert guards_intact(oy) and guards_intact(ouv) and guards_intact(back) and guards_intact(src)


def test_refused_views_leave_the_outputs_untouched(dev):
    """What the library refuses -- a packed view that is only 2- or 4-byte aligned -- comes back as ValueError, nothing written."""
    from meshflow_amd import ops
    shape = (3, 5, 6)
    n, H, W = shape
    for p_off in (2, 4, 12):
        src = place(dev, (n, H, W, 2), p_off, clip(shape, 7))
        oy, ouv = place(dev, (n, H, W), 0), place(dev, (n, H, W // 2, 2), 0)
        with pytest.raises(ValueError, match='8-byte aligned'):
            ops.unpack_y210(src[0], out=(oy[0], ouv[0]))
        back = place(dev, (n, H, W, 2), p_off)
        with pytest.raises(ValueError, match='8-byte aligned'):
            ops.pack_y210(oy[0], ouv[0], out=back[0])
        torch.cuda.synchronize()
        for placed in (oy, ouv, back):
            assert bool((placed[1] == 0xA5).all())


def test_a_packed_clip_end_to_end(dev):
    """`stabilized_y210_cropped` is unpack, the P210 warp, the P210 crop-resize from the rectangle on the device, pack; `stabilized_y210` and
    `ops.warp_y210` are unpack, warp, pack."""
    from meshflow_amd import ops, synthetic
    from meshflow_amd.stabilizer import MeshFlowStabilizer
    F, H, W, R, C = 8, 65, 96, 3, 4
    disp, hom = synthetic.motion(F, R, C, seed=71, jitter_sigma=2.0)
    s = MeshFlowStabilizer(mesh_row_count=R, mesh_col_count=C, temporal_smoothing_radius=4, optimization_num_iterations=15, device='cuda:0')
    packed_np = np.random.default_rng(9).integers(0, 65536, (F, H, W, 2), dtype=np.uint16)
    packed = torch.from_numpy(packed_np.copy()).to(dev)
    d_disp = torch.from_numpy(np.ascontiguousarray(disp, dtype=np.float64)).to(dev)
    border = (4660, 51966, 300)
    y, uv = ops.unpack_y210(packed)
    plain_y, plain_uv, b = s.stabilized_p210(y, uv, d_disp, hom, border)
    rect = tuple(b.tolist())
    assert rect != (0, 0, W - 1, H - 1)
    out, ob = s.stabilized_y210(packed, d_disp, hom, border)
    assert torch.equal(ob, b) and np.array_equal(get(out), p210_model.pack_y210(get(plain_y), get(plain_uv)))
    for size in (None, (128, 91), (48, 33)):
        sy, suv, sb = s.stabilized_p210_cropped(y, uv, d_disp, hom, border, output_size=size)
        got, gb = s.stabilized_y210_cropped(packed, d_disp, hom, border, output_size=size)
        assert torch.equal(gb, sb) and torch.equal(gb, b)
        assert np.array_equal(get(got), p210_model.pack_y210(get(sy), get(suv))), size
        # ... and the composition on the model's side of the crop: the warped pair through tests/p210_model.py
        my, muv = p210_model.crop_resize_clip(get(plain_y), get(plain_uv), rect, size)
        assert np.array_equal(get(got), p210_model.pack_y210(my, muv)), size
    buf = torch.empty((F, 33, 48, 2), dtype=torch.int16, device=dev).view(torch.uint16)
    r, _ = s.stabilized_y210_cropped(packed, d_disp, hom, border, out=buf, output_size=(48, 33))
    assert r.data_ptr() == buf.data_ptr() and np.array_equal(get(buf), get(got))
    assert np.array_equal(get(packed), packed_np)
