"""-m gpu: the host-frame pipeline to a caller-chosen output size -- MeshFlowStabilizer.stabilize_clip(crop=True, output_size=...) through
mf_warp_crop_to_u8c3/_u8c1_host_frames and _crop_frames(output_size=...) through mf_crop_resize_to_*_host_frames -- for BGR and grey
clips: equal to ops.crop_resize(size=...) of the uncropped result and to the oracle; outputs larger than the input (ring slots sized by
the larger frame); a clip that wraps a small ring many times."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip('torch')

from meshflow_amd import ops, synthetic  # noqa: E402
from meshflow_amd.stabilizer import MeshFlowStabilizer  # noqa: E402
from oracle import meshflow_oracle as mo  # noqa: E402


@pytest.fixture(scope='module')
def dev():
    if not torch.cuda.is_available():
        pytest.fail('no GPU visible: the -m gpu tests must run on an MI355X')
    return torch.device('cuda:0')


def clip(F, H, W, grey, seed):
    frames, disp, hom = synthetic.clip(F, H, W, 4, 4, seed=seed, kind='noise', jitter_sigma=0.5)
    if grey:
        frames = np.ascontiguousarray(frames[..., 0])
    return frames, disp, hom


def stabilizer():
    return MeshFlowStabilizer(mesh_row_count=4, mesh_col_count=4, temporal_smoothing_radius=5, optimization_num_iterations=20,
                              device='cuda:0')


def oracle_resize(frames, bounds, size):
    l, t, r, b = (int(v) for v in bounds)
    out = []
    for f in frames:
        crop = f[t:b + 1, l:r + 1]
        if crop.ndim == 2:
            out.append(mo.resize_linear_u8(np.repeat(crop[..., None], 3, axis=2), *size)[..., 0])
        else:
            out.append(mo.resize_linear_u8(crop, *size))
    return np.stack(out)


@pytest.mark.parametrize('grey', [False, True])
@pytest.mark.parametrize('size', [(61, 37), (128, 96), (301, 203), (1, 1)])
def test_stabilize_clip_output_size(dev, grey, size):
    F, H, W = 12, 96, 128
    frames, disp, hom = clip(F, H, W, grey, seed=3)
    s = stabilizer()
    uncropped, bounds, stab, score = s.stabilize_clip(list(frames), disp, hom)
    none, bounds2, stab2, score2, cropped = s.stabilize_clip(list(frames), disp, hom, crop=True, keep_uncropped=False, output_size=size)
    assert none is None and tuple(bounds2) == tuple(bounds) and np.array_equal(stab2, stab) and score2 == score
    cropped = np.stack(cropped)
    assert cropped.shape == (F, size[1], size[0]) + frames.shape[3:]
    d = torch.from_numpy(np.ascontiguousarray(np.stack(uncropped))).to(dev)
    want = ops.crop_resize(d, bounds, size=size).cpu().numpy()
    assert np.array_equal(cropped, want)
    assert np.array_equal(cropped, oracle_resize(np.stack(uncropped), bounds, size))
    # keep_uncropped=True brings the same uncropped frames back beside them
    kept, _, _, _, cropped2 = s.stabilize_clip(list(frames), disp, hom, crop=True, output_size=size)
    assert np.array_equal(np.stack(kept), np.stack(uncropped)) and np.array_equal(np.stack(cropped2), cropped)


@pytest.mark.parametrize('grey', [False, True])
def test_crop_frames_output_size(dev, grey):
    F, H, W = 9, 70, 90
    rng = np.random.default_rng(5)
    frames = rng.integers(0, 256, (F, H, W) if grey else (F, H, W, 3), dtype=np.uint8)
    s = stabilizer()
    rect = (4, 6, 80, 61)
    for size in ((45, 28), (200, 150), (W, H)):
        got = np.stack(s._crop_frames(list(frames), rect, output_size=size))
        want = ops.crop_resize(torch.from_numpy(frames).to(dev), rect, size=size).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), size
        assert np.array_equal(got, oracle_resize(frames, rect, size))
    assert np.array_equal(np.stack(s._crop_frames(list(frames), rect, output_size=(W, H))), np.stack(s._crop_frames(list(frames), rect)))


@pytest.mark.parametrize('grey', [False, True])
def test_small_ring_wraps_many_times(dev, grey, monkeypatch):
    """One frame per chunk, two ring slots: 30 frames go through each slot 15 times, at an output smaller and one larger than the input."""
    monkeypatch.setenv('MF_PIPE_CHUNK', '1')
    monkeypatch.setenv('MF_PIPE_SLOTS', '2')
    F, H, W = 30, 64, 96
    frames, disp, hom = clip(F, H, W, grey, seed=8)
    s = stabilizer()
    for size in ((24, 16), (150, 100)):
        uncropped, bounds, _, _ = s.stabilize_clip(list(frames), disp, hom)
        _, _, _, _, cropped = s.stabilize_clip(list(frames), disp, hom, crop=True, keep_uncropped=False, output_size=size)
        want = ops.crop_resize(torch.from_numpy(np.ascontiguousarray(np.stack(uncropped))).to(dev), bounds, size=size).cpu().numpy()
        assert np.array_equal(np.stack(cropped), want), size
        got = np.stack(s._crop_frames(uncropped, bounds, output_size=size))
        assert np.array_equal(got, want), size
