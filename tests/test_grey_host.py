"""CPU: single-channel frames at the host boundary -- pipeline.HostClip takes (F, H, W) uint8 arrays and lists of (H, W) frames (as the
reference does: mfs.py:942, 1129 read shape[:2] only) and keeps its refusals; dist.gather_frames gathers (n, H, W) shards under gloo."""
import os
import socket
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def test_host_clip_accepts_grey():
    from meshflow_amd import pipeline
    F, H, W = 5, 6, 7
    a = np.arange(F * H * W, dtype=np.uint8).reshape(F, H, W)
    c = pipeline.HostClip(a, F)
    assert (c.channels, c.height, c.width, c.frame_shape) == (1, H, W, (H, W)) and c.array is not None
    wide = np.stack([a, a], axis=-1)
    frames = [wide[0][..., 0], a[1], np.frombuffer(a[2].tobytes(), np.uint8).reshape(H, W), a[3], a[3]]
    c = pipeline.HostClip(frames, F)
    assert c.channels == 1 and c.frame_shape == (H, W) and len(c.frames) == F
    assert all(f.flags.c_contiguous and f.shape == (H, W) for f in c.frames)
    np.testing.assert_array_equal(c.frames[0], a[0])
    c3 = pipeline.HostClip(np.zeros((F, H, W, 3), np.uint8), F)
    assert c3.channels == 3 and c3.frame_shape == (H, W, 3)


def test_host_clip_grey_refusals():
    from meshflow_amd import pipeline
    F, H, W = 4, 6, 7
    g = [np.zeros((H, W), np.uint8)] * F
    col = [np.zeros((H, W, 3), np.uint8)] * F
    for bad in ([np.zeros((H, W, 1), np.uint8)] * F, np.zeros((F, H, W, 1), np.uint8), col[:2] + [g[2]] + col[3:],
                g[:2] + [col[2]] + g[3:], [np.zeros((H, W, 4), np.uint8)] * F, g[:3] + [np.zeros((H + 1, W), np.uint8)],
                np.zeros((F + 1, H, W), np.uint8), g[:3]):
        with pytest.raises(ValueError):
            pipeline.HostClip(bad, F)
    for bad in ([f.astype(np.uint16) for f in g], np.zeros((F, H, W), np.float32), g[:3] + [g[3].astype(np.uint16)]):
        with pytest.raises(TypeError):
            pipeline.HostClip(bad, F)


def _gather_worker(rank, world, port, q):
    sys.path.insert(0, REPO)
    os.environ.update(RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK=str(rank), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    from meshflow_amd import dist as mfdist, host
    mfdist.init_from_env('cpu')
    F, H, W = 7, 5, 6
    full = torch.arange(F * H * W, dtype=torch.int64).remainder(251).to(torch.uint8).view(F, H, W)
    lo, hi = host.shard_range(F, world, rank)
    got = mfdist.gather_frames(full[lo:hi].contiguous(), F)
    if rank == 0:
        q.put(bool(got.shape == full.shape and torch.equal(got, full)))
    dist.destroy_process_group()


def test_gather_frames_of_grey_shards():
    import torch.multiprocessing as mp
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_gather_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
    assert all(p.exitcode == 0 for p in procs)
    assert q.get(timeout=5) is True
