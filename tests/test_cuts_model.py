"""tests/cuts_model.py, the specification of the scene-cut statistic: its own properties, and how far it separates the material the GPU tests
cut their clips from -- computed here with exactly this statistic, so that the default threshold of 0.30 is seen to have room on both sides.
No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cuts_clip  # noqa: E402
import cuts_model as cm  # noqa: E402
import luma_clip  # noqa: E402
import luma_model  # noqa: E402

W, H = cuts_clip.W, cuts_clip.H


def noise(shape, seed):
    return luma_clip._noise(shape, 256, seed).astype(np.uint8)


@pytest.mark.parametrize('shape', [(1, 1), (5, 3), (7, 9), (96, 128), (97, 131), (3, 2), (2, 40)])
def test_counters_sum_to_the_frame(shape):
    sig = cm.signature(noise(shape, 3))
    assert sig.dtype == np.int32 and sig.shape == (256,) and (sig >= 0).all() and int(sig.sum()) == shape[0] * shape[1]
    per_tile = sig.reshape(4, 4, 16).sum(axis=2)
    rows, cols = cm.tile_edges(shape[0]), cm.tile_edges(shape[1])
    want = np.outer(np.diff(rows), np.diff(cols))
    assert per_tile.tolist() == want.tolist()


def test_tile_bounds():
    assert cm.tile_edges(5) == [0, 1, 2, 3, 5] and cm.tile_edges(3) == [0, 0, 1, 2, 3]            # (H, W) = (5, 3): tile column 0 is empty
    assert cm.tile_edges(7) == [0, 1, 3, 5, 7] and cm.tile_edges(9) == [0, 2, 4, 6, 9]
    assert cm.tile_edges(97) == [0, 24, 48, 72, 97] and cm.tile_edges(131) == [0, 32, 65, 98, 131]
    sig = cm.signature(np.full((5, 3), 200, np.uint8)).reshape(4, 4, 16)
    assert (sig[:, 0] == 0).all() and sig[3, 3, 200 >> 4] == 2 and sig[0, 1, 200 >> 4] == 1


def test_layout_and_bins():
    frame = np.zeros((8, 8), np.uint8)
    frame[2:4, 6:8] = 0x5f                          # tile row 1, tile column 3, bin 5
    sig = cm.signature(frame)
    assert sig[(1 * 4 + 3) * 16 + 5] == 4 and sig[(1 * 4 + 3) * 16 + 0] == 0 and int(sig.sum()) == 64
    for value, b in ((0, 0), (15, 0), (16, 1), (239, 14), (240, 15), (255, 15)):
        sig = cm.signature(np.full((4, 4), value, np.uint8)).reshape(16, 16)
        assert (sig[:, b] == 1).all() and int(sig.sum()) == 16, value


def test_permuting_a_tile_s_pixels_changes_nothing():
    frame = noise((97, 131), 5)
    rows, cols = cm.tile_edges(97), cm.tile_edges(131)
    shuffled = frame.copy()
    rng = np.random.default_rng(7)
    for i in range(4):
        for j in range(4):
            tile = shuffled[rows[i]:rows[i + 1], cols[j]:cols[j + 1]]
            tile[...] = rng.permutation(tile.reshape(-1)).reshape(tile.shape)
    assert not np.array_equal(shuffled, frame)
    assert cm.signature(shuffled).tobytes() == cm.signature(frame).tobytes()


def test_distance_is_symmetric_and_reaches_its_extreme():
    a, b = cm.signature(noise((97, 131), 11)), cm.signature(noise((97, 131), 12) >> 1)
    assert cm.distance(a, b) == cm.distance(b, a) > 0 and cm.distance(a, a) == 0
    for shape in ((1, 1), (5, 3), (96, 128)):
        black, white = cm.signature(np.zeros(shape, np.uint8)), cm.signature(np.full(shape, 255, np.uint8))
        assert cm.distance(black, white) == 2 * shape[0] * shape[1]
    sigs = np.stack([a, b, a])
    assert cm.distances(sigs).tolist() == [0, cm.distance(a, b), cm.distance(a, b)]
    assert cm.distances(sigs, prev=b).tolist() == [cm.distance(a, b)] * 3
    assert cm.distances(sigs).dtype == np.int32
    assert 2 * 32767 * 32767 < 2 ** 31


def test_the_decision():
    dist = [0, 10, 11, 20]
    assert cm.cut_bound(0.5, 5, 2) == 10 and cm.cuts(dist, 0.5, 5, 2) == [2, 3]          # a cut is ABOVE floor(threshold * 2HW)
    assert cm.cuts(dist, 1.0, 5, 2) == [] and cm.cuts(dist, 0.0, 5, 2) == [1, 2, 3]
    assert cm.cuts([2 * H * W], 1.0, W, H) == []                                            # at 1.0 nothing is ever a cut
    assert cm.DEFAULT_THRESHOLD == 0.30


def ratios(stack):
    return cm.distances(cm.signatures(stack))[1:] / (2.0 * H * W)


def test_the_test_material_is_separated():
    """Within a scene D / 2HW is 0.052 to 0.109, and 0.598 to 0.618 across a cut at any frame t (frame t - 1 of one scene, frame t of the
    other, either way round); the luma of the colour form B = 255 - g, G = g, R = g gives 0.043 to 0.107 within and 0.591 to 0.610 across."""
    a, b = cuts_clip.scene_a(), cuts_clip.scene_b()
    assert a.shape == b.shape == (10, H, W)
    within, across = [], []
    for grey in (lambda g: g, lambda g: luma_model.luma(luma_clip.bgr(g))):
        ga, gb = grey(a), grey(b)
        w = np.concatenate([ratios(ga), ratios(gb)])
        sa, sb = cm.signatures(ga), cm.signatures(gb)
        # a cut at frame t: from frame t - 1 of one scene to frame t of the other
        x = np.array([cm.distance(p[t - 1], q[t]) for p, q in ((sa, sb), (sb, sa)) for t in range(1, 10)]) / (2.0 * H * W)
        print('within %.3f .. %.3f, across %.3f .. %.3f' % (w.min(), w.max(), x.min(), x.max()))
        within.append(w)
        across.append(x)
    for w, x in zip(within, across):
        assert w.max() < 0.15 and x.min() > 0.5                         # the default 0.30 has room on both sides
    assert cm.find_cuts(cuts_clip.one_cut())[0] == [5] and cm.find_cuts(cuts_clip.two_cuts())[0] == [3, 7] and cm.find_cuts(a)[0] == []
