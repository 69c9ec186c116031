"""Frames, grids and point sets for the tracker's edge tests (tests/test_track_edge_cases.py, tests/test_gpu_track_edges.py,
tests/test_track_second_opinion.py): sub-frames taller than the 64 rows `fast_compact_kernel` walks per round, FAST at other thresholds, at
the 8-bit maximum score and with tied neighbours, grids with fewer sub-frames than asked for, LK launches whose sub-frames differ in
pyramid depth, LK on 0/255 images, and outlier-step launches that send `track_gather_kernel`'s lane strides on a second trip.  Everything
comes from `synthetic.hash32`: the same on every platform.  Nothing here loads the HIP library; tests/test_track_edge_cases.py asserts with
the models alone that every case reaches the path it is named for."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ransac_cases as rc  # noqa: E402
import track_model as tm  # noqa: E402
import tracker_clip  # noqa: E402
from meshflow_amd import synthetic  # noqa: E402

ROUND = 64                                                               # mask rows fast_compact_kernel takes per round: one per lane


def noise(h, w, seed):
    return (synthetic.hash32(np.arange(h * w), seed) & 255).astype(np.uint8).reshape(h, w)


def binary(h, w, seed, block=1):
    """0 or 255 per `block` x `block` pixels, hashed."""
    bh, bw = -(-h // block), -(-w // block)
    small = ((synthetic.hash32(np.arange(bh * bw), seed) & 1) * 255).astype(np.uint8).reshape(bh, bw)
    return np.ascontiguousarray(np.repeat(np.repeat(small, block, axis=0), block, axis=1)[:h, :w])


def band_counts(img, threshold=10):
    """The model's corners of `img` as one sub-frame, per band of 64 rows."""
    ys = tm.fast_corners(img, threshold)[:, 1].astype(np.int64)
    return np.bincount(ys // ROUND, minlength=-(-img.shape[0] // ROUND)).tolist()


# ---- a. FAST, sub-frames of more than 64 rows -------------------------------------------------------------------------------------------

def tall_noise():
    return noise(150, 40, 31)


def tall_gap():
    """Rows 60 .. 134 constant: no row of the second round (64 .. 127) holds a corner."""
    img = noise(200, 40, 33)
    img[60:135] = 90
    return img


def tall_wide():
    return noise(200, 61, 32)


# name -> (frame, the model's corners per 64-row band as ONE sub-frame, ((rows, cols, max_per, where the capacity cuts), ...)); where = None: no
# overflow; r: strictly inside round r (counted from 0); ('fills', r): exactly at the end of round r, with corners still to come
def tall_cases():
    return {
        'noise 40 x 150': (tall_noise(), [216, 234, 72], ((1, 1, 1024, None), (1, 1, 300, 1), (1, 1, 216, ('fills', 0)), (1, 1, 460, 2))),
        'gap 40 x 200': (tall_gap(), [207, 0, 232, 20], ((1, 1, 1024, None), (1, 1, 230, 2))),
        'wide 61 x 200': (tall_wide(), [357, 386, 364, 33], ((1, 1, 2048, None), (1, 2, 2048, None))),
    }


def tall_stack():
    """Two images in one launch, the second constant: its slot's count starts from 0, not from the first slot's."""
    return np.stack([tall_noise(), np.full((150, 40), 77, np.uint8)])


# ---- b. FAST, thresholds and extremes ---------------------------------------------------------------------------------------------------

THRESHOLDS = {1: 262, 10: 259, 40: 191, 100: 23, 254: 0}                 # the model's corners of noise(48, 64, 1) at each threshold


def threshold_frame():
    return noise(48, 64, 1)


def binary_frame(block=1):
    return binary(48, 64, 5, block)


def quadrant(corner_x, corner_y, h=40, w=80):
    """The ideal two-level quadrant of tests/test_track_model.py: (corner_x, corner_y) and its diagonal neighbour both score 199 and the
    strict comparison keeps neither."""
    img = np.full((h, w), 20, np.uint8)
    img[corner_y:, corner_x:] = 220
    return img


# FAST tiles decide 56 x 14 pixels: the tie (x, y), (x + 1, y + 1) across a tile's right edge, its lower edge, and both
QUADRANT_CORNERS = ((55, 20), (30, 13), (55, 13))


def tie_pairs(img, threshold=10):
    """Pairs of 8-neighbours with equal non-zero model scores (each pair once)."""
    s = tm.fast_scores(img, threshold)
    h, w = s.shape
    pairs = 0
    for dy, dx in ((0, 1), (1, -1), (1, 0), (1, 1)):
        a = s[0:h - dy, max(0, -dx):w - max(0, dx)]
        b = s[dy:h, max(0, dx):w - max(0, -dx)]
        pairs += int(np.count_nonzero((a == b) & (a > 0)))
    return pairs


# ---- c. FAST, fewer sub-frames than asked for -------------------------------------------------------------------------------------------

FEWER = (49, 49, 8, 8)                                                   # W, H, sub_rows, sub_cols: ceil(49 / 8) = 7, so 7 x 7 sub-frames of 7 x 7


def fewer_frame(lit):
    """49 x 49, the centre pixel -- the one pixel of a 7 x 7 sub-frame that can be a corner -- lit in the sub-frames `lit` (model order)."""
    img = np.full((49, 49), 40, np.uint8)
    for s, (left, top, w, h) in enumerate(tm.subframes(49, 49, 8, 8)):
        if lit[s]:
            img[top + 3, left + 3] = 200
    return img


def fewer_lit_sets():
    s = np.arange(49)
    return [s % 2 == 0, s % 3 == 1, (synthetic.hash32(s, 9) & 1) == 1]


# ---- d. LK, sub-frames of unequal pyramid depth in one launch ---------------------------------------------------------------------------

MIXED_MAX_PER = 64


def mixed_canvas():
    return tracker_clip.canvas(190, 190, 11, boxes=200)


# name -> (size, crop origin (y, x) of the early frame, of the late frame, the model's num_levels per sub-frame as 2 x 2)
MIXED = {
    '169 x 169': (169, (10, 10), (8, 13), [2, 1, 1, 1]),
    '85 x 85': (85, (10, 10), (9, 12), [1, 0, 0, 0]),
}


def mixed_pair(name):
    size, (ey, ex), (ly, lx), _ = MIXED[name]
    big = mixed_canvas()
    return np.ascontiguousarray(big[ey:ey + size, ex:ex + size]), np.ascontiguousarray(big[ly:ly + size, lx:lx + size])


def depth_pair():
    """200 x 180 as one sub-frame: depth 3, 180 rows (three rounds of the compaction)."""
    big = tracker_clip.canvas(200, 230, 11)
    return np.ascontiguousarray(big[12:192, 20:220]), np.ascontiguousarray(big[9:189, 25:225])


def depths(w, h, rows, cols):
    return [tm.num_levels(sw, sh) for _, _, sw, sh in tm.subframes(w, h, rows, cols)]


# ---- e. LK, steep gradients -------------------------------------------------------------------------------------------------------------

def steep_big(block):
    return binary(70, 90, 7, block)


def steep_pairs():
    """[(name, early, late)], 48 x 40 each: the per-pixel and the 3 x 3-block 0/255 image shifted by one pixel, and the blocked one by six."""
    out = []
    for name, block, x in (('pixels, 1 px', 1, 19), ('blocks, 1 px', 3, 19), ('blocks, 6 px', 3, 14)):
        big = steep_big(block)
        out.append((name, np.ascontiguousarray(big[5:45, 20:68]), np.ascontiguousarray(big[5:45, x:x + 48])))
    return out


def steep_points():
    ys, xs = np.mgrid[2:40:5, 2:48:5]
    return (np.stack([xs.ravel(), ys.ravel()], 1) + 0.25).astype(np.float32)


def checker(h, w, seed, rate=8):
    """A 0/255 checkerboard of 2 x 2 squares -- |Ix| = |Iy| = 2,550 at every pixel, the steepest an image can be everywhere at once -- with one
    square in `rate` flipped by the hash, so that windows differ and the pattern is not periodic."""
    y, x = np.mgrid[0:h, 0:w]
    bh, bw = -(-h // 2), -(-w // 2)
    flip = (synthetic.hash32(np.arange(bh * bw), seed) % rate == 0).astype(np.int64).reshape(bh, bw)
    v = (((x >> 1) + (y >> 1)) & 1) ^ np.repeat(np.repeat(flip, 2, axis=0), 2, axis=1)[:h, :w]
    return (v * 255).astype(np.uint8)


def checker_pair():
    """(early, late, points): the checkerboard shifted by one pixel, tracked from INTEGER positions (weights (2^14, 0, 0, 0): nothing is
    averaged away), where the model's window sums pass 2^31."""
    big = checker(70, 90, 8)
    return np.ascontiguousarray(big[5:45, 20:68]), np.ascontiguousarray(big[5:45, 19:67]), steep_points() - np.float32(0.25)


def raw_window_sums(img, points):
    """The model's three exact integer sums (Ix Ix, Ix Iy, Iy Iy) over the level-0 window of every point, before the float32 scaling: int64
    (n, 3), rows of zeros for points whose window lies outside the image."""
    img = np.asarray(img)
    pts = np.asarray(points, np.float32).reshape(-1, 2)
    h, w = img.shape
    dx, dy = tm.scharr(img)
    pad_dx, pad_dy = np.pad(dx.astype(np.int64), tm._PAD), np.pad(dy.astype(np.int64), tm._PAD)
    prev = pts - tm.HALF
    ip = np.floor(prev).astype(np.int64)
    inside = ~tm._outside(ip, w, h)
    out = np.zeros((len(pts), 3), np.int64)
    ip, prev = ip[inside], prev[inside]
    w4 = tm._weights(prev[:, 0] - ip[:, 0].astype(np.float32), prev[:, 1] - ip[:, 1].astype(np.float32))
    gx = tm._bilinear(pad_dx, ip[:, 0], ip[:, 1], w4, tm.W_BITS)
    gy = tm._bilinear(pad_dy, ip[:, 0], ip[:, 1], w4, tm.W_BITS)
    out[inside] = np.stack([(gx * gx).sum(axis=(1, 2)), (gx * gy).sum(axis=(1, 2)), (gy * gy).sum(axis=(1, 2))], 1)
    return out


# ---- f. outlier step and gather: second trips of the 64-lane strides --------------------------------------------------------------------

STRIDE_SLOTS = 16
STRIDE_K = (0, 3, 9, 16, 12, 16)
# name -> (pairs, sub-frames, (W, H, sub_rows, sub_cols) of a frame cut into that many sub-frames)
STRIDE_LAUNCHES = {
    '70 pairs x 2': (70, 2, (40, 20, 1, 2)),
    '2 pairs x 70': (2, 70, (140, 20, 2, 35)),
}
STRIDE_SURVIVORS = 989
# per pair the model keeps 0, 20 or 23 survivors: 20 flags the empty pairs only; 21 also those of 20, whose survivors the pairs behind must skip
STRIDE_MIN_FEATURES = (4, 20, 21)


def stride_launch(name):
    """Sub-frame i of the launch (pair-major) gets k = (0, 3, 9, 16, 12, 16)[i % 6] planted correspondences from seed 500 + i, a fifth of them
    outliers where k > 8.  Both launches hold the same 140 sub-frames, cut into pairs differently."""
    n, S, _ = STRIDE_LAUNCHES[name]
    L = rc.Launch(n, S, STRIDE_SLOTS)
    for i in range(n * S):
        k = STRIDE_K[i % 6]
        e, l, _ = rc.planted(max(k, 1), 0.2 if k > 8 else 0.0, 500 + i)
        L.add(e[:k], l[:k])
    return L.arrays()
