"""The specification of the scene-cut statistic (`ops.frame_signatures`, `ops.cut_distances`, `ops.find_cuts`; mf_frame_signature_u8 and
mf_cut_distance_i32 in include/meshflow_hip.h): NumPy, integers only, so any order of summation gives the same bytes.

    signature   of an (H, W) uint8 frame: 4 x 4 tiles; tile row i covers rows [floor(i*H/4), floor((i+1)*H/4)), tile columns split W the same
                way (a tile may be empty when H < 4 or W < 4); 16 counters per tile, counter b = the number of the tile's pixels with
                value >> 4 == b; layout [tile_row][tile_col][bin], 256 counters per frame, which sum to H*W
    distance    D(a, b) = sum over the 256 counters of |a - b|, an integer in 0 .. 2*H*W (below 2^31 for W, H <= 32767)
    decision    on the host, from the integers: frame t starts a new shot iff D_t > floor(threshold * 2*H*W); threshold in [0, 1], default
                0.30 -- a design choice, not a value tuned on footage; at 1.0 nothing is ever a cut

This statistic is the project's own; the reference has none."""
import math

import numpy as np

TILES, BINS = 4, 16
COUNTERS = TILES * TILES * BINS
DEFAULT_THRESHOLD = 0.30


def tile_edges(size):
    """The TILES + 1 edges of the tiles along a side of `size` pixels."""
    return [i * size // TILES for i in range(TILES + 1)]


def signature(frame):
    """(256,) int32 of one (H, W) uint8 frame."""
    frame = np.asarray(frame)
    if frame.dtype != np.uint8 or frame.ndim != 2:
        raise ValueError(f'a signature is of one (H, W) uint8 frame (got {frame.dtype} {frame.shape})')
    rows, cols = tile_edges(frame.shape[0]), tile_edges(frame.shape[1])
    sig = np.zeros((TILES, TILES, BINS), np.int64)
    for i in range(TILES):
        for j in range(TILES):
            sig[i, j] = np.bincount((frame[rows[i]:rows[i + 1], cols[j]:cols[j + 1]] >> 4).reshape(-1), minlength=BINS)
    return sig.reshape(COUNTERS).astype(np.int32)


def signatures(stack):
    """(n, 256) int32 of an (n, H, W) uint8 stack."""
    return np.stack([signature(f) for f in stack])


def distance(a, b):
    return int(np.abs(np.asarray(a, np.int64) - np.asarray(b, np.int64)).sum())


def distances(sigs, prev=None):
    """(n,) int32: entry 0 is D(prev, sigs[0]) where prev is given, else 0; entry i is D(sigs[i - 1], sigs[i])."""
    sigs = np.asarray(sigs)
    first = distance(prev, sigs[0]) if prev is not None else 0
    return np.array([first] + [distance(sigs[i - 1], sigs[i]) for i in range(1, len(sigs))], np.int32)


def cut_bound(threshold, W, H):
    """The largest distance that is NOT a cut."""
    return math.floor(threshold * (2 * H * W))


def cuts(dist, threshold, W, H):
    """The indices i with dist[i] > floor(threshold * 2*H*W)."""
    bound = cut_bound(threshold, W, H)
    return [i for i, d in enumerate(dist) if int(d) > bound]


def find_cuts(stack, threshold=DEFAULT_THRESHOLD, prev=None):
    """(indices of the stack's frames that start a shot, distances (n,) int32, the last frame's signature)."""
    sigs = signatures(stack)
    dist = distances(sigs, prev)
    return cuts(dist, threshold, stack.shape[2], stack.shape[1]), dist, sigs[-1]
