"""A second statement of three functions of tests/track_model.py -- FAST scores and corners, pyrDown, the Scharr derivative -- written from
their definitions instead of the model's formulas, so that a mistake the model shares with the kernel (`fast_best` and the model's arc
minima are one formula written twice) does not pass unseen.  Slow and plain on purpose; CPU only (tests/test_track_second_opinion.py).

  FAST     a pixel p is a corner at t if some 9 contiguous pixels of its 16-pixel circle are all > p + t or all < p - t; no pixel within 3
           of an edge is one.  That is tested as written, per pixel and per t, with boolean arrays: no difference is ever minimised.  The
           score of a corner at `threshold` is the largest t in 0 .. 254 at which it still is one ("still": being a corner at t implies
           being one at every smaller t, so the search walks t upwards from `threshold` and stops where the last pixel drops out).  A
           corner is kept if its score is strictly greater than its 8 neighbours' (0 outside the image and for non-corners).
  pyrDown  np.pad(img, 2, mode='reflect') -- NumPy's 'reflect' does not repeat the edge sample: BORDER_REFLECT_101 --, [1 4 6 4 1] along x
           then along y in exact integers, every second sample from 0, (s + 128) >> 8.  For sizes of 3 and more per side (a pad of 2 by
           reflection needs 3 samples).
  Scharr   the same padding by 1, (3, 10, 3) across and (-1, 0, 1) along the derivative's axis, int16."""
import numpy as np

# the Bresenham circle of radius 3, clockwise from the pixel below (dx, dy); any rotation or direction of it defines the same corners
RING = ((0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2),
        (-1, 3))


def _has_run_of_9(flags):
    """flags (16, ...) bool around the circle -> (...) bool: 9 contiguous true, the circle closed."""
    closed = np.concatenate([flags, flags[:8]])
    hit = np.zeros(flags.shape[1:], bool)
    for start in range(16):
        run = np.ones(flags.shape[1:], bool)
        for i in range(9):
            run &= closed[start + i]
        hit |= run
    return hit


def fast_scores(img, threshold=10):
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    h, w = img.shape
    score = np.zeros((h, w), np.int32)
    if h < 7 or w < 7:
        return score
    p = img.astype(np.int64)
    ys, xs = [v.ravel() for v in np.mgrid[3:h - 3, 3:w - 3]]
    for t in range(int(threshold), 255):
        if len(ys) == 0:
            break
        centre = p[ys, xs]
        ring = np.stack([p[ys + dy, xs + dx] for dx, dy in RING])
        corner = _has_run_of_9(ring > centre + t) | _has_run_of_9(ring < centre - t)
        ys, xs = ys[corner], xs[corner]
        score[ys, xs] = t                                                # still a corner at t: at least t
    return score


def fast_corners(img, threshold=10):
    s = fast_scores(img, threshold)
    h, w = s.shape
    out = []
    for y in range(h):
        for x in range(w):
            if s[y, x] == 0:
                continue
            near = [s[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dy or dx) and 0 <= y + dy < h and 0 <= x + dx < w]
            if all(s[y, x] > v for v in near):
                out.append((x, y))
    return np.array(out, np.float32).reshape(-1, 2)


def pyr_down(img):
    img = np.asarray(img)
    h, w = img.shape
    assert h >= 3 and w >= 3
    p = np.pad(img.astype(np.int64), 2, mode='reflect')
    across = p[:, 0:w] + 4 * p[:, 1:w + 1] + 6 * p[:, 2:w + 2] + 4 * p[:, 3:w + 3] + p[:, 4:w + 4]          # (h + 4, w), centred on x
    both = across[0:h] + 4 * across[1:h + 1] + 6 * across[2:h + 2] + 4 * across[3:h + 3] + across[4:h + 4]  # (h, w), centred on (x, y)
    return ((both[::2, ::2] + 128) >> 8).astype(np.uint8)


def scharr(img):
    img = np.asarray(img)
    h, w = img.shape
    assert h >= 2 and w >= 2
    p = np.pad(img.astype(np.int64), 1, mode='reflect')
    ix, iy = np.zeros((h, w), np.int64), np.zeros((h, w), np.int64)
    for j, weight in enumerate((3, 10, 3)):
        ix += weight * (p[j:j + h, 2:w + 2] - p[j:j + h, 0:w])           # rows y - 1, y, y + 1; columns x + 1 minus x - 1
        iy += weight * (p[2:h + 2, j:j + w] - p[0:h, j:j + w])
    return ix.astype(np.int16), iy.astype(np.int16)
