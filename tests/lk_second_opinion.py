"""A second opinion on Lucas-Kanade that owes nothing to tests/track_model.py: analytic scenes whose motion is known exactly, and a
float64 textbook tracker written from the normal equations.  NumPy float64 only: no fixed point, no cvRound, no float32, and no import of
the model.  The model (tests/test_lk_second_opinion.py) and the kernel (tests/test_gpu_lk_second_opinion.py) are judged against both.

  scene      a band-limited texture in closed form (largest wave number 0.433 rad / pixel: the shortest period is 14.5 pixels; the
             amplitudes add up to 120 around 128, so nothing clips).  `late` is the same formula at the analytically inverse-mapped
             coordinates, rounded once to uint8: no resampling, no interpolation error.  `truth_fn` maps points exactly.
  textbook   the pyramid is `track_definition.pyr_down` (at most 3 extra levels, none whose width or height is not larger than 21), the
             gradient is `track_definition.scharr / 32` of the early level, ZERO outside the image; image taps are reflect-101 with float64
             bilinear weights.  Per level the template I(x) and G = sum grad grad^T over the 21 x 21 window (offsets -10 .. 10 around the
             point) are taken once; each iteration is v -= G^-1 sum (J(x + v) - I(x)) grad; v goes to the next finer level as 2 v.  Coarse
             levels stop after 30 iterations or a step below 0.01 pixel.  Level 0 runs to its FIXED POINT (step below 1e-7, at most 200
             iterations, `converged` says whether it got there), so that the answer does not depend on a stop rule; stop='cv2' stops level
             0 like the coarse levels and exists only to measure how far a stop rule of that size leaves a tracker from its fixed point.
  judged     the points the comparison is about: the textbook converged and its fixed point lies within 0.6 pixel of the truth.  All
             else are tracks Lucas-Kanade loses for reasons of its own (aperture, reach at the top level) and is compared with nothing.

The textbook knows nothing of "lost" points, minimum eigenvalues, half-step exits or the second bounds test; a singular G or a track that
runs away simply does not converge."""
import functools

import numpy as np

import track_definition as td

WINDOW = 21
REACH = 10                              # window offsets -10 .. 10
MAX_EXTRA_LEVELS = 3
COARSE_ITERATIONS, COARSE_STEP = 30, 0.01
FIXED_ITERATIONS, FIXED_STEP = 200, 1e-7
JUDGED_RADIUS = 0.6
BAR = 0.01                              # cv2's convergence radius, TOLERANCE of tests/test_cv2_track_crosscheck.py


def texture_at(x, y):
    """Wave vectors (0.31, +-0.23), (0.13, 0.19), (0.07, -0.11), (0.33, -0.28): the last is the largest, 0.433 rad / pixel."""
    return 128 + 40 * np.sin(x * 0.31 + 0.2) * np.cos(y * 0.23) + 35 * np.sin(x * 0.13 + y * 0.19 + 1) + 30 * np.cos(x * 0.07 - y * 0.11) + \
        15 * np.sin(x * 0.33 - y * 0.28)


def as_homography(motion):
    """A translation (dx, dy), a 2 x 3 affine or a 3 x 3 homography as a 3 x 3 float64 matrix."""
    m = np.asarray(motion, np.float64)
    if m.shape == (2,):
        return np.array([[1.0, 0.0, m[0]], [0.0, 1.0, m[1]], [0.0, 0.0, 1.0]])
    if m.shape == (2, 3):
        return np.vstack([m, [0.0, 0.0, 1.0]])
    assert m.shape == (3, 3), m.shape
    return m


def transfer(matrix, points):
    points = np.asarray(points, np.float64).reshape(-1, 2)
    q = points @ matrix[:, :2].T + matrix[:, 2]
    return q[:, :2] / q[:, 2:]


def scene(h, w, motion):
    """(early, late, truth_fn): the content of `early` at x is the content of `late` at truth_fn(x)."""
    m = as_homography(motion)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    early = np.rint(texture_at(x, y))
    back = transfer(np.linalg.inv(m), np.stack([x.ravel(), y.ravel()], 1))
    late = np.rint(texture_at(back[:, 0], back[:, 1])).reshape(h, w)
    assert early.min() >= 0 and early.max() <= 255 and late.min() >= 0 and late.max() <= 255
    return early.astype(np.uint8), late.astype(np.uint8), functools.partial(transfer, m)


def _reflect101(i, n):
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    i = np.abs(i) % period
    return np.where(i >= n, period - i, i)


def bilinear(img, x, y, outside):
    """img (float64) at real positions; taps outside the image are reflected ('reflect': gfedcb|abcdefgh|gfedcba) or 0 ('zero')."""
    h, w = img.shape
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    x0, y0 = x0.astype(np.int64), y0.astype(np.int64)

    def tap(xi, yi):
        if outside == 'reflect':
            return img[_reflect101(yi, h), _reflect101(xi, w)]
        assert outside == 'zero'
        inside = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
        return np.where(inside, img[np.clip(yi, 0, h - 1), np.clip(xi, 0, w - 1)], 0.0)

    return (1 - fy) * ((1 - fx) * tap(x0, y0) + fx * tap(x0 + 1, y0)) + fy * ((1 - fx) * tap(x0, y0 + 1) + fx * tap(x0 + 1, y0 + 1))


def pyramid(img):
    levels = [np.asarray(img)]
    while len(levels) <= MAX_EXTRA_LEVELS:
        h, w = levels[-1].shape
        if (w + 1) // 2 <= WINDOW or (h + 1) // 2 <= WINDOW:
            break
        levels.append(td.pyr_down(levels[-1]))
    return levels


def _track_level(early, late, where, v, iterations, smallest_step, gradient_border):
    """One level: `where` (N, 2) the points on this level, `v` (N, 2) the displacement so far (updated in place) -> converged (N,)."""
    gx, gy = (g.astype(np.float64) / 32 for g in td.scharr(early))
    early, late = early.astype(np.float64), late.astype(np.float64)
    offsets = np.arange(-REACH, REACH + 1, dtype=np.float64)
    x = where[:, 0, None, None] + offsets[None, None, :]
    y = where[:, 1, None, None] + offsets[None, :, None]
    template = bilinear(early, x, y, 'reflect')
    ix, iy = bilinear(gx, x, y, gradient_border), bilinear(gy, x, y, gradient_border)
    gxx, gxy, gyy = (ix * ix).sum((1, 2)), (ix * iy).sum((1, 2)), (iy * iy).sum((1, 2))
    det = gxx * gyy - gxy * gxy
    converged = np.zeros(len(where), bool)
    active = det > 1e-9 * (gxx + gyy) ** 2 + 1e-300                   # a singular G has no inverse: the track stays where it is
    limit = 4.0 * max(early.shape)                                      # a track this far out has run away: stop following it
    for _ in range(iterations):
        i = np.nonzero(active)[0]
        if len(i) == 0:
            break
        mismatch = bilinear(late, x[i] + v[i, 0, None, None], y[i] + v[i, 1, None, None], 'reflect') - template[i]
        bx, by = (mismatch * ix[i]).sum((1, 2)), (mismatch * iy[i]).sum((1, 2))
        step = np.stack([gyy[i] * bx - gxy[i] * by, gxx[i] * by - gxy[i] * bx], 1) / det[i, None]        # G^-1 b
        v[i] -= step
        size = np.hypot(step[:, 0], step[:, 1])
        arrived = size < smallest_step
        converged[i[arrived]] = True
        active[i[arrived | ~(np.abs(v[i]).max(1) < limit)]] = False
    return converged


def textbook_lk(early, late, points, stop='fixed_point', gradient_border='zero'):
    """-> (moved (N, 2) float64, converged (N,) bool).  stop='fixed_point' or 'cv2' (above).  gradient_border='reflect' is NOT the
    textbook: it exists to show what the other reading of the derivative's border does."""
    assert stop in ('fixed_point', 'cv2')
    early, late = np.asarray(early), np.asarray(late)
    assert early.shape == late.shape and early.ndim == 2
    points = np.asarray(points, np.float64).reshape(-1, 2)
    v = np.zeros_like(points)
    converged = np.zeros(len(points), bool)
    if len(points) == 0:
        return points.copy(), converged
    levels = list(zip(pyramid(early), pyramid(late)))
    for level in range(len(levels) - 1, -1, -1):
        iterations, smallest = (FIXED_ITERATIONS, FIXED_STEP) if level == 0 and stop == 'fixed_point' else (COARSE_ITERATIONS, COARSE_STEP)
        converged = _track_level(levels[level][0], levels[level][1], points / 2.0 ** level, v, iterations, smallest, gradient_border)
        if level:
            v *= 2.0
    return points + v, converged


def distance(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    return np.hypot(d[..., 0], d[..., 1])


def judged(fixed_point, converged, truth):
    return np.asarray(converged, bool) & (distance(fixed_point, truth) <= JUDGED_RADIUS)


# ---- the case table: the smallest images (width x height) that still have each pyramid depth, and an odd one ------------------------------

IMAGES = ((48, 40), (80, 60), (96, 88), (180, 200), (61, 45))
DEPTHS = (0, 1, 2, 3, 1)


def _affine():
    """Rotation 0.01 rad, zoom 1.01, shift (1.3, -0.7), about the image's origin: up to 4 pixels of motion at the far corner of 180 x 200."""
    c, s = 1.01 * np.cos(0.01), 1.01 * np.sin(0.01)
    return as_homography([[c, -s, 1.3], [s, c, -0.7]])


def _homography():
    """The affine with a perspective row that changes the scale by about 1 % across the largest image."""
    m = _affine()
    m[2, :2] = 6e-5, -4e-5
    return m


SHIFTS = ((2.25, -1.5), (-3.5, 4.0), (0.5, 0.5), (0.125, -0.0625), (1.0, 0.0), (0.0, 0.0))
INTEGER_SHIFTS = ((1.0, 0.0), (0.0, 0.0))
# A case whose judged share the textbook alone puts below 0.9 is replaced by a gentler one, never judged more loosely.  (-3.5, 4) carries the
# border set's first column and the interior grid's windows out of the four smaller images (shares 0.86, 0.88, 0.87, 0.83) and (2.25, -1.5)
# does the same on 61 x 45 (0.88).  Halving (-3.5, 4) was NOT the replacement: on 80 x 60 it leaves one judged border track whose iteration
# contracts so slowly that a 0.01 stop rule ends 0.025 pixel short of the fixed point (profiles/tracker.md), which is no tracker's error.
GENTLER = {((48, 40), (-3.5, 4.0)): (-2.5, 3.0), ((80, 60), (-3.5, 4.0)): (-2.5, 3.0), ((96, 88), (-3.5, 4.0)): (-2.5, 3.0),
           ((61, 45), (-3.5, 4.0)): (-2.5, 3.0), ((61, 45), (2.25, -1.5)): (1.75, -1.0)}


def _table():
    out = {}
    for size in IMAGES:
        for shift in SHIFTS:
            shift = GENTLER.get((size, shift), shift)
            out['%dx%d-shift_%g_%g' % (size + shift)] = (size, as_homography(shift))
        out['%dx%d-affine' % size] = (size, _affine())
        out['%dx%d-homography' % size] = (size, _homography())
    return out


TABLE = _table()
CASES = tuple(TABLE)
INTEGER_CASES = tuple('%dx%d-shift_%g_%g' % (size + shift) for size in IMAGES for shift in INTEGER_SHIFTS)


def grid_points(w, h):
    """(points (N, 2) float64, interior (N,) bool): the interior grid -- steps 11 x 9 from 12 pixels inside, every third point moved by
    (0.375, 0.625) --, then a border set with the same steps from 2 pixels inside: its windows hang over the near borders at level 0 and
    over every border at the coarse levels (at the top level of 180 x 200, 23 x 25 pixels, no window fits inside)."""
    ys, xs = np.meshgrid(np.arange(12, h - 12, 9), np.arange(12, w - 12, 11), indexing='ij')
    inner = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
    inner[::3] += (0.375, 0.625)
    ys, xs = np.meshgrid(np.arange(2, h - 2, 9), np.arange(2, w - 2, 11), indexing='ij')
    outer = np.stack([xs.ravel(), ys.ravel()], 1).astype(np.float64)
    return np.concatenate([inner, outer]), np.arange(len(inner) + len(outer)) < len(inner)


class Reference:
    """Everything the textbook has to say about one pair of images and its points; computed once and shared, never modified."""

    def __init__(self, early, late, points, truth):
        self.early, self.late, self.points, self.truth = early, late, points, truth
        self.fixed_point, self.converged = textbook_lk(early, late, points)
        self.judged = judged(self.fixed_point, self.converged, truth)
        for a in (self.early, self.late, self.points, self.truth, self.fixed_point, self.converged, self.judged):
            a.setflags(write=False)

    @property
    def share(self):
        return float(self.judged.mean())

    @functools.cached_property
    def cv2_stop(self):
        return textbook_lk(self.early, self.late, self.points, stop='cv2')[0]

    def verdict(self, moved, found):
        """The three assertions on a tracker's answer for these points, as worst figures over the judged points:
        (the number judged and not found, max |moved - fixed point|, max (|moved - truth| - |fixed point - truth|))."""
        j = self.judged
        moved, found = np.asarray(moved, np.float64)[j], np.asarray(found)[j]
        if not j.any():
            return 0, 0.0, 0.0
        return (int((found != 1).sum()), float(distance(moved, self.fixed_point[j]).max()),
                float((distance(moved, self.truth[j]) - distance(self.fixed_point[j], self.truth[j])).max()))


def crop_reference(early, late, points, truth_fn, left=0, top=0, w=None, h=None):
    """The reference of one sub-frame as an image of its own: `points` and the truth are relative to (left, top)."""
    w, h = early.shape[1] - left if w is None else w, early.shape[0] - top if h is None else h
    e, l = (np.ascontiguousarray(a[top:top + h, left:left + w]) for a in (early, late))
    points = np.asarray(points, np.float64).reshape(-1, 2)
    return Reference(e, l, points, truth_fn(points + (left, top)) - (left, top))


@functools.lru_cache(maxsize=None)
def case_scene(name):
    """(early, late, truth_fn, the 3 x 3 matrix) of a table case."""
    (w, h), matrix = TABLE[name]
    return scene(h, w, matrix) + (matrix,)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    early, late, truth_fn, _ = case_scene(name)
    points, interior = grid_points(early.shape[1], early.shape[0])
    ref = crop_reference(early, late, points, truth_fn)
    ref.interior = interior
    return ref


def subframes(width, height, rows, cols):
    """[(left, top, w, h)] of the tracker's sub-frame grid in its order: ceil-sized, left outer, top inner, the last column / row smaller."""
    sub_w, sub_h = -(-width // cols), -(-height // rows)
    return [(left, top, min(sub_w, width - left), min(sub_h, height - top)) for left in range(0, width, sub_w) for top in range(0, height, sub_h)]


@functools.lru_cache(maxsize=None)
def subframe_references(name, rows, cols):
    """A table case's scene cut into rows x cols sub-frames, each an image of its own with the grid points of its own size."""
    early, late, truth_fn, _ = case_scene(name)
    return tuple(crop_reference(early, late, grid_points(w, h)[0], truth_fn, left, top, w, h)
                 for left, top, w, h in subframes(early.shape[1], early.shape[0], rows, cols))


# The sub-frame scenes of the device tests: the 180 x 200 and 61 x 45 cases as 2 x 2 sub-frames, the 96 x 88 pairs of the three-motions
# launch, and 180 x 200 as 1 x 3 for the launch with an empty sub-frame.  The bar from the textbook alone is a condition on them as on the
# table (tests/test_lk_second_opinion.py).  One is left out because it misses that condition: in the 31 x 22 sub-frame of 61x45-shift_1.75_-1
# a judged border track contracts so slowly that the textbook's own cv2-sized stop ends 0.0104 pixel from its fixed point.
THREE_MOTIONS = ('96x88-shift_2.25_-1.5', '96x88-affine', '96x88-homography')
EMPTY_MIDDLE = '180x200-shift_2.25_-1.5'
TWO_BY_TWO = tuple(n for n in CASES if n.startswith(('180x200-', '61x45-')) and n != '61x45-shift_1.75_-1')
SUBFRAME_CASES = tuple((n, 2, 2) for n in TWO_BY_TWO + THREE_MOTIONS) + ((EMPTY_MIDDLE, 1, 3),)


def assert_verdict(ref, moved, found, what):
    """found == 1, |moved - fixed point| <= 0.01 and |moved - truth| <= |fixed point - truth| + 0.01 on every judged point."""
    lost, from_fixed_point, beyond_textbook = ref.verdict(moved, found)
    print('%s: %d judged of %d, %d not found, |moved - fixed point| <= %.4f, |moved - truth| - |fixed point - truth| <= %.4f'
          % (what, ref.judged.sum(), len(ref.judged), lost, from_fixed_point, beyond_textbook))
    assert lost == 0, (what, lost)
    assert from_fixed_point <= BAR, (what, from_fixed_point)
    assert beyond_textbook <= BAR, (what, beyond_textbook)
    return from_fixed_point, beyond_textbook
