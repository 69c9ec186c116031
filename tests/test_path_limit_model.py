"""tests/path_limit_model.py, the path limiter's specification, by itself: answers that can be worked out by hand, the slew recurrence against
its closed form, and -- through the C oracle's warp and crop scan, with nothing of the kernels involved -- the condition the GPU session test
rests on: the model's limited paths are `covered`, on tests/path_limit_fields.py's set.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import path_limit_fields as pf  # noqa: E402
import path_limit_model as pm  # noqa: E402

W, H = 128, 96
RECT = (10, 7, 117, 88)
K = 32


def translation(R, C, dx, dy):
    """(c, p) of one frame: p - c = (dx, dy) at every vertex, on a c that is not zero."""
    c = np.linspace(-3.0, 4.0, (R + 1) * (C + 1) * 2)
    p = c.reshape(-1, 2) + np.array([dx, dy], np.float64)
    # (make the difference exactly (dx, dy): c + d - c may round)
    c = p - np.array([dx, dy], np.float64)
    assert np.array_equal(p - c, np.broadcast_to([dx, dy], p.shape))
    return c.reshape(-1), p.reshape(-1)


@pytest.mark.parametrize('mesh', [(1, 1), (4, 4), (3, 1)])
@pytest.mark.parametrize('shift', [(16, 0), (-16, 0), (0, 10), (0, -10)])
def test_a_translation_stops_strictly_before_the_guarded_side(mesh, shift):
    """Guarded rectangle (8, 5, 119, 90) in a frame (0, 0, 127, 95): 8 px of room sideways, 5 px vertically.  f * 16 < 8 and f * 10 < 5 hold
    strictly for k <= 15 of 32: at k = 16 the frame's edge lies ON the guarded side, and an edge on it is not clear."""
    R, C = mesh
    c, p = translation(R, C, *shift)
    assert pm.k_raw(c, p, W, H, R, C, RECT, 2.0, K) == 15
    ok = pm.passes(c, p, W, H, R, C, RECT, 2.0, K)
    assert ok[:15].all() and not ok[15:].any()
    limited, k, raw = pm.limit(c[None], p[None], W, H, R, C, RECT, K, 2.0, 2)
    assert k.dtype == np.int32 and k.tolist() == [15] and raw.tolist() == [15]
    assert limited[0].tobytes() == (c + (np.float64(15) / np.float64(32)) * (p - c)).tobytes()
    # guard 0: 10 px sideways, 7 vertically -- f * 16 < 10 for k <= 19, f * 10 < 7 for k <= 22
    assert pm.k_raw(c, p, W, H, R, C, RECT, 0.0, K) == (19 if shift[0] else 22)


def test_no_correction_is_step_K_and_the_stabilized_bits():
    R, C = 4, 4
    c = np.linspace(-5.0, 5.0, 50)
    limited, k, raw = pm.limit(np.stack([c, c]), np.stack([c, c]), W, H, R, C, RECT, K, 2.0, 2)
    assert k.tolist() == [K, K] and raw.tolist() == [K, K] and limited.tobytes() == np.stack([c, c]).tobytes()
    # k == K hands p through whatever it holds; -0.0 stays -0.0
    p = c.copy()
    p[0] = -0.0
    c2 = p.copy()
    c2[0] = 0.0
    limited, k, _ = pm.limit(c2[None], p[None], W, H, R, C, RECT, K, 2.0, 2)
    assert k.tolist() == [K] and limited[0].tobytes() == p.tobytes()


def test_not_a_number():
    R, C = 4, 4
    c, p = translation(R, C, 3, 2)
    assert pm.k_raw(c, p, W, H, R, C, RECT, 2.0, K) == K
    grid = p.reshape(R + 1, C + 1, 2)
    for row, col in ((0, 2), (2, 4), (4, 1), (3, 0), (0, 0), (4, 4)):                  # every side and two corners: both coordinates
        q = grid.copy()
        q[row, col] = np.nan
        limited, k, _ = pm.limit(c[None], q.reshape(1, -1), W, H, R, C, RECT, K, 2.0, 2)
        assert k.tolist() == [0] and limited[0].tobytes() == c.tobytes(), (row, col)
    # an infinity is a place, not a NaN: one that carries a vertex across the rectangle fails, one that carries it away from the rectangle
    # leaves a polygon that still encloses it
    for (row, col), bad, want in (((0, 2), (np.inf, np.inf), 0), ((0, 2), (-np.inf, -np.inf), K), ((2, 4), (-np.inf, 0.0), 0),
                                  ((4, 4), (np.inf, np.inf), K), ((4, 4), (-np.inf, -np.inf), 0)):
        q = grid.copy()
        q[row, col] = bad
        assert pm.k_raw(c, q.reshape(-1), W, H, R, C, RECT, 2.0, K) == want, (row, col, bad)
    # an interior vertex plays no part
    for row, col in ((1, 1), (2, 2), (3, 1)):
        q = grid.copy()
        q[row, col] = np.nan
        limited, k, _ = pm.limit(c[None], q.reshape(1, -1), W, H, R, C, RECT, K, 2.0, 2)
        assert k.tolist() == [K] and limited[0].tobytes() == q.tobytes()
    # the model's docstring: a NaN in ONE coordinate fails only where a test reads it -- along the top side x is not read (both edges are
    # cleared by their y extent), y is read by the edge that ends at the vertex (its min and max are then NaN); on the right side the centre's
    # ray reads y as well
    for (row, col, axis), want in (((0, 2, 0), K), ((0, 2, 1), 0), ((4, 1, 0), K), ((4, 1, 1), 0), ((2, 4, 0), 0), ((2, 4, 1), 0)):
        q = grid.copy()
        q[row, col, axis] = np.nan
        assert pm.k_raw(c, q.reshape(-1), W, H, R, C, RECT, 2.0, K) == want, (row, col, axis)


def test_a_mirrored_mesh_collapses_on_the_way():
    """p reflects the grid left to right: vertex x = gx + f (127 - 2 gx).  The left side is at 127 f, the right one at 127 - 127 f; both
    are clear of (8, 119) while 127 f < 8, k <= 2 of 32 -- the mesh never gets as far as turning over."""
    for R, C in ((1, 1), (4, 4)):
        xs, _ = pm.grid(W, H, R, C)
        c = np.zeros((R + 1, C + 1, 2))
        p = c.copy()
        p[..., 0] = (W - 1) - 2 * xs[None, :]
        assert pm.k_raw(c.reshape(-1), p.reshape(-1), W, H, R, C, RECT, 2.0, K) == 2
        # the mirror image alone (f = 1 only) encloses the rectangle with every cross product negative: the model does pass it
        assert pm.passes(c.reshape(-1), p.reshape(-1), W, H, R, C, RECT, 2.0, 1).tolist() == [True]


def test_the_boundary_walk():
    assert pm.boundary(1, 1).tolist() == [[0, 0], [0, 1], [1, 1], [1, 0]]
    assert pm.boundary(1, 2).tolist() == [[0, 0], [0, 1], [0, 2], [1, 2], [1, 1], [1, 0]]
    assert pm.boundary(3, 1).tolist() == [[0, 0], [0, 1], [1, 1], [2, 1], [3, 1], [3, 0], [2, 0], [1, 0]]
    for R, C in ((16, 16), (256, 256), (1, 511)):
        walk = pm.boundary(R, C)
        assert len(walk) == 2 * (R + C) == len({tuple(v) for v in walk.tolist()})
        assert all(r in (0, R) or col in (0, C) for r, col in walk.tolist())
    from meshflow_amd import host
    xs, ys = pm.grid(W, H, 16, 16)
    want = host.vertex_x_y(W, H, 16, 16).reshape(17, 17, 2)
    assert np.array_equal(xs, want[0, :, 0]) and np.array_equal(ys, want[:, 0, 1])


def test_the_slew_recurrence_is_its_closed_form():
    rng = np.random.default_rng(5)
    n, steps = 130, 64
    planted = np.full(n, steps)
    planted[0] = 0                                                     # the recovery needs the whole 64-frame look-back, and crosses it
    assert pm.slew(planted, steps, 1).tolist() == [min(t, steps) for t in range(n)]
    for raw in (planted, rng.integers(0, steps + 1, n), np.where(rng.random(n) < 0.05, rng.integers(0, 20, n), steps)):
        for rise in (1, 2, 7, 64):
            for k_prev in (None, 0, 5, 64):
                a, b = pm.slew(raw, steps, rise, k_prev), pm.slew_closed(raw, steps, rise, k_prev)
                assert a.tolist() == b.tolist(), (rise, k_prev)
                assert (np.diff(a) <= rise).all() and (a <= raw).all()
    # the carry: a chain of calls equals one call
    raw = rng.integers(0, steps + 1, n)
    whole = pm.slew(raw, steps, 2)
    first = pm.slew(raw[:1], steps, 2)
    second = pm.slew(raw[1:4], steps, 2, first[-1])
    rest = pm.slew(raw[4:], steps, 2, second[-1])
    assert np.concatenate([first, second, rest]).tolist() == whole.tolist()
    assert pm.slew([64, 64], 64, 1, k_prev=-7).tolist() == [1, 2] and pm.slew([64], 64, 1, k_prev=900).tolist() == [64]     # clamped


def test_the_refusals():
    c = np.zeros((1, 8))
    for kw in (dict(R=0), dict(C=0), dict(R=256, C=257), dict(W=1), dict(H=1), dict(rectangle=(-1, 7, 117, 88)), dict(rectangle=(10, 7, 128, 88)),
               dict(rectangle=(11, 7, 10, 88)), dict(rectangle=(10, 7, 117, 96)), dict(steps=0), dict(steps=65), dict(rise=0), dict(rise=33),
               dict(guard=-0.5), dict(guard=float('nan')), dict(guard=float('inf'))):
        a = dict(dict(W=W, H=H, R=1, C=1, rectangle=RECT, steps=K, guard=2.0, rise=2), **kw)
        with pytest.raises(ValueError):
            pm.limit(c, c, **a)


@pytest.fixture(scope='module')
def proven():
    """Every case of the shared set through the model and the C oracle, once: [(R, C, margin, covered before, covered after, k)]."""
    from oracle import clib
    out = []
    for R, C, margin, rect, c, p in pf.cases():
        frames = np.full((len(c), H, W, 3), 200, np.uint8)
        shape = (len(c), R + 1, C + 1, 2)
        _, crop, bad = clib.warp_clip(frames, R, C, c.reshape(shape), p.reshape(shape))
        assert bad == 0
        limited, k, _ = pm.limit(c, p, W, H, R, C, rect, pf.STEPS, pf.GUARD, pf.STEPS)             # rise = K: every frame by itself
        warped, crop2, bad = clib.warp_clip(frames, R, C, c.reshape(shape), limited.reshape(shape))
        assert bad == 0
        inside = warped[:, rect[1]:rect[3] + 1, rect[0]:rect[2] + 1]
        out.append((R, C, margin, pf.covered(crop, rect), pf.covered(crop2, rect), k, bool((inside == 200).all())))
    return out


def test_the_limited_path_is_covered_in_every_case(proven):
    before = np.concatenate([case[3] for case in proven])
    share = 1.0 - before.mean()
    print('uncovered before limiting: %d of %d frames (%.0f %%)' % ((~before).sum(), before.size, 100 * share))
    assert share >= 0.25                                               # the set exercises the limiter
    for R, C, margin, was, now, k, clean in proven:
        print('mesh %dx%d margin %.2f: uncovered %d -> %d of %d, mean k / K %.3f' % (R, C, margin, (~was).sum(), (~now).sum(), now.size,
                                                                                    k.mean() / pf.STEPS))
        assert now.all(), (R, C, margin, np.nonzero(~now)[0].tolist())
        assert clean, (R, C, margin)                                   # no border pixel inside the rectangle
        assert (k[was] >= 1).all()                                     # (a frame that was covered is not thrown back to the raw frame)
    ks = np.concatenate([case[5] for case in proven])
    print('mean k / K over the set: %.3f; frames limited: %d of %d' % (ks.mean() / pf.STEPS, (ks < pf.STEPS).sum(), ks.size))
