"""The specification of the path limiter (`ops.path_limit`; mf_path_limit_f64 in include/meshflow_hip.h): NumPy float64, every operation in the
stated order and rounded by itself -- NumPy fuses nothing, the library is built with -ffp-contract=off --, so the kernel gives these bits.

An online session crops every frame to a rectangle fixed in advance.  The warp puts vertex v of the mesh at g_v + (p_v - c_v): g the vertex
grid (mfs.py:881-906), c and p the unstabilized and the stabilized path.  Where the mesh so placed does not contain the rectangle, border
colour shows.  The limiter scales the correction d = p - c of a whole frame by f = k / K, k the largest step at which the mesh's perimeter
still encloses the rectangle widened by `guard` pixels.

    inputs      per frame t of n: c_t, p_t, (R+1)(C+1)*2 float64 each, `ops.cell_table`'s layout ([row][col][x, y]); per call: W, H, R, C, the
                rectangle (left, top, right, bottom), inclusive, `ops.crop_resize`'s convention; guard >= 0 pixels; steps K in 1 .. 64;
                rise in 1 .. K; an optional carried k_prev (taken as min(max(k_prev, 0), K))
    candidate   k in 1 .. K has f = (double)k / (double)K; vertex v lies at g_v + f * d_v, d_v = p_v - c_v (a subtraction, a multiplication,
                an addition, each rounded); g_v = (ceil((W-1) * (col / C)), ceil((H-1) * (row / R))), integers
    polygon     the mesh's perimeter, B = 2(R + C) vertices: row 0 from column 0 to C-1; column C from row 0 to R-1; row R from column C
                down to 1; column 0 from row R down to 1.  Edge e joins vertex e to vertex (e + 1) mod B.  Interior vertices play no part.
    rectangle   x0 = left - guard, x1 = right + guard, y0 = top - guard, y1 = bottom + guard; centre cx = (x0 + x1) * 0.5, cy alike
    passes      candidate k passes iff (a) and (b):
                (a) every edge (A, B) is CLEAR of the rectangle -- one of these is affirmatively true:
                    its bounding box is disjoint: min(ax, bx) > x1, or max(ax, bx) < x0, or min(ay, by) > y1, or max(ay, by) < y0, with
                    min(a, b) = a < b ? a : b and max(a, b) = a > b ? a : b;
                    the cross products (bx-ax)*(py-ay) - (by-ay)*(px-ax) of the corners (x0,y0), (x1,y0), (x1,y1), (x0,y1) are all > 0;
                    those four are all < 0
                (b) the crossing number of the centre's rightward ray is odd: edge (A, B) counts iff (ay > cy) != (by > cy) and
                    s = (bx-ax)*(cy-ay) - (by-ay)*(cx-ax) has the sign of by - ay (s > 0 when by > ay, else s < 0)
    k_raw_t     the largest k such that every candidate 1 .. k passes (candidate 0, the unstabilized frame, is never tested)
    k_t         min(k_raw_t, k_{t-1} + rise), k_{-1} = k_prev, or K without one: the drop is immediate, the recovery slew-limited.  Closed
                form: k_t = min(K, min_{0 <= i <= t} (k_raw_{t-i} + rise * i), k_prev + rise * (t + 1))
    path        p'_t = p_t bit for bit when k_t == K, c_t bit for bit when k_t == 0, else c + f * (p - c), f = (double)k_t / (double)K

Every predicate is affirmative: a NaN makes no comparison true.  A boundary vertex that is NaN in BOTH coordinates therefore fails every
candidate: it is the B of one edge, whose min, max and cross products are then all NaN.  A NaN in ONE coordinate fails a candidate only
where a test reads it: an edge that the other axis' bounding-box test clears is clear whatever that coordinate holds, so a NaN that runs
ALONG its side of the mesh changes nothing, and the limited path keeps it where k > 0, as the unlimited path would.  An infinity is a
place: it fails where it drags an edge across the rectangle and passes where it carries its vertex away from it.

This limiter is the project's own; the reference has none."""
import math

import numpy as np

MAX_STEPS, MAX_BOUNDARY = 64, 1024


def grid(W, H, R, C):
    """((C+1,) x, (R+1,) y) float64: the vertex grid, integers (`host.vertex_x_y`)."""
    xs = np.array([math.ceil((W - 1) * (col / C)) for col in range(C + 1)], np.float64)
    ys = np.array([math.ceil((H - 1) * (row / R)) for row in range(R + 1)], np.float64)
    return xs, ys


def boundary(R, C):
    """The (B, 2) (row, col) of the perimeter's vertices in the polygon's order."""
    walk = [(0, c) for c in range(C)] + [(r, C) for r in range(R)] + [(R, c) for c in range(C, 0, -1)] + [(r, 0) for r in range(R, 0, -1)]
    return np.array(walk, np.int64)


def check(W, H, R, C, rectangle, guard, steps, rise):
    left, top, right, bottom = rectangle
    if R < 1 or C < 1 or 2 * (R + C) > MAX_BOUNDARY or W < 2 or H < 2:
        raise ValueError('bad mesh or frame size')
    if not (0 <= left <= right <= W - 1 and 0 <= top <= bottom <= H - 1):
        raise ValueError('bad rectangle')
    if not (math.isfinite(guard) and guard >= 0) or not 1 <= steps <= MAX_STEPS or not 1 <= rise <= steps:
        raise ValueError('bad guard, steps or rise')


def passes(c, p, W, H, R, C, rectangle, guard, steps):
    """(K,) bool of one frame: entry k - 1 says whether candidate k passes."""
    c, p = np.asarray(c, np.float64).reshape(R + 1, C + 1, 2), np.asarray(p, np.float64).reshape(R + 1, C + 1, 2)
    left, top, right, bottom = rectangle
    guard = np.float64(guard)
    x0, x1, y0, y1 = left - guard, right + guard, top - guard, bottom + guard
    cx, cy = (x0 + x1) * 0.5, (y0 + y1) * 0.5
    xs, ys = grid(W, H, R, C)
    walk = boundary(R, C)
    gx, gy = xs[walk[:, 1]], ys[walk[:, 0]]
    with np.errstate(invalid='ignore', over='ignore'):
        d = (p - c)[walk[:, 0], walk[:, 1]]                                    # (B, 2)
        f = (np.arange(1, steps + 1, dtype=np.float64) / np.float64(steps))[:, None]
        ax, ay = gx[None] + f * d[None, :, 0], gy[None] + f * d[None, :, 1]     # (K, B)
        bx, by = np.roll(ax, -1, axis=1), np.roll(ay, -1, axis=1)
        lo_x, hi_x = np.where(ax < bx, ax, bx), np.where(ax > bx, ax, bx)
        lo_y, hi_y = np.where(ay < by, ay, by), np.where(ay > by, ay, by)
        clear = (lo_x > x1) | (hi_x < x0) | (lo_y > y1) | (hi_y < y0)
        ex, ey = bx - ax, by - ay
        cross = [ex * (py - ay) - ey * (px - ax) for px, py in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
        clear |= (cross[0] > 0) & (cross[1] > 0) & (cross[2] > 0) & (cross[3] > 0)
        clear |= (cross[0] < 0) & (cross[1] < 0) & (cross[2] < 0) & (cross[3] < 0)
        s = ex * (cy - ay) - ey * (cx - ax)
        counts = ((ay > cy) != (by > cy)) & np.where(by > ay, s > 0, s < 0)
    return clear.all(axis=1) & (counts.sum(axis=1) % 2 == 1)


def k_raw(c, p, W, H, R, C, rectangle, guard, steps):
    """k_raw of one frame: the number of leading candidates that pass."""
    ok = passes(c, p, W, H, R, C, rectangle, guard, steps)
    return int(steps if ok.all() else np.argmin(ok))


def slew(raw, steps, rise, k_prev=None):
    """(n,) int32 k from (n,) k_raw, by the recurrence."""
    before = steps if k_prev is None else min(max(int(k_prev), 0), steps)
    out = np.empty(len(raw), np.int32)
    for t, r in enumerate(raw):
        before = out[t] = min(int(r), before + rise)
    return out


def slew_closed(raw, steps, rise, k_prev=None):
    """The same by the closed form, the way the kernel evaluates it: the terms i <= 63 only (a term at i >= 64 is >= rise * 64 >= K)."""
    raw = [int(r) for r in raw]
    out = np.empty(len(raw), np.int32)
    for t in range(len(raw)):
        terms = [steps] + [raw[t - i] + rise * i for i in range(min(t, 63) + 1)]
        if k_prev is not None and t + 1 <= 63:
            terms.append(min(max(int(k_prev), 0), steps) + rise * (t + 1))
        out[t] = min(terms)
    return out


def apply(c, p, k, steps):
    """The limited path of one frame."""
    c, p = np.asarray(c, np.float64), np.asarray(p, np.float64)
    if k == steps:
        return p.copy()
    if k == 0:
        return c.copy()
    with np.errstate(invalid='ignore', over='ignore'):
        return c + (np.float64(k) / np.float64(steps)) * (p - c)


def limit(unstab, stab, W, H, R, C, rectangle, steps=32, guard=2.0, rise=2, k_prev=None):
    """(limited (n, S) float64, k (n,) int32, k_raw (n,) int32) of n frames."""
    check(W, H, R, C, rectangle, guard, steps, rise)
    S = (R + 1) * (C + 1) * 2
    c, p = np.ascontiguousarray(unstab, np.float64).reshape(-1, S), np.ascontiguousarray(stab, np.float64).reshape(-1, S)
    raw = np.array([k_raw(c[t], p[t], W, H, R, C, rectangle, guard, steps) for t in range(len(c))], np.int32)
    k = slew(raw, steps, rise, k_prev)
    return np.stack([apply(c[t], p[t], int(k[t]), steps) for t in range(len(c))]), k, raw
