"""Homographies for the feature scores' tests and for tools/scores_dump_cases.py: the planted matrices -- one per branch of
tests/scores_model.py and of the reference's arithmetic --, the matrices whose scores are infinities or NaNs, and launches of any length
made of the planted ones and seeded perturbations of them."""
import numpy as np


def matrix(a, b, c, d, tx=0.0, ty=0.0, g=0.0, h=0.0):
    return np.array([[a, b, tx], [c, d, ty], [g, h, 1.0]], np.float64)


def rotation(scale, degrees, tx=0.0, ty=0.0):
    t = np.deg2rad(degrees)
    return matrix(scale * np.cos(t), -scale * np.sin(t), scale * np.sin(t), scale * np.cos(t), tx, ty)


def planted():
    """[(name, H)]: finite matrices with a non-zero h00 h11, every branch of the specification among them."""
    return [
        ('identity', np.identity(3)),
        ('similarity without rotation', matrix(1.25, 0.0, 0.0, 1.25, -16.0, -12.0)),
        ('similarity, 0.5 degrees (complex pair)', rotation(1.15, 0.5, 3.0, -2.0)),
        ('similarity, 30 degrees (complex pair)', rotation(0.9, 30.0)),
        ('rotation only (complex pair on the unit circle)', rotation(1.0, 2.0)),
        ('anisotropic scale', matrix(1.2, 0.0, 0.0, 1.1, -8.0, 5.0)),
        ('shear (double eigenvalue 1)', matrix(1.0, 0.3, 0.0, 1.0)),
        ('scale and shear', matrix(1.1, 0.2, 0.0, 0.95, 1.0, 1.0)),
        ('both block eigenvalues below 1', matrix(0.8, 0.05, 0.02, 0.7)),
        ('both block eigenvalues above 1', matrix(1.2, 0.01, 0.03, 1.5)),
        ('one on each side of 1', matrix(1.3, 0.02, 0.01, 0.8)),
        ('negative determinant', matrix(1.1, 0.3, 0.4, -0.9)),
        ('negative trace (m < 0)', matrix(-1.1, 0.1, 0.2, -0.9)),
        ('double eigenvalue up to 1e-9, real', matrix(1.1, 1e-9, 1e-9, 1.1)),
        ('double eigenvalue up to 1e-9, complex', matrix(1.1, 1e-9, -1e-9, 1.1)),
        ('double eigenvalue below 1 up to 1e-9', matrix(0.9, 2e-9, 0.5e-9, 0.9)),
        ('small projective terms', matrix(1.14, 0.004, -0.003, 1.16, -9.1, -6.7, 1e-5, -2e-5)),
        ('a crop of 1.15 per axis as the tracker fits it', matrix(1.1428571, 1.3e-4, -2.1e-4, 1.1428571, -9.14, -6.86, 3e-7, -1e-7)),
        ('tiny scales', matrix(1e-3, 1e-5, 2e-5, 3e-3)),
        ('large scales', matrix(40.0, 3.0, -2.0, 25.0)),
    ]


def special():
    """[(name, H)]: where IEEE decides -- infinities and NaNs that nothing refuses."""
    nan, inf = float('nan'), float('inf')
    return [
        ('zero block (big == 0; 1 / 0)', matrix(0.0, 0.0, 0.0, 0.0)),
        ('h00 == 0', matrix(0.0, 1.0, 1.0, 1.0)),
        ('h11 == -0.0', matrix(2.0, 0.5, 0.5, -0.0)),
        ('complex pair, zero trace', matrix(1.0, 3.0, -1.0, -1.0)),
        ('NaN in h00', matrix(nan, 0.0, 0.0, 1.0)),
        ('NaN in h01', matrix(1.0, nan, 0.1, 1.0)),
        ('infinite h00', matrix(inf, 0.0, 0.0, 1.0)),
        ('infinite h00 and h11', matrix(inf, 1.0, 1.0, inf)),
        ('overflowing product', matrix(1e200, 0.0, 0.0, 1e200)),
        ('underflowing product', matrix(1e-200, 0.0, 0.0, 1e-200)),
        ('float32 overflow of the ratio', matrix(1e-20, 0.0, 0.0, 1e-20)),
    ]


def launch(pairs, seed=7):
    """(pairs, 3, 3) float64: the planted matrices in turn, from the second round on with seeded perturbations of their block (legacy
    RandomState: its stream never changes)."""
    base = [h for _, h in planted()]
    rng = np.random.RandomState(seed)
    out = np.empty((pairs, 3, 3), np.float64)
    for p in range(pairs):
        out[p] = base[p % len(base)]
        if p >= len(base):
            out[p, :2, :2] += rng.uniform(-0.02, 0.02, (2, 2))
            out[p, :2, 2] += rng.uniform(-3.0, 3.0, 2)
    return out


def record(pairs, refused):
    """A fit record (pairs, 4) int32 as `ops.fit_homographies` leaves it: status 0 but for the pairs in `refused` (statuses 1-4 in turn)."""
    info = np.zeros((pairs, 4), np.int32)
    info[:, 1] = 100
    for i, p in enumerate(refused):
        info[p] = (1 + i % 4, 0, 0, 0)
    return info
