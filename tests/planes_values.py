"""Float32 planes seeded with the values real side planes carry and N(0, 1000) data never shows a kernel -- NaN, infinities, -0.0, subnormals,
values near FLT_MAX -- and the comparison rule and census the tests of tests/test_planes_model.py and tests/test_gpu_planes_values.py share.

Isolated specials sit among samples near 1000, where a subnormal or an overflowing RESULT cannot arise; those come from three solid blocks
(subnormals of mixed sign, magnitudes 2.5e38 .. FLT_MAX of mixed sign, +-0.0 mixed), placed by the caller where its maps or its crop put
output pixels whose whole footprint lies inside a block."""
import numpy as np

F32 = np.float32
FLT_MAX = np.finfo(F32).max
FLT_MIN = np.finfo(F32).tiny
SMALLEST = np.array([1], np.uint32).view(F32)[0]                       # 2^-149, the smallest subnormal
QNAN = np.array([0x7FC00000], np.uint32).view(F32)[0]
SPECIALS = np.array([QNAN, np.inf, -np.inf, -0.0, SMALLEST, -1e-40, FLT_MIN, FLT_MAX, -FLT_MAX, 3e38], F32)
BLOCK = 8                                                               # block edge: covers a 2 x 2 footprint at every scale the tests use
CLASSES = ('nan', '+inf', '-inf', '-0.0', 'subnormal', 'huge')


def block(kind, rng, h=BLOCK, w=BLOCK):
    """One solid block of a class: 'sub' subnormals of mixed sign, 'huge' 2.5e38 .. FLT_MAX of mixed sign, 'zero' +-0.0 mixed (three in four
    negative: a -0.0 result needs all four products to be -0.0)."""
    if kind == 'sub':
        mant = rng.integers(1, 1 << 23, (h, w)).astype(np.uint32)
        return (mant | (rng.integers(0, 2, (h, w)).astype(np.uint32) << 31)).view(F32)
    if kind == 'huge':
        mag = rng.uniform(2.5e38, float(FLT_MAX), (h, w)).astype(F32)
        mag[0, 0] = FLT_MAX
        return np.where(rng.integers(0, 2, (h, w)) == 1, -mag, mag).astype(F32)
    assert kind == 'zero'
    return np.where(rng.integers(0, 4, (h, w)) > 0, F32(-0.0), F32(0.0)).astype(F32)


def seed(plane, rng, blocks, share=0.02):
    """`plane` (H, W) float32, in place: `share` of the samples overwritten by SPECIALS in turn, one special within two pixels of each edge,
    then the three blocks with their top-left corners at blocks = {'sub': (y, x), 'huge': (y, x), 'zero': (y, x)}."""
    H, W = plane.shape
    k = max(int(round(share * H * W)), len(SPECIALS))
    pos = rng.choice(H * W, k, replace=False)
    plane.reshape(-1)[pos] = SPECIALS[np.arange(k) % len(SPECIALS)]
    if H >= 6 and W >= 6:
        plane[1, W // 3], plane[H - 2, W // 2], plane[H // 3, 0], plane[H // 2, W - 1] = np.inf, -np.inf, QNAN, np.inf
        plane[0, 2 * W // 3], plane[H - 1, W // 4], plane[2 * H // 3, 1], plane[H // 4, W - 2] = F32(-0.0), SMALLEST, FLT_MAX, F32(-0.0)
    for kind, (y, x) in blocks.items():
        y, x = min(max(int(y), 0), H - BLOCK), min(max(int(x), 0), W - BLOCK)
        plane[y:y + BLOCK, x:x + BLOCK] = block(kind, rng)
    return plane


def census(a, huge_above=1e38):
    """How often each class occurs in a float32 array."""
    a = np.ascontiguousarray(a, dtype=F32)
    bits = a.view(np.uint32)
    mag = bits & np.uint32(0x7FFFFFFF)
    return {'nan': int(np.isnan(a).sum()), '+inf': int((bits == 0x7F800000).sum()), '-inf': int((bits == 0xFF800000).sum()),
            '-0.0': int((bits == 0x80000000).sum()), 'subnormal': int(((mag > 0) & (mag < 0x00800000)).sum()),
            'huge': int(((mag > np.array([huge_above], F32).view(np.uint32)[0]) & (mag < 0x7F800000)).sum()), 'size': int(a.size)}


def assert_covers(a, what, nan_cap=0.05, huge_above=1e38):
    """From the model alone: every class occurs in `a`, and NaN (where only NaN-ness is compared) stays under `nan_cap` of it."""
    c = census(a, huge_above)
    print(what, c)
    assert all(c[k] >= 1 for k in CLASSES), (what, c)
    assert c['nan'] <= nan_cap * c['size'], (what, c)
    return c


def mismatches(got_bits, want):
    """The comparison rule.  got_bits: uint32; want: the model's float32.  Where the model is not NaN the bits must be equal; where it is NaN the
    result must be a NaN of any sign and payload.  Returns the boolean array of violations."""
    want = np.ascontiguousarray(want, dtype=F32)
    got_bits = np.ascontiguousarray(got_bits, dtype=np.uint32)
    assert got_bits.shape == want.shape, (got_bits.shape, want.shape)
    nan = np.isnan(want)
    return np.where(nan, ~np.isnan(got_bits.view(F32)), got_bits != want.view(np.uint32))
