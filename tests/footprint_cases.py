"""One geometry table for the warps that take the plan's hot and pair shortcuts without an LDS window (warp_body.h, NOWIN): the coordinate
maps, the float32 and label side planes, P010 luma and the NV12 / P010 chroma planes.  Made on the CPU, no HIP library: per case the motion,
the reference's maps (C oracle), noise planes in every format, every format's expected output from the existing models, and -- for the four
formats whose tail chooses per wavefront between a fast deep-interior form and a clamped one (warp_tails.h) -- which form each footprint
takes.  Computed once per case, shared, never changed.

Every case has an even W and H with W % 4 == 0 (one table serves the 4:2:0 formats, and a frame with W % 4 != 0 holds no staged, hence no hot
or pair, footprint) and is at most 288 x 512: a hot footprint needs a cell wider than a footprint, not a large frame.  Which plan classes a
case holds can only be read from the device's plan (tests/test_gpu_footprint_paths.py decodes it); the comments below give what was counted
there."""
import numpy as np

import cv16_model
import nv12_model
import p010_model
import planes_model
import plan_words

F32 = np.float32
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
# fill values of the label planes per element size, as the signed dtype's own number and as its bits; the random data never holds them
FILL = {1: (231, 231), 2: (-4083, 0xF00D), 4: (-559038737, 0xDEADBEEF), 8: (-81985529216486896, 0xFEDCBA9876543210)}
DATA_TOP = {1: 200, 2: 60000, 4: 2 ** 31, 8: 2 ** 63}
FILL_F32 = -777.25
BORDER_NV12 = (19, 203, 77)            # no default anywhere: Y, U and V all differ
BORDER_P010 = (4660, 51966, 300)       # ... and exceed 255

# synthetic.motion's arguments per kind (test_gpu_warp_maps.CASES' vocabulary, plus 'still' and 'wide'); a kind ('translate', shifts) is no
# random motion: stab - unstab = shifts[f] on every vertex of frame f, so output pixel (x, y) samples (x - dx, y - dy) of a mesh moved as a whole;
# a kind ('shear', offsets): unstab - stab = (2^-18 gy + bx, by) on the vertices of grid row gy of frame f, offsets[f] = (bx, by) -- a shear's
# inverse is a shear, so the top-left cell's inverse homography is exact: u = x + 2^-18 (y + by) + bx, v = y + by
KINDS = {
    'jitter': {},
    'shift': dict(translation_sigma=12.0),                       # large global translation: wide border rings, many uncovered pixels
    'stress': dict(translation_sigma=20.0, field_sigma=8.0),    # a strong smooth field on top: far-from-affine cells, long candidate lists
    'still': dict(translation_sigma=2.5, field_sigma=0.1),      # hardly more than a pixel of motion: deep-interior tails inside the outermost ring
    'wide': dict(translation_sigma=30.0),
}

# F, H, W, R, C, jitter, kind, seed.  Behind each case: the footprints per plan class as the MI355X's plan gave them (hot = FAST64 + plain).
CASES = [
    # the even geometries of test_gpu_warp_maps.CASES: cells below or near a footprint -- overflow lists, and the general path's long lists
    (3, 72, 100, 3, 5, 6.0, 'jitter', 75),                 # 13 overflow, 95 other (W % 32 = 4: the last column of footprints overhangs)
    (3, 144, 256, 8, 8, 2.0, 'shift', 152),                # 20 pair, 5 multi, 144 overflow, 263 other
    (4, 144, 256, 16, 16, 4.0, 'stress', 11),              # 576 overflow
    (2, 96, 128, 32, 32, 0.5, 'jitter', 130),              # 96 overflow
    (3, 128, 128, 64, 64, 0.05, 'jitter', 13),             # 192 overflow
    (2, 288, 512, 32, 32, 1.0, 'shift', 514),              # 1152 overflow
    # cells well above 32 x 8: hot footprints of both coordinate chains, pairs along the cell edges, multi around the vertices
    (3, 144, 256, 2, 2, 1.0, 'jitter', 21),                # 275 hot, 44 pair, 3 multi, 104 border, 6 other
    (3, 144, 256, 4, 4, 2.0, 'jitter', 22),                # 55 hot, 88 pair, 41 multi, 40 border, 208 other
    (3, 144, 256, 4, 4, 0.2, 'still', 24),                 # 134 hot, 127 pair, 43 multi, 95 border, 33 other: fast tails inside the ring
    (3, 144, 256, 4, 4, 1.0, 'wide', 24),                  # 77 hot, 132 pair, 42 multi, 37 border, 144 other
    # small translations: hot and pair footprints whose sources lie 1.5 to 3 pixels from the top and left edges -- the clamped tail on the
    # full-resolution planes (source column or row 1) and, with the fast tail there, on the chroma planes
    (3, 144, 256, 2, 2, 1.5, ('translate', ((-1.5, -1.5), (2.5, 1.5), (-3.0, -2.0))), 25),     # 288 hot (32 plain), 66 pair, 69 border
    # wide translations: hot footprints without FAST64 (the numerators' terms cancel: x - 100 against x + 100)
    (2, 144, 256, 2, 2, 1.5, ('translate', ((100.25, 3.0), (-90.5, 40.0))), 26),               # 92 hot (20 plain), 33 pair, 40 border, 120 other
    # cells of 16 x 18 pixels under the same small translations: two to four cells per footprint along the top and left edges
    (3, 144, 256, 8, 16, 1.0, ('translate', ((-1.5, -1.5), (2.5, 1.5), (-3.0, -2.0))), 31),    # 182 multi (16 with the clamped tail), 250 other
    # u = x + 2^-18 (y + by) + bx with a half-integer by: in every second row, wherever 32 <= u < 64, exactly half way between two float32
    # numbers -- the cheap coordinate chain must refuse on every such footprint (cheap_chain_must_refuse)
    (2, 144, 256, 2, 2, 0.0, ('shear', ((1.5, 1.5), (2.5, -1.5))), 41),                        # 192 hot, 16 of them FAST64 that must refuse
]
MIDPOINT = '256x144_2x2_shear_41'


def name_of(case):
    F, H, W, R, C, jitter, kind, seed = case
    return '%dx%d_%dx%d_%s_%d' % (W, H, R, C, kind if isinstance(kind, str) else kind[0], seed)


NAMES = [name_of(c) for c in CASES]
BY_NAME = dict(zip(NAMES, CASES))
assert len(BY_NAME) == len(CASES)
FORMATS = ('maps', 'plane_f32', 'plane_n1', 'plane_n2', 'plane_n4', 'plane_n8', 'u16c1', 'nv12_uv', 'p010_uv')
# the formats whose tail has a fast and a clamped form, and the plane whose size the tail's deep-interior test takes
TWO_FORM_TAILS = {'plane_f32': 'luma', 'u16c1': 'luma', 'nv12_uv': 'chroma', 'p010_uv': 'chroma'}
_CASES = {}


def motion(case):
    """(unstab, stab) vertex displacements (F, R + 1, C + 1, 2) float64 of a case."""
    from meshflow_amd import synthetic
    from oracle import meshflow_oracle as mo
    F, H, W, R, C, jitter, kind, seed = case
    if not isinstance(kind, str) and kind[0] == 'shear':
        assert len(kind[1]) == F and jitter == 0.0
        gy = mo.vertex_x_y(W, H, R, C).reshape(R + 1, C + 1, 2)[:, :, 1].astype(np.float64)
        disp = np.zeros((F, R + 1, C + 1, 2))
        for f, (bx, by) in enumerate(kind[1]):
            disp[f, :, :, 0], disp[f, :, :, 1] = gy * 2.0 ** -18 + bx, by
        return disp, np.zeros_like(disp)
    if not isinstance(kind, str):
        assert kind[0] == 'translate' and len(kind[1]) == F
        disp = np.random.default_rng(seed).normal(0, jitter, (F, R + 1, C + 1, 2))
        return disp, disp + np.asarray(kind[1], np.float64)[:, None, None, :]
    disp, hom = synthetic.motion(F, R, C, seed=seed, jitter_sigma=jitter, **KINDS[kind])
    return disp, mo.stabilized_vertex_displacements(W, H, 0, disp, hom, 3, 10)


def deep_interior(u, v, W, H):
    """warp_coords.h's deep_interior per sample, restated from its own words: bx = the raw bits of the float32 fma(u, 32, 1.5 * 2^23) (one
    rounding, to nearest even: fixed_point), and the sample is deep where W >= 5, H >= 5 and, as unsigned 32-bit numbers,
    bx - (0x4B400000 + 64) <= 32 (W - 3) + 31 - 64, the same for by with H -- i.e. 2 <= ix <= W - 3 and 2 <= iy <= H - 3 for ix = rint(32 u) >> 5,
    and no coordinate out of the trick's range."""
    def raw(c):
        with np.errstate(over='ignore', invalid='ignore'):
            # (32 u is exact in float64 and so is the sum: the cast rounds once, like the fma)
            return (np.asarray(c, F32).astype(np.float64) * 32.0 + 12582912.0).astype(F32).view(np.uint32)
    if W < 5 or H < 5:
        return np.zeros(np.shape(u), bool)
    with np.errstate(over='ignore'):                                    # (uint32: wraps like the kernel's)
        dx = raw(u) - np.uint32(0x4B400000 + 64)
        dy = raw(v) - np.uint32(0x4B400000 + 64)
    return (dx <= np.uint32(32 * (W - 3) + 31 - 64)) & (dy <= np.uint32(32 * (H - 3) + 31 - 64))


def per_footprint_all(mask):
    """all() of a per-pixel mask (F, H, W) over each 32 x 8 footprint -> (F, ceil(H / 8), ceil(W / 32)); pixels beyond the frame count as True."""
    F, H, W = mask.shape
    nfy, nfx = (H + plan_words.FOOT_H - 1) // plan_words.FOOT_H, (W + plan_words.FOOT_W - 1) // plan_words.FOOT_W
    full = np.ones((F, nfy * plan_words.FOOT_H, nfx * plan_words.FOOT_W), bool)
    full[:, :H, :W] = mask
    return full.reshape(F, nfy, plan_words.FOOT_H, nfx, plan_words.FOOT_W).all(axis=(2, 4))


def per_footprint_any(mask):
    return ~per_footprint_all(~np.asarray(mask, bool))


def tail_fast_map(mx, my, W, H, plane):
    """Per footprint (F, ceil(H / 8), ceil(W / 32)): True where the tail takes its FAST form -- every emitting sample of the wavefront is deep
    interior by the tail's own test on its own plane.  plane 'luma' (remap_store_plane_f32, remap_store_u16c1): every pixel of the footprint
    inside the frame emits, tested at (u, v) on (W, H).  plane 'chroma' (remap_store_chroma for NV12 and P010): the even pixels of the even
    rows emit, tested at (u / 2, v / 2) -- halved in float32 -- on (W / 2, H / 2); the other pixels' coordinates take no part."""
    if plane == 'luma':
        return per_footprint_all(deep_interior(mx, my, W, H))
    assert plane == 'chroma' and W % 4 == 0 and H % 2 == 0               # (W % 4 == 0: every lane holds two samples)
    deep = np.ones(mx.shape, bool)
    deep[:, ::2, ::2] = deep_interior(mx[:, ::2, ::2] * F32(0.5), my[:, ::2, ::2] * F32(0.5), W // 2, H // 2)
    return per_footprint_all(deep)


# warp_coords.h: the cheap float64 chain's result is dropped (the wavefront redoes its coordinates with the exact chain) when the low 29
# mantissa bits of any of its values lie within FAST64_WINDOW of 0x10000000, the pattern of a float32 rounding midpoint; the window is 4.3 x
# the chain's certified distance from the exact chain's value, i.e. that bound is below 120 float64 ulps
FAST64_WINDOW, FAST64_BOUND_ULPS = 512, 120


def cheap_chain_must_refuse(records, owner, H, W):
    """Per footprint (F, ceil(H / 8), ceil(W / 32)): True where cell_coords_fast, if the plan lets it run on the footprint's cell `owner`
    (same shape), MUST refuse at run time.  records: the oracle's cell records (F, R C, 32), whose doubles 9 .. 17 are the inverse
    homography.  The exact chain's u = ((x h0 + y h1) + h2) / ((x h6 + y h7) + h8), v alike, in float64; where the low 29 mantissa bits of one
    of them lie within FAST64_WINDOW - FAST64_BOUND_ULPS - 8 of 0x10000000 (8: this division against the kernel's reciprocal), the cheap
    chain's value -- at most the bound away -- lies inside the window, and one such value sends the whole wavefront to the exact chain."""
    F = records.shape[0]
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    hi = records[np.arange(F)[:, None, None], plan_words.per_pixel(owner, H, W)][..., 9:18]      # (F, H, W, 9): each pixel's footprint's cell
    w = (xs * hi[..., 6] + ys * hi[..., 7]) + hi[..., 8]
    near = np.zeros((F, H, W), bool)
    for a, b, c in ((0, 1, 2), (3, 4, 5)):
        value = np.ascontiguousarray(((xs * hi[..., a] + ys * hi[..., b]) + hi[..., c]) / w)
        low = value.view(np.int64) & ((1 << 29) - 1)
        near |= np.abs(low - (1 << 28)) <= FAST64_WINDOW - FAST64_BOUND_ULPS - 8
    return per_footprint_any(near)


def whole_footprints(F, H, W):
    """Per footprint: all 256 pixels lie inside the frame."""
    whole = np.ones((F, (H + plan_words.FOOT_H - 1) // plan_words.FOOT_H, (W + plan_words.FOOT_W - 1) // plan_words.FOOT_W), bool)
    if H % plan_words.FOOT_H:
        whole[:, -1, :] = False
    if W % plan_words.FOOT_W:
        whole[:, :, -1] = False
    return whole


def case_for(name):
    if name not in _CASES:
        _CASES[name] = build(BY_NAME[name])
    return _CASES[name]


def build(case):
    """Everything about one (F, H, W, R, C, jitter, kind, seed), read-only."""
    name = name_of(case)
    F, H, W, R, C, jitter, kind, seed = case
    assert W % 4 == 0 and H % 2 == 0 and W <= 512 and H <= 288
    disp, stab = motion(case)
    from oracle import clib
    mx, my = np.empty((F, H, W), F32), np.empty((F, H, W), F32)
    crop = np.empty((F, 4), np.int32)
    records = np.empty((F, R * C, 32))
    for f in range(F):
        mx[f], my[f], crop[f], bad = cv16_model.warp_maps(W, H, R, C, disp[f], stab[f])
        assert bad == 0, (name, f, bad)
        records[f] = clib.cell_table(W, H, R, C, disp[f], stab[f])[0]
    cm = [nv12_model.chroma_maps(mx[f], my[f]) for f in range(F)]
    cmx, cmy = np.stack([m[0] for m in cm]), np.stack([m[1] for m in cm])
    rng = np.random.default_rng(seed)
    planes = rng.normal(0, 1000.0, (F, H, W)).astype(F32)
    labels = {es: rng.integers(0, DATA_TOP[es], (F, H, W), dtype=np.uint64).astype(UINT[es]) for es in UINT}
    y8 = rng.integers(0, 256, (F, H, W), dtype=np.uint8)
    uv8 = rng.integers(0, 256, (F, H // 2, W // 2, 2), dtype=np.uint8)
    y16 = rng.integers(0, 65536, (F, H, W), dtype=np.uint16)
    uv16 = rng.integers(0, 65536, (F, H // 2, W // 2, 2), dtype=np.uint16)
    frames = range(F)
    want = {
        'maps': np.stack([mx, my], axis=-1),
        'plane_f32': np.stack([planes_model.remap_linear_f32(planes[f], mx[f], my[f], FILL_F32) for f in frames]),
        'u16c1': np.stack([p010_model.remap_luma(y16[f], mx[f], my[f], BORDER_P010[0]) for f in frames]),
        'p010_uv': np.stack([p010_model.remap_chroma(uv16[f], cmx[f], cmy[f], BORDER_P010[1:]) for f in frames]),
        'nv12_y': np.stack([nv12_model.remap_luma(y8[f], mx[f], my[f], BORDER_NV12[0]) for f in frames]),
        'nv12_uv': np.stack([nv12_model.remap_chroma(uv8[f], cmx[f], cmy[f], BORDER_NV12[1:]) for f in frames]),
    }
    for es in UINT:
        want['plane_n%d' % es] = np.stack([planes_model.remap_nearest(labels[es][f], mx[f], my[f], FILL[es][1]) for f in frames])
    # where an expected sample is something else than the border / fill value (maps: the pixel has an owner), per luma pixel; a chroma
    # sample counts at its luma pixel (2 cx, 2 cy), the other luma pixels of a chroma format hold nothing
    def at_even(mask):
        out = np.zeros((F, H, W), bool)
        out[:, ::2, ::2] = mask
        return out
    live = {
        'maps': ~((mx == F32(W + 1)) & (my == F32(H + 1))),
        'plane_f32': want['plane_f32'].view(np.uint32) != np.asarray(FILL_F32, F32).view(np.uint32),
        'u16c1': want['u16c1'] != BORDER_P010[0],
        'p010_uv': at_even((want['p010_uv'] != np.asarray(BORDER_P010[1:], np.uint16)).any(axis=-1)),
        'nv12_uv': at_even((want['nv12_uv'] != np.asarray(BORDER_NV12[1:], np.uint8)).any(axis=-1)),
    }
    for es in UINT:
        live['plane_n%d' % es] = want['plane_n%d' % es] != UINT[es](FILL[es][1])
    whole = whole_footprints(F, H, W)
    live_footprints = {fmt: per_footprint_any(m) & whole for fmt, m in live.items()}
    tail_fast = {plane: tail_fast_map(mx, my, W, H, plane) for plane in ('luma', 'chroma')}
    c = dict(name=name, F=F, H=H, W=W, R=R, C=C, disp=disp, stab=stab, records=records, mx=mx, my=my, cmx=cmx, cmy=cmy, crop=crop, planes=planes, labels=labels,
             y8=y8, uv8=uv8, y16=y16, uv16=uv16, want=want, live=live, live_footprints=live_footprints, whole=whole, tail_fast=tail_fast)
    arrays = [disp, stab, records, mx, my, cmx, cmy, crop, planes, y8, uv8, y16, uv16, whole, *labels.values(), *want.values(), *live.values(),
              *live_footprints.values(), *tail_fast.values()]
    for a in arrays:
        a.setflags(write=False)
    return c


def tail_names(c, fmt):
    """Per footprint the tail form `fmt`'s kernel takes on case c: 'fast' / 'clamped' for the two-form tails, 'one' for the others."""
    if fmt not in TWO_FORM_TAILS:
        return np.full(c['whole'].shape, 'one', dtype='<U7')
    return np.where(c['tail_fast'][TWO_FORM_TAILS[fmt]], 'fast', 'clamped')
