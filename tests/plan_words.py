"""Decoding of the footprint plan and region words a cell table carries behind its records (layout: csrc/mf_common.h), for tests that
must know which warp path a geometry reaches.  One footprint = 8 rows x 32 columns; per footprint 16 plan bytes, then 8 region bytes."""
import numpy as np

PLAN_HOT = 0x2000
PLAN_VALID = 0x4000
PLAN_BORDER = 0x1000
PLAN_FAST64 = 0x0002            # in entry 1, only with PLAN_HOT: the cheap float64 coordinate chain is allowed (MF_PLAN_FAST64)
PLAN_OVERFLOW = 0xFFFF          # entry 7: more than 8 candidate cells, entries 0-3 hold the cell range (MF_PLAN_OVERFLOW)
FOOT_W, FOOT_H = 32, 8          # MF_FOOT_W, MF_FOOT_H
# footprint_class_map's labels, in the order of their codes
CLASS_NAMES = ('hot_fast64', 'hot_plain', 'pair', 'multi', 'border', 'overflow', 'other')
REGION_STAGED = 0x80000000
REGION_COMPACT = 0x20000000
REGION_BORDER = 0x08000000
REGION_ORIGIN_MASK = 0x007FFFFF
GREY_PITCH = 80                 # the grey warp re-cuts a staged window only for frames of at least this many columns (warp_tails.h, MF_C1_PITCH)
C4_COLS = 56                    # the 4-channel warp's re-cut window: this many columns, frames of at least as many (warp_tails.h, MF_C4_COLS)
STAGE_PITCH, COMPACT_PITCH = 160, 112       # the plan's staged windows: bytes per row, wide and COMPACT (mf_common.h)


def plan_and_regions(buf, n, W, H, R, C, src=False):
    """(plan uint32 (n * per_frame, 4), region flags uint32 (n * per_frame,)) of a table buffer (a device or host uint8 tensor); with
    src=True also the region's second word, the window's first dword in its frame (uint32 (n * per_frame,))."""
    nfp = n * ((H + 7) // 8) * ((W + 31) // 32)
    nrec = n * R * C
    plan_off = (nrec * (32 * 8 + 8 + (16 + 12) * 4) + 15) & ~15
    raw = buf[plan_off:plan_off + 24 * nfp].cpu().numpy()
    plan = raw[:16 * nfp].view(np.uint32).reshape(nfp, 4)
    words = raw[16 * nfp:].view(np.uint32).reshape(nfp, 2)
    if src:
        return plan, words[:, 0], words[:, 1]
    return plan, words[:, 0]


def classes(plan, region):
    """Boolean masks per footprint: hot / pair / border (the plan's classes, as tools/class_census.py counts them), multi (MF_PLAN_HOT in
    the first edge-code word, entry 4, and none of the three), overflow (entry 7 is 0xFFFF: the first four entries then hold a cell range,
    whose numbers never carry bit 12 or 13), hot_fast64 (MF_PLAN_FAST64 next to MF_PLAN_HOT in entry 1) and the region's staged / compact /
    border-window flags."""
    x, y, z, w = plan[:, 0], plan[:, 1], plan[:, 2], plan[:, 3]
    hot = ((x >> 16) & PLAN_HOT) != 0
    border = (((x >> 16) & (PLAN_VALID | PLAN_BORDER)) == PLAN_BORDER) & ~hot
    pair = ((y & PLAN_HOT) != 0) & ~hot & ~border
    multi = ((z & PLAN_HOT) != 0) & ~hot & ~pair & ~border
    return dict(hot=hot, pair=pair, border=border, multi=multi, overflow=(w >> 16) == PLAN_OVERFLOW,
                hot_fast64=hot & (((x >> 16) & PLAN_FAST64) != 0),
                staged=(region & REGION_STAGED) != 0, compact=(region & REGION_COMPACT) != 0, border_window=(region & REGION_BORDER) != 0)


def entry_counts(plan):
    """Candidate cells per footprint as footprint_body's general path counts them: the leading entries that carry bit 14 (0 for an empty list
    and for an overflow list, whose first four entries are row and column numbers)."""
    valid = (np.ascontiguousarray(plan).view(np.uint16).reshape(-1, 8) & PLAN_VALID) != 0
    return np.cumprod(valid, axis=1).sum(axis=1)


def footprint_class_map(table):
    """One label per footprint of `table` (an ops.CellTable after ops.cell_table), uint8 (n, ceil(H / 8), ceil(W / 32)) of indices into
    CLASS_NAMES: footprint t of frame f is row t // nfx, column t % nfx (footprint_body's ty, tx).  The classes in the order the warps that
    take the shortcuts without a window test them (warp_body.h, NOWIN): hot -- split by MF_PLAN_FAST64 --, then pair; border, multi and
    overflow lists go through the general path there, 'other' is every remaining list (one uncertified cell, five to eight cells, none)."""
    nfy, nfx = (table.H + FOOT_H - 1) // FOOT_H, (table.W + FOOT_W - 1) // FOOT_W
    plan, region = plan_and_regions(table.buf, table.n, table.W, table.H, table.R, table.C)
    k = classes(plan, region)
    label = np.full(plan.shape[0], CLASS_NAMES.index('other'), np.uint8)
    for name, mask in (('overflow', k['overflow']), ('multi', k['multi']), ('border', k['border']), ('pair', k['pair']),
                       ('hot_plain', k['hot'] & ~k['hot_fast64']), ('hot_fast64', k['hot_fast64'])):
        label[mask] = CLASS_NAMES.index(name)
    return label.reshape(table.n, nfy, nfx)


def per_pixel(footprint_map, H, W):
    """A per-footprint array (n, ceil(H / 8), ceil(W / 32)) expanded to the luma pixels (n, H, W) its footprints hold.  The chroma sample
    (cx, cy) of a 4:2:0 plane belongs to luma pixel (2 cx, 2 cy): per_pixel(...)[:, ::2, ::2]."""
    return np.repeat(np.repeat(np.asarray(footprint_map), FOOT_H, axis=1), FOOT_W, axis=2)[:, :H, :W]


def grey_paths(table, aligned=True):
    """The grey warp paths (warp8c1_footprint) the frames of `table` (an ops.CellTable after ops.cell_table) take, as a set of names:
    'window160' / 'window112' (the grey LDS window re-cut from a STAGED / COMPACT window), 'hot_window' / 'pair_window' (those fast
    paths through it), 'staged_narrow' (a staged footprint in a frame too narrow for the grey window), 'border_region' (a BORDER
    window: no grey window), 'w_mod4' (W % 4 != 0) and 'unaligned' (a stack that is not 4-byte aligned: warp8c1_footprint<false>)."""
    W = table.W
    plan, region = plan_and_regions(table.buf, table.n, W, table.H, table.R, table.C)
    k = classes(plan, region)
    window = k['staged'] & ~k['border_window'] & (W >= GREY_PITCH) & aligned
    seen = set()
    for name, mask in (('window160', window & ~k['compact']), ('window112', window & k['compact']), ('hot_window', window & k['hot']),
                       ('pair_window', window & k['pair']), ('staged_narrow', k['staged'] & (W < GREY_PITCH)),
                       ('border_region', k['border_window'])):
        if mask.any():
            seen.add(name)
    if W % 4:
        seen.add('w_mod4')
    if not aligned:
        seen.add('unaligned')
    return seen


def c4_window_columns(region, src_dwords, W):
    """First column of the 4-byte window (warp_body.h's C4_STAGE block) of each region, decoded as footprint_body does: origin = the low 23
    bits, sy0 = (4 src_dwords - origin) / (3 W - P) + 1/2 in float32 (P = 160, or 112 for COMPACT), bs = origin - P sy0, and the column
    gx = bs / 3 before the clamp to W - C4_COLS.  Meaningful only for STAGED regions."""
    region = np.asarray(region, dtype=np.uint32)
    src_dwords = np.asarray(src_dwords, dtype=np.uint32)
    P = np.where((region & REGION_COMPACT) != 0, COMPACT_PITCH, STAGE_PITCH).astype(np.uint32)
    origin = region & np.uint32(REGION_ORIGIN_MASK)
    with np.errstate(over='ignore'):
        num = ((src_dwords << np.uint32(2)) - origin).astype(np.float32)
        den = (np.uint32(3 * W) - P).astype(np.float32)
        sy0 = (num / den + np.float32(0.5)).astype(np.uint32)
        bs = origin - P * sy0
    return bs // np.uint32(3)


def c4_paths(table, offset):
    """The 4-channel warp paths (warp8c4_footprint) the frames of `table` take from a stack `offset` bytes into a buffer (None: an
    allocation of its own, 16-byte aligned), as a set of names: 'window' / 'window_compact' (the 4-byte LDS window re-cut from a STAGED /
    COMPACT window), 'hot_window' / 'pair_window' (those fast paths through it), 'window_clamped' (its first column clamped to
    W - C4_COLS), 'staged_narrow' (a staged footprint in a frame narrower than C4_COLS), 'border_region' (a BORDER window: not re-cut),
    'w_mod4' (W % 4 != 0), 'unaligned' (not 4-byte aligned: warp8c4_footprint<false>) and 'aligned4_not16' (STAGE on, the stack 4, 8 or
    12 bytes past a 16-byte boundary)."""
    W = table.W
    plan, region, src = plan_and_regions(table.buf, table.n, W, table.H, table.R, table.C, src=True)
    k = classes(plan, region)
    aligned = offset is None or offset % 4 == 0
    window = k['staged'] & ~k['border_window'] & (W >= C4_COLS) & aligned
    clamped = np.zeros_like(window)
    if window.any():
        clamped[window] = c4_window_columns(region[window], src[window], W) > W - C4_COLS
    seen = set()
    for name, mask in (('window', window & ~k['compact']), ('window_compact', window & k['compact']), ('hot_window', window & k['hot']),
                       ('pair_window', window & k['pair']), ('window_clamped', clamped), ('staged_narrow', k['staged'] & (W < C4_COLS)),
                       ('border_region', k['border_window'])):
        if mask.any():
            seen.add(name)
    if W % 4:
        seen.add('w_mod4')
    if not aligned:
        seen.add('unaligned')
    elif offset is not None and offset % 16:
        seen.add('aligned4_not16')
    return seen
