"""Decoding of the footprint plan and region words a cell table carries behind its records (layout: csrc/mf_common.h), for tests that
must know which warp path a geometry reaches.  One footprint = 8 rows x 32 columns; per footprint 16 plan bytes, then 8 region bytes."""
import numpy as np

PLAN_HOT = 0x2000
PLAN_VALID = 0x4000
PLAN_BORDER = 0x1000
REGION_STAGED = 0x80000000
REGION_COMPACT = 0x20000000
REGION_BORDER = 0x08000000
GREY_PITCH = 80                 # the grey warp re-cuts a staged window only for frames of at least this many columns (warp.hip)


def plan_and_regions(buf, n, W, H, R, C):
    """(plan uint32 (n * per_frame, 4), region flags uint32 (n * per_frame,)) of a table buffer (a device or host uint8 tensor)."""
    nfp = n * ((H + 7) // 8) * ((W + 31) // 32)
    nrec = n * R * C
    plan_off = (nrec * (32 * 8 + 8 + (16 + 12) * 4) + 15) & ~15
    raw = buf[plan_off:plan_off + 24 * nfp].cpu().numpy()
    plan = raw[:16 * nfp].view(np.uint32).reshape(nfp, 4)
    region = raw[16 * nfp:].view(np.uint32).reshape(nfp, 2)[:, 0]
    return plan, region


def classes(plan, region):
    """Boolean masks per footprint: hot / pair / border (the plan's classes, as tools/class_census.py counts them) and the region's
    staged / compact / border-window flags."""
    x, y = plan[:, 0], plan[:, 1]
    hot = ((x >> 16) & PLAN_HOT) != 0
    border = (((x >> 16) & (PLAN_VALID | PLAN_BORDER)) == PLAN_BORDER) & ~hot
    pair = ((y & PLAN_HOT) != 0) & ~hot & ~border
    return dict(hot=hot, pair=pair, border=border, staged=(region & REGION_STAGED) != 0, compact=(region & REGION_COMPACT) != 0,
                border_window=(region & REGION_BORDER) != 0)


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
