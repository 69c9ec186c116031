"""No GPU: tests/plan_words.py's decoding on hand-made table buffers -- the 4-channel warp paths (region words written as cell_table.hip
lays them out: flags | LDS origin, then the window's first dword in its frame) and the footprint classes (candidate lists written as
mf_common.h describes them), per footprint and per pixel."""
import types

import numpy as np
import pytest

import plan_words as pw

torch = pytest.importorskip('torch')


def fake_table(W, H, regions):
    """A one-frame, 1 x 1 mesh table whose footprints carry `regions` [(flags, origin, src_dwords)], the rest zero."""
    n, R, C = 1, 1, 1
    nfp = n * ((H + 7) // 8) * ((W + 31) // 32)
    plan_off = (n * R * C * (32 * 8 + 8 + (16 + 12) * 4) + 15) & ~15
    buf = np.zeros(plan_off + 24 * nfp, np.uint8)
    words = buf[plan_off + 16 * nfp:].view(np.uint32).reshape(nfp, 2)
    for i, (flags, origin, src) in enumerate(regions):
        words[i] = (flags | origin, src)
    return types.SimpleNamespace(W=W, H=H, n=n, R=R, C=C, buf=torch.from_numpy(buf))


def fake_plan_table(W, H, lists, n=1):
    """An n-frame, 1 x 1 mesh table whose footprints carry the candidate lists `lists` [the eight uint16 entries e[0..7] of a FootPlan, as
    cell_table.hip writes them], the rest zero; no region words."""
    t = fake_table(W, H, [])
    R = C = 1
    nfp = n * ((H + 7) // 8) * ((W + 31) // 32)
    plan_off = (n * R * C * (32 * 8 + 8 + (16 + 12) * 4) + 15) & ~15
    buf = np.zeros(plan_off + 24 * nfp, np.uint8)
    entries = buf[plan_off:plan_off + 16 * nfp].view(np.uint16).reshape(nfp, 8)
    for i, e in enumerate(lists):
        entries[i] = e
    t.n, t.buf = n, torch.from_numpy(buf)
    return t


# plan entries as mf_common.h lays them out: bits 0-11 the cell, bit 14 valid, bit 15 IN; the flags of the unused entries
VALID, IN, CODES = 0x4000, 0x8000, 0x8000
UNIT, HOT, FAST64, BORDER = 0x0001, 0x2000, 0x0002, 0x1000
LISTS = {
    'hot_fast64': [VALID | IN | 5, UNIT | HOT | FAST64, 0, 0, 0, 0, 0, 0],
    'hot_plain': [VALID | IN | 7, UNIT | HOT, 0, 0, 0, 0, 0, 0],
    'pair': [VALID | 3, VALID | IN | 2, HOT | 0x0001 | 0x0002, 0, CODES | 1, CODES, 0, 0],            # PAIR_FAST | PAIR_VERT beside HOT
    'multi': [VALID | 9, VALID | 8, VALID | 4, VALID | 3, CODES | HOT | 0x1000 | 3 << 6 | 8 | 1 << 4, CODES | 2, CODES | 3, CODES | 0],
    'border': [VALID | 1, UNIT | BORDER, 0, 0, CODES | 2, 0, 0, 0],
    'border_in': [VALID | IN | 1, UNIT | BORDER, 0, 0, 0, 0, 0, 0],                                   # BORDER beside UNIT on an IN cell
    'overflow': [3, 7, 2, 9, 0, 0, 0, 0xFFFF],                                                          # cell rows 3..7, columns 2..9
    'one_uncertified': [VALID | IN | 4, 0, 0, 0, 0, 0, 0, 0],                                           # one IN cell without UNIT
    'unit_not_deep': [VALID | IN | 4, UNIT, 0, 0, 0, 0, 0, 0],
    'two_uncoded': [VALID | 6, VALID | 5, 0, 0, CODES | 4, CODES | 4, 0, 0],                           # a pair the plan did not certify
    'five_cells': [VALID | 9, VALID | 8, VALID | 7, VALID | 6, VALID | IN | 5, 0, 0, 0],
    'empty': [0] * 8,
}


def test_footprint_classes_on_hand_made_lists():
    W, H = 100, 24                                                      # 4 x 3 footprints, the last column 4 pixels wide
    names = list(LISTS)
    t = fake_plan_table(W, H, [LISTS[k] for k in names])
    plan, region = pw.plan_and_regions(t.buf, 1, W, H, 1, 1)
    k = pw.classes(plan, region)
    at = {name: i for i, name in enumerate(names)}
    assert np.flatnonzero(k['hot']).tolist() == [at['hot_fast64'], at['hot_plain']]
    assert np.flatnonzero(k['hot_fast64']).tolist() == [at['hot_fast64']]
    assert np.flatnonzero(k['pair']).tolist() == [at['pair']]
    assert np.flatnonzero(k['multi']).tolist() == [at['multi']]
    assert np.flatnonzero(k['border']).tolist() == [at['border'], at['border_in']]
    assert np.flatnonzero(k['overflow']).tolist() == [at['overflow']]
    want_entries = {'hot_fast64': 1, 'hot_plain': 1, 'pair': 2, 'multi': 4, 'border': 1, 'border_in': 1, 'overflow': 0, 'one_uncertified': 1,
                    'unit_not_deep': 1, 'two_uncoded': 2, 'five_cells': 5, 'empty': 0}
    assert pw.entry_counts(plan).tolist() == [want_entries[n] for n in names]
    cmap = pw.footprint_class_map(t)
    assert cmap.shape == (1, 3, 4) and cmap.dtype == np.uint8
    want = [n if n in pw.CLASS_NAMES else 'border' if n == 'border_in' else 'other' for n in names]
    assert [pw.CLASS_NAMES[c] for c in cmap.reshape(-1)] == want        # footprint t at row t // 4, column t % 4
    assert set(want) == set(pw.CLASS_NAMES)
    # a cell range whose numbers look like flags where valid entries carry them stays an overflow list (rows / columns are below 64)
    assert pw.CLASS_NAMES[pw.footprint_class_map(fake_plan_table(32, 8, [[63, 63, 63, 63, 0, 0, 0, 0xFFFF]]))[0, 0, 0]] == 'overflow'


def test_footprint_class_map_frames_and_pixels():
    W, H, n = 68, 20, 2                                                 # 3 x 3 footprints per frame: the last column 4 wide, the last row 4 high
    order = ['hot_fast64', 'pair', 'empty', 'border', 'multi', 'overflow', 'hot_plain', 'one_uncertified', 'pair']
    t = fake_plan_table(W, H, [LISTS[k] for k in order + order[::-1]], n=n)
    cmap = pw.footprint_class_map(t)
    assert cmap.shape == (2, 3, 3)
    label = lambda k: pw.CLASS_NAMES.index(k if k in pw.CLASS_NAMES else 'other')  # noqa: E731
    assert cmap[0].reshape(-1).tolist() == [label(k) for k in order] and cmap[1].reshape(-1).tolist() == [label(k) for k in order[::-1]]
    px = pw.per_pixel(cmap, H, W)
    assert px.shape == (n, H, W)
    for f in range(n):
        for y in range(H):
            for x in range(W):
                assert px[f, y, x] == cmap[f, y // 8, x // 32]
    # a 4:2:0 chroma sample (cx, cy) belongs to luma pixel (2 cx, 2 cy)
    chroma = px[:, ::2, ::2]
    assert chroma.shape == (n, H // 2, W // 2) and chroma[1, 9, 33] == cmap[1, 2, 2] and chroma[0, 3, 15] == cmap[0, 0, 0] and chroma[0, 4, 16] == cmap[0, 1, 1]


def window(P, W, sy0, bs):
    """(origin, src_dwords) of a staged window at row sy0, byte column bs (a multiple of 4) of a 3-byte-pixel frame of width W."""
    assert bs % 4 == 0
    return P * sy0 + bs, (3 * W * sy0 + bs) // 4


def test_c4_window_columns_and_clamp():
    W = 84                                                              # the 4-byte window: columns gx .. gx + 55, gx <= W - 56 = 28
    wide = pw.REGION_STAGED
    compact = pw.REGION_STAGED | pw.REGION_COMPACT
    cases = [(wide, 160, 3, 88, 29), (wide, 160, 32760, 72, 24), (compact, 112, 5, 84, 28), (compact, 112, 32700, 96, 32)]
    regions = [(f, *window(P, W, sy0, bs)) for f, P, sy0, bs, _ in cases]
    t = fake_table(W, 24, regions)
    _, region, src = pw.plan_and_regions(t.buf, 1, W, 24, 1, 1, src=True)
    assert pw.c4_window_columns(region[:4], src[:4], W).tolist() == [gx for *_, gx in cases]
    seen = pw.c4_paths(t, None)
    assert {'window', 'window_compact', 'window_clamped'} <= seen and 'unaligned' not in seen and 'aligned4_not16' not in seen
    assert 'window_clamped' not in pw.c4_paths(fake_table(W, 24, regions[1:3]), None)          # gx 24 and 28: no clamp
    assert pw.c4_paths(t, 8) >= {'window', 'aligned4_not16'}
    unaligned = pw.c4_paths(t, 3)
    assert 'unaligned' in unaligned and not unaligned & {'window', 'window_compact', 'window_clamped'}
    narrow = pw.c4_paths(fake_table(48, 24, [(wide, *window(160, 48, 2, 8))]), None)
    assert 'staged_narrow' in narrow and 'window' not in narrow
    border = pw.c4_paths(fake_table(W, 24, [(wide | pw.REGION_BORDER, *window(160, W, 2, 8))]), 12)
    assert 'border_region' in border and 'window' not in border and 'aligned4_not16' in border
    assert 'w_mod4' in pw.c4_paths(fake_table(85, 24, []), None)
