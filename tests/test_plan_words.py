"""No GPU: tests/plan_words.py's decoding of the 4-channel warp paths on a hand-made table buffer (region words written as
cell_table.hip lays them out: flags | LDS origin, then the window's first dword in its frame)."""
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
