"""CPU: tests/cv16_area.py, the exact-2x (INTER_AREA fast path) branch of cv2.resize on uint16, against hand-computed answers -- above
all the ties, where the area form (half up) and the float path (half to even) part."""
import numpy as np

import cv16_area
import cv16_model


def block(a, b, c, d):
    """A 2 x 2 x 1 uint16 image with S00 = a, S01 = b, S10 = c, S11 = d."""
    return np.array([[[a], [b]], [[c], [d]]], dtype=np.uint16)


def test_known_answers():
    # (S00, S01, S10, S11) -> (sum + 2) >> 2
    cases = [((0, 0, 0, 0), 0), ((1, 0, 0, 0), 0), ((1, 1, 0, 0), 1),          # 2 / 4 = 0.5 -> 1 (half up)
             ((1, 1, 1, 0), 1), ((3, 3, 0, 0), 2),                               # 6 / 4 = 1.5 -> 2
             ((5, 5, 0, 0), 3),                                                  # 10 / 4 = 2.5 -> 3 (half to even would give 2)
             ((65535, 65535, 65535, 65535), 65535), ((65535, 65535, 65535, 65533), 65535),   # 262138 / 4 = 65534.5 -> 65535
             ((100, 200, 300, 401), 250)]                                        # 1001 / 4 = 250.25 -> 250
    for taps, want in cases:
        assert int(cv16_area.area_fast_u16(block(*taps))[0, 0, 0]) == want, taps


def test_ties_differ_from_float_path_exactly_where_sum_is_2_mod_4_and_rounds_to_even_below():
    rng = np.random.default_rng(7)
    src = rng.integers(0, 65536, (64, 96, 3), dtype=np.uint16)
    area = cv16_area.area_fast_u16(src).astype(np.int64)
    flt = cv16_model.resize_linear_u16(src, 48, 32).astype(np.int64)
    s = src.astype(np.int64)
    q = s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2]
    tie_down = (q % 4 == 2) & ((q // 4) % 2 == 0)           # x.5 with an even x: half to even keeps x, half up gives x + 1
    assert np.array_equal(area - flt, tie_down.astype(np.int64))
    assert tie_down.any() and (~tie_down).any()


def test_dispatch():
    rng = np.random.default_rng(3)
    src = rng.integers(0, 65536, (10, 14, 3), dtype=np.uint16)
    assert cv16_area.is_area_fast(14, 10, 7, 5)
    assert np.array_equal(cv16_area.resize_u16(src, 7, 5), cv16_area.area_fast_u16(src))
    for w, h in ((7, 4), (6, 5), (14, 10), (3, 2), (28, 20)):             # one axis 2x is not enough; other ratios take the float path
        assert not cv16_area.is_area_fast(14, 10, w, h)
        assert np.array_equal(cv16_area.resize_u16(src, w, h), cv16_model.resize_linear_u16(src, w, h))
