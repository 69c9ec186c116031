"""tools/isa_compare.py's normalisation (CPU, synthetic listings): the padding an assembler leaves after a kernel's last s_endpgm is not part
of the kernel; everything else is."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import isa_compare  # noqa: E402

BODY = ['s_load_dwordx4 s[0:3], s[4:5], 0x0', 's_cbranch_scc1 12', 's_endpgm', 'v_mov_b32_e32 v0, 0', 'global_store_dword v1, v0, s[0:1]',
        's_endpgm']


def test_a_padding_only_tail_compares_equal():
    tails = [[], ['s_nop 0'] * 225, ['s_nop 0', 's_nop 0', '...'], ['...'], ['s_code_end'] * 3 + ['s_nop 0', '...']]
    for t in tails:
        assert isa_compare.strip_padding(BODY + t) == BODY, t


def test_a_real_instruction_in_the_tail_is_a_difference():
    for t in (['s_nop 0', 'v_mov_b32_e32 v0, 1', 's_nop 0'], ['s_nop 1'], ['s_nop 0', 's_branch 65533']):
        assert isa_compare.strip_padding(BODY + t) == BODY + t
        assert isa_compare.strip_padding(BODY + t) != isa_compare.strip_padding(BODY + ['s_nop 0'] * len(t))


def test_a_difference_before_the_tail_is_a_difference():
    other = list(BODY)
    other[3] = 'v_mov_b32_e32 v0, 1'
    assert isa_compare.strip_padding(other + ['s_nop 0'] * 4) != isa_compare.strip_padding(BODY + ['s_nop 0'] * 4)
    # padding in the middle of a kernel (before its last s_endpgm) is code: it stays and it counts
    inner = BODY[:3] + ['s_nop 0'] + BODY[3:]
    assert isa_compare.strip_padding(inner + ['...']) == inner != BODY


def test_a_listing_without_s_endpgm_is_left_alone():
    assert isa_compare.strip_padding(['s_nop 0', '...']) == ['s_nop 0', '...']
    assert isa_compare.strip_padding([]) == []
