"""The single-channel kernels in the built library (CPU, tools/codeobj.py): they exist, use no scratch and spill nothing, and the two
warp_kernel instantiations are still the only kernels whose name contains 'warp_kernel' (tools/isa_guard.py selects by that name).
The grey warp uses neither the inline-asm byte-tap runs nor the speculative matrix load (footprint_body compiles both into the
staged uint8 BGR instantiation only), so isa_guard's invariants do not concern it."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import codeobj  # noqa: E402

LIB = os.path.join(REPO, 'meshflow_amd', 'libmeshflow_hip.so')


def _found(ks, short):
    return {k: v for k, v in ks.items() if f'{len(short)}{short}' in k}


def test_grey_kernels_exist_without_scratch_or_spills():
    ks = codeobj.all_kernels(LIB)
    for short, count in (('warp8c1_footprint', 2), ('resize8c1_kernel', 1)):
        found = _found(ks, short)
        assert len(found) == count, (short, list(found))
        for name, md in found.items():
            assert md['private_segment_fixed_size'] == 0, (name, md)
            assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, (name, md)


def test_grey_warp_is_no_warp_kernel():
    ks = codeobj.all_kernels(LIB)
    assert len([k for k in ks if 'warp_kernel' in k]) == 2
    assert not [k for k in _found(ks, 'warp8c1_footprint') if 'warp_kernel' in k]

