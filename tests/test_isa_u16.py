"""The uint16 kernels in the built library (CPU, tools/codeobj.py): they exist, use no scratch and spill nothing, and the two warp_kernel
instantiations are still the only kernels whose name contains 'warp_kernel' (tools/isa_guard.py selects by that name)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import codeobj  # noqa: E402

LIB = os.path.join(REPO, 'meshflow_amd', 'libmeshflow_hip.so')
NEW = ('warp16_footprint', 'resize16_kernel', 'resize16_tables_kernel')


def test_u16_kernels_exist_without_scratch_or_spills():
    ks = codeobj.all_kernels(LIB)
    for short in NEW:
        found = {k: v for k, v in ks.items() if f'{len(short)}{short}E' in k}
        assert len(found) == 1, (short, list(found))
        (name, md), = found.items()
        assert md['private_segment_fixed_size'] == 0, (name, md)
        assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, (name, md)


def test_warp_kernel_names_stay_two():
    ks = codeobj.all_kernels(LIB)
    assert sorted(k for k in ks if 'warp_kernel' in k) == sorted(k for k in ks if k.startswith('_ZN2mf11warp_kernelIL'))
    assert len([k for k in ks if 'warp_kernel' in k]) == 2
