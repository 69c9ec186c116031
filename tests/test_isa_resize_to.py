"""The kernels of mf_crop_resize_to_* in the built library (CPU, tools/codeobj.py): each instantiation exists once, uses no scratch and
spills nothing, and none of them is named like a warp kernel (tools/isa_guard.py and test_isa_u16.py select by 'warp_kernel')."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import codeobj  # noqa: E402

LIB = os.path.join(REPO, 'meshflow_amd', 'libmeshflow_hip.so')

# mangled-name fragment -> how many instantiations: u8c3 up + down + direct, u8c1 up + down + direct, u16c3
KERNELS = {'16resize_to_kernelILi8ELi9ELi800ELb0E': 1, '16resize_to_kernelILi2ELi4E': 1, '16resize_to_kernelILi2ELi1ELi0ELb1E': 1,
           '19resize8c1_to_kernelILi8ELi9ELi272ELb0E': 1, '19resize8c1_to_kernelILi4ELi8ELi1024ELb1E': 1,
           '19resize8c1_to_kernelILi4ELi1ELi0ELb1E': 1, '18resize16_to_kernel': 1}
# the direct instantiations reserve no LDS (the down kernels' budget would cost them occupancy)
DIRECT = ('16resize_to_kernelILi2ELi1ELi0ELb1E', '19resize8c1_to_kernelILi4ELi1ELi0ELb1E')


def test_resize_to_kernels_exist_without_scratch_or_spills():
    ks = codeobj.all_kernels(LIB)
    for frag, count in KERNELS.items():
        found = {k: v for k, v in ks.items() if frag in k}
        assert len(found) == count, (frag, list(found))
        for name, md in found.items():
            assert md['private_segment_fixed_size'] == 0, (name, md)
            assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, (name, md)
            assert 'warp_kernel' not in name
    assert len([k for k in ks if '_to_kernel' in k]) == sum(KERNELS.values())


def test_direct_instantiations_use_no_lds():
    ks = codeobj.all_kernels(LIB)
    for frag in DIRECT:
        (md,) = [v for k, v in ks.items() if frag in k]
        assert md['group_segment_fixed_size'] == 0, (frag, md)
