"""The 4-channel uint8 kernels in the built library (CPU, tools/codeobj.py): each exists once, uses no scratch and spills nothing, and none of
them is named like a warp kernel or a crop-resize-to kernel -- the counts tools/isa_guard.py, test_isa_u16.py, test_isa_grey.py and
test_isa_resize_to.py select by stay what they are."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import codeobj  # noqa: E402

LIB = os.path.join(REPO, 'meshflow_amd', 'libmeshflow_hip.so')

# mangled-name fragment -> instantiations: the warp of aligned and unaligned stacks; crop-resize up (the same-size call too), down, direct
KERNELS = {'17warp8c4_footprintILb1E': 1, '17warp8c4_footprintILb0E': 1, '16resize8c4_kernelILi8ELi9ELi1040ELb0E': 1,
           '16resize8c4_kernelILi2ELi4ELi2432ELb1E': 1, '16resize8c4_kernelILi2ELi1ELi0ELb1E': 1}


def test_u8c4_kernels_exist_without_scratch_or_spills():
    ks = codeobj.all_kernels(LIB)
    for frag, count in KERNELS.items():
        found = {k: v for k, v in ks.items() if frag in k}
        assert len(found) == count, (frag, list(found))
        for name, md in found.items():
            assert md['private_segment_fixed_size'] == 0, (name, md)
            assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, (name, md)
    assert len([k for k in ks if '8c4' in k]) == sum(KERNELS.values())


def test_other_kernel_counts_unchanged():
    ks = codeobj.all_kernels(LIB)
    assert len([k for k in ks if 'warp_kernel' in k]) == 2
    assert len([k for k in ks if '_to_kernel' in k]) == 7
    assert not [k for k in ks if '8c4' in k and ('warp_kernel' in k or '_to_kernel' in k)]


def test_direct_instantiation_uses_no_lds():
    ks = codeobj.all_kernels(LIB)
    (md,) = [v for k, v in ks.items() if '16resize8c4_kernelILi2ELi1ELi0ELb1E' in k]
    assert md['group_segment_fixed_size'] == 0
