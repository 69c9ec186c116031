"""The luma kernels in the built library (CPU, tools/codeobj.py): luma_kernel<SRC> exists in four instantiations -- BGR and BGRA uint8, BGR
uint16, the 16-bit plane --, each with 64-lane wavefronts and 256-lane workgroups, without scratch, spills or LDS, and none is named like the
kernels the other test_isa_*.py files select by name.  Resource checks only."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import codeobj  # noqa: E402

LIB = os.path.join(REPO, 'meshflow_amd', 'libmeshflow_hip.so')
FRAGMENT = '11luma_kernelILi'                   # mf::luma_kernel<(int)...>: not the crop-resize's hdr_luma_resize kernels
COUNTED_ELSEWHERE = ('8c1', '8c4', '16c1', 'p010', 'nv12', 'plane', 'maps', 'hfit_', 'fast_', 'pyr_', 'lk_', 'hdr_', 'chroma', 'ransac', 'gather',
                     '_to_kernel', '_dev_kernel', 'warp_kernel', 'warp8c1_footprint', 'resize_tables')


def test_the_four_kernels_exist_without_scratch_spills_or_lds():
    ks = codeobj.all_kernels(LIB)
    found = {k: v for k, v in ks.items() if FRAGMENT in k}
    assert sorted(k[:len('_ZN2mf11luma_kernelILi0EEE')] for k in found) == ['_ZN2mf11luma_kernelILi%dEEE' % i for i in range(4)], sorted(found)
    for name, md in found.items():
        assert md['wavefront_size'] == 64 and md['max_flat_workgroup_size'] == 256, (name, md)
        assert md['private_segment_fixed_size'] == 0 and not md.get('uses_dynamic_stack', False), (name, md)
        assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, (name, md)
        assert md['group_segment_fixed_size'] == 0, (name, md)
        assert md.get('agpr_count', 0) == 0, (name, md)
        assert md['vgpr_count'] <= 64, (name, md)              # eight wavefronts per SIMD: a streaming kernel lives on loads in flight
        for other in COUNTED_ELSEWHERE:
            assert other not in name, (name, other)


def test_no_other_kernel_came_with_them():
    ks = codeobj.all_kernels(LIB)
    assert sorted(k for k in ks if 'luma' in k and 'hdr_luma' not in k) == sorted(k for k in ks if FRAGMENT in k)
