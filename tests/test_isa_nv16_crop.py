"""The NV16 crop-resize's chroma kernels in the built library (CPU, tools/codeobj.py metadata only): uv422_tables_kernel and uv422_resize_kernel
and their device-rectangle twins uv422_tables_rect_kernel and uv422_resize_rect_kernel (csrc/resize_uv422_body.h compiled twice) exist once
each, run in workgroups of 256, use no scratch and spill nothing, hold no LDS beyond 16 bytes, and are not named like the kernels the other
test_isa_*.py files select by name.  Luma has no kernel of its own here: the u8c1 crop-resize kernels are still the only ones, and the NV12
chroma kernels are still four.
(That every OTHER kernel of the library is instruction for instruction what it was is checked with tools/isa_compare.py against a build of the
parent commit; its report line and the register counts are in profiles/nv16_crop.md.)"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import codeobj  # noqa: E402

LIB = os.path.join(REPO, 'meshflow_amd', 'libmeshflow_hip.so')
KERNELS = ('19uv422_tables_kernelE', '24uv422_tables_rect_kernelE', '19uv422_resize_kernelE', '24uv422_resize_rect_kernelE')
COUNTED_ELSEWHERE = ('nv16', 'nv12', 'chroma_tables', 'chroma_resize', '_to_kernel', '_dev_kernel', '8c1', '8c4', 'plane', 'maps', 'resize16',
                     'warp', 'hdr')


def test_uv422_kernels_exist_once_without_scratch_spills_or_lds():
    ks = codeobj.all_kernels(LIB)
    assert len([k for k in ks if 'uv422' in k]) == 4
    for frag in KERNELS:
        found = {k: v for k, v in ks.items() if frag in k}
        assert len(found) == 1, (frag, sorted(found))
        (name, md), = found.items()
        assert md['wavefront_size'] == 64 and md['max_flat_workgroup_size'] == 256, (name, md)
        assert md['private_segment_fixed_size'] == 0, (name, md)
        assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, (name, md)
        assert md['group_segment_fixed_size'] <= 16, (name, md)              # direct taps: no window
        for other in COUNTED_ELSEWHERE:
            assert other not in name, (name, other)


def test_luma_and_nv12_chroma_kernel_counts_are_what_they_were():
    ks = codeobj.all_kernels(LIB)
    # the luma plane goes through the grey crop-resize as it is: no second copy of any of its kernels
    assert len([k for k in ks if '16resize8c1_kernelE' in k]) == 1 and len([k for k in ks if '20resize8c1_dev_kernelE' in k]) == 1
    assert len([k for k in ks if '19resize8c1_to_kernelI' in k]) == 3 and len([k for k in ks if '23resize8c1_to_dev_kernelI' in k]) == 2
    assert len([k for k in ks if '20resize_tables_kernelE' in k]) == 1 and len([k for k in ks if '24resize_tables_dev_kernelE' in k]) == 1
    assert len([k for k in ks if 'chroma_tables' in k or 'chroma_resize' in k]) == 4
