"""The NV12 crop-resize's chroma kernels in the built library (CPU, tools/codeobj.py): chroma_tables_kernel and chroma_resize_kernel and their
device-rectangle twins chroma_tables_rect_kernel and chroma_resize_rect_kernel (csrc/resize_uv_body.h compiled twice) exist once each, use no
scratch and spill nothing, hold no LDS, do no atomic (the status word is the luma tables kernel's to raise), and are not named like the kernels
the other test_isa_*.py files select by name.  Luma has no kernel of its own here: the u8c1 crop-resize kernels are still the only ones.
(That every OTHER kernel of the library is instruction for instruction what it was is checked with tools/isa_compare.py against a build of the
parent commit; its report line and the register counts are in profiles/nv12_crop.md.)"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import codeobj  # noqa: E402
import isa_compare  # noqa: E402

LIB = os.path.join(REPO, 'meshflow_amd', 'libmeshflow_hip.so')
TABLES = ('20chroma_tables_kernelE', '25chroma_tables_rect_kernelE')
RESIZE = ('20chroma_resize_kernelE', '25chroma_resize_rect_kernelE')
COUNTED_ELSEWHERE = ('nv12', '_to_kernel', '_dev_kernel', '8c1', '8c4', 'plane', 'maps', 'resize16', 'warp_kernel', 'warp16')


def test_chroma_kernels_exist_once_without_scratch_spills_or_lds():
    ks = codeobj.all_kernels(LIB)
    assert len([k for k in ks if 'chroma_tables' in k or 'chroma_resize' in k]) == 4
    for frag in TABLES + RESIZE:
        found = {k: v for k, v in ks.items() if frag in k}
        assert len(found) == 1, (frag, sorted(found))
        (name, md), = found.items()
        assert md['wavefront_size'] == 64 and md['max_flat_workgroup_size'] == 256, (name, md)
        assert md['private_segment_fixed_size'] == 0, (name, md)
        assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, (name, md)
        assert md['group_segment_fixed_size'] <= 16, (name, md)              # direct taps: no window
        for other in COUNTED_ELSEWHERE:
            assert other not in name, (name, other)
    # the luma plane goes through the grey crop-resize as it is: no second copy of any of its kernels
    assert len([k for k in ks if '16resize8c1_kernelE' in k]) == 1 and len([k for k in ks if '20resize8c1_dev_kernelE' in k]) == 1
    assert len([k for k in ks if '19resize8c1_to_kernelI' in k]) == 3 and len([k for k in ks if '23resize8c1_to_dev_kernelI' in k]) == 2
    assert len([k for k in ks if '20resize_tables_kernelE' in k]) == 1 and len([k for k in ks if '24resize_tables_dev_kernelE' in k]) == 1


def test_chroma_kernels_do_no_atomic():
    """The status word of the device-rectangle call is raised once, by the luma tables kernel; the chroma kernels have no atomic at all."""
    listings = isa_compare.listings(LIB)
    for frag in TABLES + RESIZE:
        (name,) = [k for k in listings if frag in k]
        assert len(listings[name]) > 20, name
        assert not [l for l in listings[name] if 'atomic' in l], name
