"""The P010 crop-resize's kernels in the built library (CPU, tools/codeobj.py): hdr_luma_resize_kernel, hdr_uv_tables_kernel and
hdr_uv_resize_kernel and their device-rectangle twins hdr_*_rect_kernel (csrc/resize_hdr_body.h compiled twice) exist once each, with 64-lane
wavefronts, use no scratch and spill nothing, hold no LDS, do no atomic (the status word is the luma tables kernel's to raise), and are not
named like the kernels the other test_isa_*.py files select by name.  The luma tables have no kernel of their own here: the uint16
crop-resize's tables kernels and resize kernels are still the only ones.
(That every OTHER kernel of the library is instruction for instruction what it was is checked with tools/isa_compare.py against a build of the
parent commit; its report line and the register counts are in profiles/p010_crop.md.)"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import codeobj  # noqa: E402
import isa_compare  # noqa: E402

LIB = os.path.join(REPO, 'meshflow_amd', 'libmeshflow_hip.so')
NEW = ('22hdr_luma_resize_kernelE', '27hdr_luma_resize_rect_kernelE', '20hdr_uv_tables_kernelE', '25hdr_uv_tables_rect_kernelE',
       '20hdr_uv_resize_kernelE', '25hdr_uv_resize_rect_kernelE')
COUNTED_ELSEWHERE = ('p010', '16c1', 'chroma_tables', 'chroma_resize', '_to_kernel', '_dev_kernel', 'nv12', '8c1', '8c4', 'plane', 'maps',
                     'warp_kernel', 'warp16', 'resize16')
KEPT = ('22resize16_tables_kernelE', '26resize16_tables_dev_kernelE', '18resize16_to_kernelE', '22resize16_to_dev_kernelE')


def test_the_six_kernels_exist_once_without_scratch_spills_or_lds():
    ks = codeobj.all_kernels(LIB)
    assert len([k for k in ks if 'hdr_' in k]) == 6
    for frag in NEW:
        found = {k: v for k, v in ks.items() if frag in k}
        assert len(found) == 1, (frag, sorted(found))
        (name, md), = found.items()
        assert md['wavefront_size'] == 64 and md['max_flat_workgroup_size'] == 256, (name, md)
        assert md['private_segment_fixed_size'] == 0, (name, md)
        assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, (name, md)
        assert md['group_segment_fixed_size'] == 0, (name, md)               # direct taps: no LDS
        for other in COUNTED_ELSEWHERE:
            assert other not in name, (name, other)


def test_the_uint16_tables_and_resize_kernels_are_still_one_each():
    """Luma's tables are launched through the units that own resize16_tables_kernel / resize16_tables_dev_kernel: no second copy."""
    ks = codeobj.all_kernels(LIB)
    for frag in KEPT:
        assert len([k for k in ks if frag in k]) == 1, frag


def test_the_six_kernels_do_no_atomic():
    """The status word of the device-rectangle call is raised once, by the luma tables kernel; the new kernels have no atomic at all."""
    listings = isa_compare.listings(LIB)
    for frag in NEW:
        (name,) = [k for k in listings if frag in k]
        assert len(listings[name]) > 20, name
        assert not [l for l in listings[name] if 'atomic' in l], name
