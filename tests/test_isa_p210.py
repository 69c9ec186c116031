"""The P210 / Y210 kernels in the built library (CPU, tools/codeobj.py metadata only): one chroma footprint kernel (p210_chroma_footprint,
csrc/warp_p210.hip), four crop kernels (wide422_tables_kernel, wide422_resize_kernel and their device-rectangle twins,
csrc/resize_wide422_body.h compiled twice) and two pack kernels (unpack_y210_kernel, pack_y210_kernel, csrc/pack_y210.hip) exist once each, use
no scratch and spill nothing, hold no LDS beyond the footprint body's 1024 bytes / 16 bytes, and are not named like the kernels the other
test_isa_*.py files select by name -- whose counts are what they were.  Luma has no kernel of its own: warp16c1_footprint and
hdr_luma_resize_kernel are still the only ones.
(That every OTHER kernel of the library is instruction for instruction what it was is checked with tools/isa_compare.py against a build of the
parent commit; its report line and the register counts are in profiles/p210.md.)"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import codeobj  # noqa: E402

LIB = os.path.join(REPO, 'meshflow_amd', 'libmeshflow_hip.so')
# (mangled fragment, workgroup size, LDS bound)
FOOTPRINT = (('21p210_chroma_footprintE', 64, 1024),)
CROP = (('21wide422_tables_kernelE', 256, 16), ('26wide422_tables_rect_kernelE', 256, 16), ('21wide422_resize_kernelE', 256, 16),
        ('26wide422_resize_rect_kernelE', 256, 16))
PACK = (('18unpack_y210_kernelE', 256, 16), ('16pack_y210_kernelE', 256, 16))
COUNTED_ELSEWHERE = ('hdr_', 'uv422', 'p010', '16c1', 'nv16', 'nv12', 'luma', 'plane', 'maps', '_to_kernel', '_dev_kernel', 'chroma_tables',
                     'chroma_resize', '8c4', '8c1', 'warp_kernel', 'resize16', 'warp16', '16unpack422_kernelE', '14pack422_kernelE')


def test_new_kernels_exist_once_without_scratch_spills_or_lds():
    ks = codeobj.all_kernels(LIB)
    assert len([k for k in ks if 'p210' in k]) == 1 and len([k for k in ks if 'wide422' in k]) == 4 and len([k for k in ks if 'y210' in k]) == 2
    for frag, lanes, lds in FOOTPRINT + CROP + PACK:
        found = {k: v for k, v in ks.items() if frag in k}
        assert len(found) == 1, (frag, sorted(found))
        (name, md), = found.items()
        assert md['wavefront_size'] == 64 and md['max_flat_workgroup_size'] == lanes, (name, md)
        assert md['private_segment_fixed_size'] == 0, (name, md)
        assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, (name, md)
        assert md['group_segment_fixed_size'] <= lds, (name, md)
        for other in COUNTED_ELSEWHERE:
            assert other not in name, (name, other)


def test_the_counts_the_older_files_pin_are_what_they_were():
    ks = codeobj.all_kernels(LIB)

    def count(*frags):
        return len([k for k in ks if any(f in k for f in frags)])

    assert count('uv422') == 4 and count('hdr_') == 6 and count('chroma_tables', 'chroma_resize') == 4
    assert count('21p010_chroma_footprintE') == 1 and count('21nv16_chroma_footprintE') == 1 and count('21nv12_chroma_footprintE') == 1
    assert count('18warp16c1_footprintE') == 1                      # the luma warp of P010 and P210 alike: no second copy
    assert count('22hdr_luma_resize_kernelE') == 1 and count('27hdr_luma_resize_rect_kernelE') == 1
    assert count('16unpack422_kernelE') == 1 and count('14pack422_kernelE') == 1
    assert count('22resize16_tables_kernelE') == 1
