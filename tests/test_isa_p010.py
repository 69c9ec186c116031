"""The kernels of the built library by name and number (CPU, tools/codeobj.py): one warp16c1_footprint and one p010_chroma_footprint, without
scratch or spills, beside the kernels that were there -- still one warp16_footprint, one nv12_chroma_footprint, two warp8c1_footprint, two
warp_kernel.  (That every other kernel is instruction for instruction what it was is checked with tools/isa_compare.py against a build of the
parent commit; its report line and the register counts are in profiles/p010.md.)"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import codeobj  # noqa: E402

LIB = os.path.join(REPO, 'meshflow_amd', 'libmeshflow_hip.so')
COUNTS = {'18warp16c1_footprintE': 1, '21p010_chroma_footprintE': 1, '16warp16_footprintE': 1, '21nv12_chroma_footprintE': 1,
          '17warp8c1_footprintI': 2, '11warp_kernelI': 2, '14maps_footprintE': 1, '15plane_footprintI': 5}


def test_kernel_counts():
    ks = codeobj.all_kernels(LIB)
    for frag, count in COUNTS.items():
        assert len([k for k in ks if frag in k]) == count, (frag, sorted(k for k in ks if frag in k))
    assert len([k for k in ks if 'p010' in k or '16c1' in k]) == 2


def test_new_kernels_use_no_scratch_and_spill_nothing():
    ks = codeobj.all_kernels(LIB)
    for frag in ('18warp16c1_footprintE', '21p010_chroma_footprintE'):
        (name, md), = [(k, v) for k, v in ks.items() if frag in k]
        assert md['wavefront_size'] == 64 and md['max_flat_workgroup_size'] == 64, (name, md)
        assert md['private_segment_fixed_size'] == 0, (name, md)
        assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, (name, md)
        assert md['group_segment_fixed_size'] <= 1024, (name, md)        # nine matrix rows and 16 spare bytes: no window
