"""The tracker's kernels in the built library (CPU, tools/codeobj.py): fast_detect_kernel, fast_compact_kernel, pyr_down_kernel and
lk_level_kernel exist once each, with 64-lane wavefronts, use no scratch and spill nothing, hold the LDS DESIGN.md section 4.18 states, and are
not named like the kernels the other test_isa_*.py files select by name.  Resource checks only."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import codeobj  # noqa: E402

LIB = os.path.join(REPO, 'meshflow_amd', 'libmeshflow_hip.so')
# mangled fragment -> (workgroup size, LDS bytes): the FAST tile 22 x 72 bytes + 16 x 16 score words; 19 x 32 uint16 row sums; the LK tile
# 24 x 24 bytes + 22 x 22 derivative words
NEW = {'18fast_detect_kernelE': (256, 22 * 72 + 16 * 16 * 4), '19fast_compact_kernelE': (64, 0), '15pyr_down_kernelE': (256, 19 * 32 * 2),
       '15lk_level_kernelE': (64, 24 * 24 + 22 * 22 * 4)}
COUNTED_ELSEWHERE = ('warp_kernel', '_to_kernel', '_dev_kernel', '8c1', '8c4', '16c1', 'hdr_', 'chroma', 'nv12', 'p010', 'plane', 'maps')


def test_the_four_kernels_exist_once_without_scratch_or_spills():
    ks = codeobj.all_kernels(LIB)
    assert len([k for k in ks if 'fast_' in k or 'pyr_' in k or 'lk_' in k]) == 4
    for frag, (threads, lds) in NEW.items():
        found = {k: v for k, v in ks.items() if frag in k}
        assert len(found) == 1, (frag, sorted(found))
        (name, md), = found.items()
        assert md['wavefront_size'] == 64 and md['max_flat_workgroup_size'] == threads, (name, md)
        assert md['private_segment_fixed_size'] == 0, (name, md)
        assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, (name, md)
        assert md['group_segment_fixed_size'] == lds, (name, md)
        for other in COUNTED_ELSEWHERE:
            assert other not in name, (name, other)


def test_the_lk_kernel_leaves_room_for_four_waves_per_simd():
    """One wavefront per feature, latency hidden by occupancy: at most 128 VGPRs (4 waves per SIMD), no AGPR use."""
    ks = codeobj.all_kernels(LIB)
    (md,) = [v for k, v in ks.items() if '15lk_level_kernelE' in k]
    assert md['vgpr_count'] <= 128, md
    assert md.get('agpr_count', 0) == 0, md
