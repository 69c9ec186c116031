"""The homography fit's kernels in the built library (CPU, tools/codeobj.py): hfit_sums_kernel and hfit_solve_kernel exist once each, with
64-lane wavefronts, use no scratch and spill nothing, hold the LDS DESIGN.md section 4.18 states, and are not named like the kernels the other
test_isa_*.py files select by name.  Resource checks only."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import codeobj  # noqa: E402

LIB = os.path.join(REPO, 'meshflow_amd', 'libmeshflow_hip.so')
# mangled fragment -> (workgroup size, LDS bytes): 4 wavefront totals x 23 sums; the 9 x 9 matrix and its eigenvectors (81 doubles each, the
# second array starting on a 16-byte boundary)
NEW = {'16hfit_sums_kernelE': (256, 4 * 23 * 8), '17hfit_solve_kernelE': (64, 81 * 8 + 8 + 81 * 8)}
COUNTED_ELSEWHERE = ('fast_', 'pyr_', 'lk_', 'ransac', 'gather', 'maps', 'plane', 'hdr_', 'chroma', 'nv12', 'p010', '8c1', '8c4', '16c1',
                     '_to_kernel', '_dev_kernel', 'warp_kernel')


def test_the_two_kernels_exist_once_without_scratch_or_spills():
    ks = codeobj.all_kernels(LIB)
    assert len([k for k in ks if 'hfit_' in k]) == 2
    for frag, (threads, lds) in NEW.items():
        found = {k: v for k, v in ks.items() if frag in k}
        assert len(found) == 1, (frag, sorted(found))
        (name, md), = found.items()
        assert md['wavefront_size'] == 64 and md['max_flat_workgroup_size'] == threads, (name, md)
        assert md['private_segment_fixed_size'] == 0, (name, md)
        assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, (name, md)
        assert md['group_segment_fixed_size'] == lds, (name, md)
        assert md.get('agpr_count', 0) == 0, (name, md)
        for other in COUNTED_ELSEWHERE:
            assert other not in name, (name, other)


def test_design_states_the_same_lds():
    text = open(os.path.join(REPO, 'DESIGN.md')).read()
    assert 'hfit_sums_kernel' in text and 'hfit_solve_kernel' in text
    assert '736 bytes' in text and '1,304 bytes' in text
