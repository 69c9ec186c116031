"""The coordinate-map kernel in the built library (CPU, tools/codeobj.py): it exists once, uses no scratch and spills nothing, stores 16 bytes
at a time, reads no frame -- no byte taps, no window copy -- writes memory from the vector unit only (no scalar store, scalar atomic or
scalar cache write-back), and is not named like a warp kernel: the counts tools/isa_guard.py and the other test_isa_*.py files select by stay what they are.
(That every OTHER kernel of the library is instruction for instruction what it was is checked with tools/isa_compare.py against a build of the
parent commit; its report line is quoted in profiles/warp_maps.md.)"""
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import codeobj  # noqa: E402
import isa_compare  # noqa: E402
import isa_guard  # noqa: E402

LIB = os.path.join(REPO, 'meshflow_amd', 'libmeshflow_hip.so')
FRAG = '14maps_footprintE'

# scalar-unit writes to memory and what goes with them, whatever the width or addressing form: the scalar prefix + one of these stems
STEMS = ('store_', 'buffer_store_', 'scratch_store_', 'atomic_', 'buffer_atomic_', 'dcache_wb', 'dcache_discard')
FORBIDDEN = re.compile('^s_(' + '|'.join(STEMS) + ')')


def _kernel():
    ks = {k: v for k, v in codeobj.all_kernels(LIB).items() if FRAG in k}
    assert len(ks) == 1, list(ks)
    return next(iter(ks.items()))


def _listing():
    name, _ = _kernel()
    lines = isa_compare.listings(LIB)[name]
    assert len(lines) > 100, len(lines)
    return [l.split() for l in lines if l.strip()]


def test_maps_kernel_exists_without_scratch_or_spills():
    name, md = _kernel()
    assert md['private_segment_fixed_size'] == 0, md
    assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, md
    assert md['wavefront_size'] == 64 and md['max_flat_workgroup_size'] == 64, md
    assert md['vgpr_count'] <= 64, md                         # (where it fell without a cap: profiles/warp_maps.md)
    assert md['group_segment_fixed_size'] <= 1024, md         # nine matrix rows and 16 spare bytes: no window
    assert 'warp_kernel' not in name and '8c4' not in name and '8c1' not in name and '_to_kernel' not in name


def test_other_kernel_counts_unchanged():
    ks = codeobj.all_kernels(LIB)
    assert len([k for k in ks if 'warp_kernel' in k]) == 2
    assert len([k for k in ks if '_to_kernel' in k]) == 7
    assert len([k for k in ks if '8c4' in k]) == 5
    assert len([k for k in ks if 'maps' in k]) == 1
    assert len(isa_guard.check_library(LIB)) == 5


def test_stores_wide_and_reads_no_frame():
    ops = [w[0] for w in _listing()]
    assert 'global_store_dwordx4' in ops
    assert 'global_store_dwordx2' in ops                      # the 8-byte form of rows that are not 16-byte aligned and of the right edge
    assert not [o for o in ops if o.startswith('global_store_') and o not in ('global_store_dwordx4', 'global_store_dwordx2')], 'narrow store'
    for bad in ('ds_read_u8', 'ds_read_u8_d16_hi', 'global_load_lds_dwordx4', 'global_load_ubyte', 'global_load_ushort', 'global_load_dwordx2',
                'global_load_dwordx3'):
        assert bad not in ops, bad
    assert not [o for o in ops if o.startswith('buffer_load')]
    assert not [o for o in ops if o.startswith('scratch_')]
    # the only global -> LDS copies are the 4-byte ones that fetch candidate matrices (80-byte rows of the cell table)
    assert {o for o in ops if o.startswith('global_load_lds')} <= {'global_load_lds_dword'}


def test_no_scalar_memory_writes():
    for w in _listing():
        assert not FORBIDDEN.match(w[0]), ' '.join(w)
