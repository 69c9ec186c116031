"""The 4:2:2 kernels in the built library (CPU, tools/codeobj.py).  nv16_chroma_footprint exists once, uses no scratch and spills nothing, copies
no window into LDS, takes a deep sample's tap row as one 4-byte load and clamped taps as 2-byte loads, stores 4 bytes per lane, and touches no
crop value (no atomic).  The luma plane has no kernel of its own: the grey warp's two instantiations are still the only ones.  The two
streaming kernels of pack422.hip use no scratch, no LDS and no atomics, and hold both the 16-byte accesses of the wide path and the dword /
2-byte accesses it declines to.
(That every OTHER kernel of the library is instruction for instruction what it was is checked with tools/isa_compare.py against a build of the
parent commit; its report line and the register counts are in profiles/nv16.md.)"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import codeobj  # noqa: E402
import isa_compare  # noqa: E402

LIB = os.path.join(REPO, 'meshflow_amd', 'libmeshflow_hip.so')
FRAG = '21nv16_chroma_footprintE'


_LISTINGS = []


def ops_of(frag):
    if not _LISTINGS:
        _LISTINGS.append(isa_compare.listings(LIB))                     # (the library is disassembled once)
    listings = _LISTINGS[0]
    (name,) = [k for k in listings if frag in k]
    ops = [l.split()[0] for l in listings[name] if l.strip()]
    assert len(ops) > 50, name
    return ops


def test_chroma_kernel_exists_without_scratch_or_spills():
    ks = codeobj.all_kernels(LIB)
    found = {k: v for k, v in ks.items() if 'nv16' in k}
    assert len(found) == 1, sorted(found)
    (name, md), = found.items()
    assert FRAG in name
    assert md['wavefront_size'] == 64 and md['max_flat_workgroup_size'] == 64, md
    assert md['private_segment_fixed_size'] == 0, md
    assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, md
    assert md['group_segment_fixed_size'] <= 1024, md                    # nine matrix rows and 16 spare bytes: no window
    for other in ('warp_kernel', '_to_kernel', '_dev_kernel', '8c4', '8c1', 'maps', 'resize16', 'warp16', 'plane', 'nv12'):
        assert other not in name, (name, other)
    # the luma plane goes through the grey warp as it is: no second copy
    assert len([k for k in ks if 'warp8c1_footprint' in k]) == 2


def test_chroma_kernel_taps_and_stores():
    ops = ops_of(FRAG)
    assert 'global_load_dword' in ops                                    # a deep sample's tap row: two 2-byte pixels in one load
    assert 'global_load_ushort' in ops or 'global_load_short_d16' in ops or 'global_load_short_d16_hi' in ops       # a clamped tap: one pixel
    assert 'global_store_dword' in ops and 'global_store_short' in ops   # the lane's two samples; the single one at the end of a W % 4 == 2 row
    assert not [o for o in ops if o.startswith('scratch_') or o.startswith('buffer_')]
    assert not [o for o in ops if 'atomic' in o]                         # the crop rows and the rectangle are the luma launch's
    # the only global -> LDS copies are the 4-byte ones that fetch candidate matrices (80-byte rows of the cell table)
    assert {o for o in ops if o.startswith('global_load_lds')} <= {'global_load_lds_dword'}
    assert not [o for o in ops if o.startswith('ds_read_u8')]
    assert not [o for o in ops if o.startswith('global_load_ubyte')]     # no byte taps: pixels are read whole


def test_streaming_kernels():
    ks = codeobj.all_kernels(LIB)
    for frag, wide_load, narrow_load, narrow_store in (('16unpack422_kernelE', 'global_load_dwordx4', 'global_load_dword', 'global_store_short'),
                                                       ('14pack422_kernelE', 'global_load_dwordx4', 'global_load_ushort', 'global_store_dword')):
        found = {k: v for k, v in ks.items() if frag in k}
        assert len(found) == 1, (frag, sorted(found))
        (md,) = found.values()
        assert md['private_segment_fixed_size'] == 0 and md['group_segment_fixed_size'] == 0, md
        assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, md
        assert md['max_flat_workgroup_size'] == 256, md
        ops = ops_of(frag)
        assert wide_load in ops and 'global_store_dwordx4' in ops, frag                  # the wide path
        assert narrow_load in ops or narrow_load + '_d16' in ops or 'global_load_short_d16' in ops, frag      # what it declines to
        assert narrow_store in ops, frag                                 # the planes' 2-byte stores / the packed head and tail's word
        assert 'v_perm_b32' in ops, frag
        assert not [o for o in ops if 'atomic' in o or o.startswith('ds_') or o.startswith('scratch_') or o.startswith('buffer_')], frag
