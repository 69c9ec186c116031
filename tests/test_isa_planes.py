"""The side-plane kernels in the built library (CPU, tools/codeobj.py): the five plane warps and the twelve plane crop-resize kernels exist
once each, use no scratch and spill nothing; the float32 warp takes its deep taps as 8-byte loads and stores 16 bytes at a time; no plane warp
copies a window into LDS; and none of them is named like the kernels tools/isa_guard.py and the other test_isa_*.py files select by name.
(That every OTHER kernel of the library is instruction for instruction what it was is checked with tools/isa_compare.py against a build of the
parent commit; its report line is quoted in profiles/planes.md.)"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import codeobj  # noqa: E402
import isa_compare  # noqa: E402

LIB = os.path.join(REPO, 'meshflow_amd', 'libmeshflow_hip.so')
WARPS = ['15plane_footprintILNS_2PxE%dE' % v for v in (5, 6, 7, 8, 9)]          # PLANE_F32, PLANE_N1, N2, N4, N8
RESIZE = {'19plane_resize_tablesE': 1, '16plane_resize_f32E': 1, '20plane_resize_nearestI': 4,
          '23plane_resize_tables_devE': 1, '20plane_resize_f32_devE': 1, '24plane_resize_nearest_devI': 4}


def _kernels():
    return {k: v for k, v in codeobj.all_kernels(LIB).items() if 'plane' in k}


def test_plane_kernels_exist_without_scratch_or_spills():
    ks = _kernels()
    for frag in WARPS:
        (md,) = [v for k, v in ks.items() if frag in k]
        assert md['wavefront_size'] == 64 and md['max_flat_workgroup_size'] == 64, md
        assert md['vgpr_count'] <= 64, md
        assert md['group_segment_fixed_size'] <= 1024, md         # nine matrix rows and 16 spare bytes: no window
    for frag, count in RESIZE.items():
        assert len([k for k in ks if frag in k]) == count, frag
    assert len(ks) == len(WARPS) + sum(RESIZE.values())
    for name, md in ks.items():
        assert md['private_segment_fixed_size'] == 0, (name, md)
        assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, (name, md)
        for other in ('warp_kernel', '_to_kernel', '_dev_kernel', '8c4', '8c1', 'maps', 'resize16', 'warp16'):
            assert other not in name, (name, other)


def test_float_warp_loads_tap_rows_and_stores_wide():
    listings = isa_compare.listings(LIB)
    (name,) = [k for k in listings if WARPS[0] in k]
    ops = [l.split()[0] for l in listings[name] if l.strip()]
    assert len(ops) > 100
    assert 'global_load_dwordx2' in ops                           # a deep pixel's tap row: S00 S01 in one load
    assert 'global_store_dwordx4' in ops and 'global_store_dword' in ops
    assert not [o for o in ops if o.startswith('scratch_') or o.startswith('buffer_')]
    assert not [o for o in ops if o.startswith('v_pk_')]          # (the blend is scalar float32; whether it is unfused, the GPU tests see bit for bit)
    for frag in WARPS:
        (k,) = [k for k in listings if frag in k]
        ops = {l.split()[0] for l in listings[k] if l.strip()}
        # the only global -> LDS copies are the 4-byte ones that fetch candidate matrices (80-byte rows of the cell table)
        assert {o for o in ops if o.startswith('global_load_lds')} <= {'global_load_lds_dword'}, frag
        assert not [o for o in ops if o.startswith('ds_read_u8')], frag
