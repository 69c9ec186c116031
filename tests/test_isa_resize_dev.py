"""The kernels of mf_crop_resize_dev_* in the built library (CPU, tools/codeobj.py): the bodies of the host-rectangle kernels compiled a
second time with the rectangle read from device memory (csrc/resize_rect.h).  Each exists once, uses no scratch and spills nothing; each
keeps the LDS budget of the kernel it is the twin of; the rectangle comes in by ONE scalar 16-byte load; no scalar store or scalar atomic
anywhere (the status word is a vector atomic); and none is named like the kernels the other ISA tests count ('warp_kernel', '_to_kernel',
'8c4')."""
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'tools'))
import codeobj  # noqa: E402

LIB = os.path.join(REPO, 'meshflow_amd', 'libmeshflow_hip.so')

# mangled-name fragment of the new kernel -> fragment of its host-rectangle twin (None: the tables kernels, no LDS either way)
TWINS = {'24resize_tables_dev_kernelE': None, '26resize16_tables_dev_kernelE': None,
         '17resize_dev_kernelE': '13resize_kernelE', '20resize8c1_dev_kernelE': '16resize8c1_kernelE',
         '19resize16_dev_kernelE': '15resize16_kernelE', '22resize16_to_dev_kernelE': '18resize16_to_kernelE',
         '20resize_to_dev_kernelILi8ELi9ELi800ELb0E': '16resize_to_kernelILi8ELi9ELi800ELb0E',
         '20resize_to_dev_kernelILi2ELi4ELi2048ELb1E': '16resize_to_kernelILi2ELi4ELi2048ELb1E',
         '23resize8c1_to_dev_kernelILi8ELi9ELi272ELb0E': '19resize8c1_to_kernelILi8ELi9ELi272ELb0E',
         '23resize8c1_to_dev_kernelILi4ELi8ELi1024ELb1E': '19resize8c1_to_kernelILi4ELi8ELi1024ELb1E',
         '22resize_bgra_dev_kernelILi8ELi9ELi1040ELb0E': '16resize8c4_kernelILi8ELi9ELi1040ELb0E',
         '22resize_bgra_dev_kernelILi2ELi4ELi2432ELb1E': '16resize8c4_kernelILi2ELi4ELi2432ELb1E'}


def scalar_unit_writes(line):
    """A scalar-unit instruction (mnemonic 's_...') that stores, does an atomic or writes back / discards the scalar data cache."""
    op = line.split()[0] if line.split() else ''
    return op.startswith('s_') and any(w in op for w in ('store', 'atomic', 'dcache'))



def test_dev_kernels_exist_without_scratch_or_spills_with_their_twins_lds():
    ks = codeobj.all_kernels(LIB)
    for frag, twin in TWINS.items():
        found = {k: v for k, v in ks.items() if frag in k}
        assert len(found) == 1, (frag, list(found))
        (name, md), = found.items()
        assert md['private_segment_fixed_size'] == 0, (name, md)
        assert md.get('sgpr_spill_count', 0) == 0 and md.get('vgpr_spill_count', 0) == 0, (name, md)
        assert 'warp_kernel' not in name and '_to_kernel' not in name and '8c4' not in name
        if twin is None:
            assert md['group_segment_fixed_size'] == 0
        else:
            (tmd,) = [v for k, v in ks.items() if twin in k]
            assert md['group_segment_fixed_size'] == tmd['group_segment_fixed_size'], (name, md, tmd)
    assert len([k for k in ks if '_dev_kernel' in k]) == len(TWINS)


def test_the_rectangle_is_one_scalar_load_and_the_scalar_unit_writes_nothing():
    seen = 0
    for co in codeobj.code_objects(LIB):
        for name, lines in codeobj.disassemble(co).items():
            if '_dev_kernel' not in name:
                continue
            seen += 1
            assert not [l for l in lines if scalar_unit_writes(l)], name
            # the first loads of the kernel: its arguments, then four dwords from the pointer among them -- before any vector memory access
            first_vmem = next(i for i, l in enumerate(lines) if re.search(r'\b(global_|flat_|buffer_|ds_)', l))
            head = [l for l in lines[:first_vmem] if 's_load_dwordx4' in l and re.search(r', 0x0\s*$', l)]
            assert head, (name, lines[:12])
            atomics = [l for l in lines if 'atomic' in l]
            assert len(atomics) == (1 if 'tables' in name else 0) and all('global_atomic_add' in l for l in atomics), (name, atomics)
    assert seen == len(TWINS)
