"""Per-kernel ISA comparison of two builds of libmeshflow_hip.so: for every kernel symbol of the FIRST library, its llvm-objdump listing
(no raw bytes, addresses stripped: tools/codeobj.py) must be identical in the second.  Kernels only the second has are listed as new.

    python tools/isa_compare.py base/libmeshflow_hip.so meshflow_amd/libmeshflow_hip.so

A listing is compared up to and including its last s_endpgm.  What the assembler puts after it to fill the text section out (s_nop 0,
s_code_end, objdump's '...' for a run of zeros) depends on which kernel comes last in its code object, not on the kernel, and is dropped;
anything else after the last s_endpgm still counts.

Exit status 0 when every kernel of the first library is unchanged."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import codeobj  # noqa: E402


PADDING = ('s_nop 0', 's_code_end', '...')


def strip_padding(lines):
    """The listing without its end-of-text padding: cut after the last s_endpgm if every line behind it is padding, unchanged otherwise."""
    last = max((i for i, l in enumerate(lines) if l == 's_endpgm'), default=None)
    if last is None or any(l not in PADDING for l in lines[last + 1:]):
        return lines
    return lines[:last + 1]


def listings(so_path):
    """{kernel symbol: [instruction lines]} over every code object of the library."""
    out = {}
    for co in codeobj.code_objects(so_path):
        dis = codeobj.disassemble(co)
        for name, md in codeobj.kernel_metadata(co).items():
            sym = md['symbol'][:-3] if md['symbol'].endswith('.kd') else md['symbol']
            out[name] = strip_padding(dis.get(sym, []))
    return out


def compare(base_so, new_so):
    a, b = listings(base_so), listings(new_so)
    same = [k for k in a if k in b and a[k] == b[k]]
    changed = [k for k in a if k in b and a[k] != b[k]]
    missing = [k for k in a if k not in b]
    added = sorted(k for k in b if k not in a)
    return a, same, changed, missing, added


def main():
    a, same, changed, missing, added = compare(sys.argv[1], sys.argv[2])
    print(f'{len(a)} kernels in {sys.argv[1]}: {len(same)} identical, {len(changed)} changed, {len(missing)} missing')
    for k in changed:
        print('  CHANGED', k)
    for k in missing:
        print('  MISSING', k)
    for k in added:
        print('  new', k)
    return 0 if not changed and not missing else 1


if __name__ == '__main__':
    sys.exit(main())
