"""Are the gfx950 kernels of two assembly files (`python msmp-pde_amd/build.py --asm UNIT.hip -o FILE`) the same code?
    python scripts/isa_compare.py before.s after.s [before_symbol=after_symbol ...]
Kernels are paired by symbol without the argument type (a renamed kernel: give the pair, also without it).  For every pair: registers, scratch, LDS, occupancy of both, and whether the
instruction streams are identical once symbols, labels and comments are taken out; where they are not, the instruction counts by class that
moved."""
import collections
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
from isa import parse          # noqa: E402  (the one parser of the assembly's kernel blocks)


def klass(l):
    op = l.split()[0]
    for k in ('v_mfma', 'buffer_load', 'global_load', 'global_store', 'ds_read', 'ds_write', 's_barrier', 's_waitcnt', 'v_accvgpr', 's_load', 's_cbranch', 's_branch'):
        if op.startswith(k):
            return k
    return 'valu' if op.startswith('v_') else 'salu' if op.startswith('s_') else 'other'


if __name__ == '__main__':
    a, b = ({name.split('EvNS_')[0]: k for name, k in parse(open(path).read()).items()} for path in sys.argv[1:3])
    rename = dict(p.split('=') for p in sys.argv[3:])
    same = 0
    for name in a:
        other = rename.get(name, name)
        if other not in b:
            print(f'{name}: not in {sys.argv[2]}')
            continue
        x, y = a[name], b[other]
        res = lambda k: f'registers {k.vgpr} scratch {k.scratch} lds {k.lds} occ {k.occ}'
        xl, yl = x.lines, y.lines
        if xl == yl:
            same += 1
            print(f'{other}: IDENTICAL ({len(xl)} instructions; {res(y)})')
        else:
            cx, cy = collections.Counter(map(klass, xl)), collections.Counter(map(klass, yl))
            moved = ', '.join(f'{k} {cx[k]} -> {cy[k]}' for k in sorted(set(cx) | set(cy)) if cx[k] != cy[k]) or 'same counts by class, another order or other registers'
            print(f'{other}: DIFFERENT ({len(xl)} -> {len(yl)} instructions; before {res(x)}; after {res(y)}): {moved}')
    print(f'{same} of {len(a)} identical')
