"""Are the gfx950 kernels of two `hipcc -S --cuda-device-only` outputs the same code?
    python scripts/isa_compare.py before.s after.s [before_symbol=after_symbol ...]
Kernels are paired by symbol without the argument type (a renamed kernel: give the pair, also without it).  For every pair: registers, scratch, LDS, occupancy of both, and whether the
instruction streams are identical once symbols, labels and comments are taken out; where they are not, the instruction counts by class that
moved."""
import collections
import re
import sys


def kernels(path):
    text = open(path).read()
    out = {}
    for m in re.finditer(r'^(\w+):\s*; @\1\n(.*?)\.end_amdhsa_kernel.*?; Occupancy: (\d+)', text, re.S | re.M):
        name, body = m.group(1).split('EvNS_')[0], m.group(2)
        code = body.split('.section', 1)[0]
        num = lambda key: int(re.search(r'\.amdhsa_' + key + r'\s+(\d+)', body).group(1))
        lines = []
        for l in code.splitlines():
            l = re.sub(r';.*', '', l).strip()
            if not l or l.startswith('.') and not l.endswith(':'):
                continue
            l = re.sub(r'\.?LBB\d+_\d+', 'L', l)
            l = re.sub(r'_Z\w+', 'SYM', l)
            lines.append(l)
        out[name] = dict(lines=lines, regs=num('next_free_vgpr'), scratch=num('private_segment_fixed_size'), lds=num('group_segment_fixed_size'),
                         occ=int(m.group(3)))
    return out


def klass(l):
    op = l.split()[0]
    for k in ('v_mfma', 'buffer_load', 'global_load', 'global_store', 'ds_read', 'ds_write', 's_barrier', 's_waitcnt', 'v_accvgpr', 's_load', 's_cbranch', 's_branch'):
        if op.startswith(k):
            return k
    return 'valu' if op.startswith('v_') else 'salu' if op.startswith('s_') else 'other'


if __name__ == '__main__':
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    rename = dict(p.split('=') for p in sys.argv[3:])
    same = 0
    for name in a:
        other = rename.get(name, name)
        if other not in b:
            print(f'{name}: not in {sys.argv[2]}')
            continue
        x, y = a[name], b[other]
        res = lambda k: f"registers {k['regs']} scratch {k['scratch']} lds {k['lds']} occ {k['occ']}"
        if x['lines'] == y['lines']:
            same += 1
            print(f'{other}: IDENTICAL ({len(x["lines"])} instructions; {res(y)})')
        else:
            cx, cy = collections.Counter(map(klass, x['lines'])), collections.Counter(map(klass, y['lines']))
            moved = ', '.join(f'{k} {cx[k]} -> {cy[k]}' for k in sorted(set(cx) | set(cy)) if cx[k] != cy[k]) or 'same counts by class, another order or other registers'
            print(f'{other}: DIFFERENT ({len(x["lines"])} -> {len(y["lines"])} instructions; before {res(x)}; after {res(y)}): {moved}')
    print(f'{same} of {len(a)} identical')
