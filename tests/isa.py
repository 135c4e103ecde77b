"""The gfx950 code of the library's units, for the static checks (tests/test_isa_*.py) and the scripts/isa_*.py tools: one compile cache
and the one parser of the assembly's kernel blocks.  A unit is compiled by msmp-pde_amd/build.py's device_asm, i.e. with the flags the
library is built with, at most once per process.  No GPU: hipcc cross-compiles.
    python tests/isa.py UNIT.hip [pattern]      per-kernel table: name, registers, scratch, LDS, occupancy"""
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_TEXT, _KERNELS, _TMP = {}, {}, []


def build():
    """msmp-pde_amd/build.py (imported late: parse() and find() serve any assembly file without the package)"""
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    from msmp_pde_amd import build
    return build


def needs_compiler():
    """pytestmark of a module of static checks: skipped, not passed, where there is no hipcc"""
    import pytest
    return pytest.mark.skipif(not os.path.exists(build().hipcc()), reason='hipcc not found')


def asm(unit):
    """assembly text of one unit of build.SOURCES"""
    if unit not in _TEXT:
        if not _TMP:
            _TMP.append(tempfile.TemporaryDirectory(prefix='msmp_isa_'))
        _TEXT[unit] = open(build().device_asm(unit, os.path.join(_TMP[0].name, unit.replace('.hip', '.s')))).read()
    return _TEXT[unit]


class Kernel:
    """One kernel of an assembly text: `body` (its instructions as printed, from its label to its descriptor), the resources of its
    descriptor (vgpr: next_free_vgpr, scratch: private_segment_fixed_size, lds: group_segment_fixed_size), `occ` (waves per SIMD)."""

    def __init__(self, name, body, descriptor, occ):
        num = lambda key: int(re.search(r'\.amdhsa_' + key + r'\s+(\d+)', descriptor).group(1))
        self.name, self.body, self.occ = name, body, occ
        self.vgpr, self.scratch, self.lds = num('next_free_vgpr'), num('private_segment_fixed_size'), num('group_segment_fixed_size')

    def count(self, pattern):
        return len(re.findall(pattern, self.body))

    @property
    def lines(self):
        """the instruction stream without comments and directives, labels and symbols made anonymous: equal for equal code"""
        out = []
        for l in self.body.splitlines():
            l = re.sub(r';.*', '', l).strip()
            if not l or l.startswith('.') and not l.endswith(':'):
                continue
            out.append(re.sub(r'_Z\w+', 'SYM', re.sub(r'\.?LBB\d+_\d+', 'L', l)))
        return out

    def __repr__(self):
        return f'{self.name}: registers {self.vgpr} scratch {self.scratch} lds {self.lds} occ {self.occ}'


def parse(text):
    """{mangled name: Kernel} of every kernel of an assembly text, in its order"""
    out, occupancy = {}, re.compile(r'^; Occupancy: (\d+)', re.M)
    for d in re.finditer(r'^\t\.amdhsa_kernel (\w+)\n(.*?)^\t\.end_amdhsa_kernel', text, re.S | re.M):
        name = d.group(1)
        label = text.rindex(f'\n{name}:', 0, d.start()) + 1
        body = text[text.index('\n', label) + 1:d.start()].rsplit('\t.section', 1)[0]       # (the descriptor has a section of its own)
        out[name] = Kernel(name, body, d.group(2), int(occupancy.search(text, d.end()).group(1)))
    return out


def kernels(unit):
    if unit not in _KERNELS:
        _KERNELS[unit] = parse(asm(unit))
    return _KERNELS[unit]


def find(found, pattern):
    """The kernels of `found` (a unit's name or a parse() result) whose mangled name starts with `pattern`, a prefix or a regular
    expression.  None: an error that lists what is there."""
    found = kernels(found) if isinstance(found, str) else found
    hit = [k for n, k in found.items() if re.match(pattern, n)]
    assert hit, f'no kernel {pattern!r} among ' + ', '.join(found)
    return hit


def kernel(found, pattern):
    """the one kernel find() gives"""
    hit = find(found, pattern)
    assert len(hit) == 1, f'{pattern!r} names ' + ', '.join(k.name for k in hit)
    return hit[0]


if __name__ == '__main__':
    for k in find(os.path.basename(sys.argv[1]), sys.argv[2] if len(sys.argv) > 2 else ''):
        print(k)
