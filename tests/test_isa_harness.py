"""The static checks look at the code the library contains: the command tests/isa.py compiles a unit with carries every flag the build
gives that unit, and build() forms its own command by the same function.  The commands are recorded, nothing is compiled."""
from types import SimpleNamespace

import isa

build = isa.build()


def test_the_harness_compiles_a_unit_with_the_flags_of_the_build(monkeypatch, tmp_path):
    ran, formed = [], []
    form = build.compile_command

    def run(cmd, **kw):
        ran.append(cmd)
        if '-S' in cmd:
            open(cmd[cmd.index('-o') + 1], 'w').write('; nothing\n')
    monkeypatch.setattr(build, 'subprocess', SimpleNamespace(run=run, check_call=run))
    monkeypatch.setattr(build, 'compile_command', lambda *a, **kw: formed.append(form(*a, **kw)) or formed[-1])
    monkeypatch.setattr(isa, '_TEXT', {})
    monkeypatch.setattr(isa, '_TMP', [SimpleNamespace(name=str(tmp_path))])

    for unit in ('lem_kernel.hip', 'graph_kernels.hip'):         # (the two units with flags of their own)
        assert isa.asm(unit) == '; nothing\n'
        (cmd,) = ran
        assert cmd is formed[0] and cmd[0] == build.hipcc()
        for flag in build.COMMON + build.SOURCES[unit]:
            assert flag in cmd, (flag, cmd)
        assert '-S' in cmd and '-c' not in cmd

        del ran[:], formed[:]
        build.build(force=True)                                     # (recorded, not run)
        of_unit = [c for c in ran if any(a.endswith('/' + unit) for a in c)]
        assert len(of_unit) == 1 and any(of_unit[0] is c for c in formed), of_unit
        assert of_unit[0][:of_unit[0].index('-c')] == cmd[:cmd.index('-S')]         # the compiler and every flag, in the build's order
        del ran[:], formed[:]
