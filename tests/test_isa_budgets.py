"""Static checks on the gfx950 code of the hot kernels (no GPU: hipcc cross-compiles here).  They pin what round 4 found by reading the ISA
 and what a later edit can silently undo:
  * register budgets that decide the resident workgroups per CU (a volatile guard asm took the gather message kernel from 128 to 194);
  * no scratch in the message / LEM kernels;
  * an LDS-DMA prefetch is not waited for where it is issued (a second __shared__ array in the node tail brings that back)."""
import os
import re

import pytest

import isa

build = isa.build()
pytestmark = isa.needs_compiler()


@pytest.mark.parametrize('src,prefix,max_vgpr', [
    ('tile_kernels.hip', '_ZN4msmp16edge_tile_kernelILi2ELb0E', 168),        # three workgroups per CU
    ('tile_kernels.hip', '_ZN4msmp16edge_tile_kernelILi2ELb1E', 168),
    ('mlp_kernels.hip', '_ZN4msmp20edge_mlp_kernel_occ2ILi1ELb1ELb1ELb1E', 128),   # the gather message kernel (RPU): four waves per SIMD
    ('mlp_kernels.hip', '_ZN4msmp22node_tail_split_kernelILb1E', 256),
    ('lem_kernel.hip', '_ZN4msmp22lem_encoder_ws3_kernelILi4ELi1E', 256),
    ('lem_kernel.hip', '_ZN4msmp22lem_encoder_ws3_kernelILi6ELi2E', 256),
])
def test_register_budgets(src, prefix, max_vgpr):
    k = isa.kernel(src, prefix)
    assert k.vgpr <= max_vgpr, f'{prefix}: {k.vgpr} vector registers (budget {max_vgpr})'
    # (measured on the code as the library builds it: the gated tail 244 registers, the 1-D LEM 251, the 2-D LEM 252, none with scratch --
    # the 24 bytes once allowed to the tail and the 2-D LEM are not needed)
    assert k.scratch == 0, f'{prefix}: {k.scratch} bytes of scratch'


def wait_distances(body):
    """(distance in instructions, barriers between) of every vmcnt wait to the youngest load it completes"""
    ins = [t.strip() for t in body.splitlines() if t.strip() and not t.strip().startswith((';', '.'))]
    pend, nb, out = [], 0, []
    for k, t in enumerate(ins):
        if t.startswith('s_barrier'): nb += 1
        if re.match(r'(global|buffer)_load', t): pend.append((k, nb, 'lds' in t.split()[0]))
        m = re.match(r's_waitcnt.*vmcnt\((\d+)\)', t)
        if m:
            done = pend[:max(len(pend) - int(m.group(1)), 0)]
            if done: out.append((k - done[-1][0], nb - done[-1][1], done[-1][2], k))
            pend = pend[len(done):]
    return out


def test_node_tail_does_not_wait_for_its_lds_dma_prefetch():
    body = isa.kernel('mlp_kernels.hip', '_ZN4msmp22node_tail_split_kernelILb1E').body
    early = [w for w in wait_distances(body) if w[2] and w[0] < 40 and w[3] > 400]      # (past the kernel's prologue)
    # one is expected: the second head's prologue (its first weight chunk and its bias batch are both needed at once)
    assert len(early) <= 1, f'LDS-DMA waited for {early[0][0]} instructions behind its request (instr {early[0][3]}): see DESIGN 4.18 (one __shared__ object; requests pinned)'


def test_message_kernel_k_loop_waits_for_its_dma_at_the_barrier():
    body = isa.kernel('tile_kernels.hip', '_ZN4msmp16edge_tile_kernelILi2ELb0E').body
    dma = [w for w in wait_distances(body) if w[2]]
    assert dma and all(w[0] >= 60 for w in dma), dma


def _regs(tok):
    tok = tok.strip().rstrip(',')
    m = re.match(r'v\[(\d+):(\d+)\]$', tok)
    if m: return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.match(r'v(\d+)$', tok)
    return {int(m.group(1))} if m else set()


def _project_text(path, seen):
    """the text of a source file and of the project headers it includes with #include "...", recursively"""
    if path in seen or not os.path.exists(path):
        return ''
    seen.add(path)
    text = open(path).read()
    return text + ''.join(_project_text(os.path.join(d, h), seen) for h in re.findall(r'^\s*#\s*include\s+"([^"]+)"', text, re.M)
                          for d in (os.path.dirname(path), build.CSRC, os.path.join(build.ROOT, 'include')))


def units_without_mfma():
    """The units of the library that cannot contain an MFMA: the word is neither in their own text nor in a header of the project they
    include.  A test on the sources, no compile; the hazard scan leaves these out."""
    return [u for u in build.SOURCES if 'mfma' not in _project_text(os.path.join(build.CSRC, u), set()).lower()]


@pytest.mark.parametrize('src', [u for u in build.SOURCES if u not in units_without_mfma()])
def test_no_vector_write_in_the_slot_in_front_of_an_mfma_that_reads_it(src):
    """gfx950 does not interlock a VALU write against an MFMA reading the register as SrcA / SrcB in the next issue slot (DESIGN.md 4.18,
    profiles/r04N_mfma_operand_hazard.md).  The compiler pads its own instructions; inline asm is guarded in the source (mfma_operand_guard).
    This checks the result: in no kernel of the file does a vector instruction write an operand of the MFMA right behind it."""
    prev, bad = None, []
    for line in isa.asm(src).splitlines():
        t = line.strip()
        if not t or t.startswith((';', '.')) or t.endswith(':'): continue
        if t.startswith('v_mfma') and prev and prev.startswith('v_') and not prev.startswith(('v_mfma', 'v_cmp', 'v_readlane', 'v_readfirstlane')):
            ops = [o.strip() for o in t.split(None, 1)[1].split(',')]
            written = _regs(prev.split(None, 1)[1].split(',')[0])
            if written & (_regs(ops[1]) | _regs(ops[2])): bad.append((prev, t))
        prev = t
    assert not bad, f'{len(bad)} unguarded VALU -> MFMA operand pairs, e.g. {bad[0]}'
