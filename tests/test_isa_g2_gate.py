"""Static check of the gfx950 code of the gradient-gate kernels (no GPU: hipcc cross-compiles here, as in test_isa_gated_decoder.py).  The
forward and both backward passes are latency-bound gathers: no scratch, and at most 128 vector registers, i.e. four waves per SIMD.  Reads
the kernels' resource blocks only."""
import pytest

import isa

pytestmark = isa.needs_compiler()
KERNELS = ['g2_gate_blend_kernelILb1E', 'g2_gate_blend_kernelILb0E', 'g2_gate_bwd_node_kernel', 'g2_gate_bwd_gather_kernel']


@pytest.mark.parametrize('kernel', KERNELS)
def test_no_scratch_and_four_waves_per_simd(kernel):
    r = isa.kernel('g2_gate_kernel.hip', r'_ZN4msmp\d+' + kernel)
    print(r)
    assert r.scratch == 0, r
    assert r.vgpr <= 128, r
    assert r.lds == 0, r       # no cross-lane step: every thread runs its node's edge lists on its own
