"""Static check of the gfx950 code of the fused wide message kernel (no GPU: hipcc cross-compiles here, as in test_isa_budgets.py): the
instantiations that hold the most weights in registers (KT = 6: the GLU classes' width 164; KT = 8: width 256) stay within the 256 vector
registers of two waves per SIMD and use no scratch."""
import pytest

import isa

pytestmark = isa.needs_compiler()


@pytest.mark.parametrize('kt', [6, 8])
def test_registers_and_scratch(kt):
    k = isa.kernel('wide_message_kernel.hip', '_ZN4msmp19wide_message_kernelILi%dE' % kt)
    assert k.vgpr <= 256, k
    assert k.scratch == 0, k
