"""Static check of the gfx950 code of the fused wide node tail (no GPU: hipcc cross-compiles here, as in test_isa_wide_message.py): the
instantiations for the GLU classes' width 164 (KT = 6) and for width 256 (KT = 8) stay within the 256 vector registers of two waves per SIMD,
use no scratch, and fit the 160 KB of LDS of a compute unit."""
import pytest

import isa

pytestmark = isa.needs_compiler()


@pytest.mark.parametrize('kt', [6, 8])
def test_registers_scratch_and_lds(kt):
    k = isa.kernel('wide_node_tail_kernel.hip', '_ZN4msmp21wide_node_tail_kernelILi%dE' % kt)
    assert k.vgpr <= 256, k
    assert k.scratch == 0, k
    assert k.lds <= 163840, k
