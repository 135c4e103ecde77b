"""Static check of the gfx950 code of the gated decoder kernels of the GLU classes (no GPU: hipcc cross-compiles here, as in
test_isa_wide_node_proj.py).  Each is held to the one-network decoder of the same build that it stands beside at time_window 25
(decoder_split_kernel<25,16,3,14> / decoder2d_split_kernel<25,16,3,14>): no scratch, no more vector registers, and an LDS table that
allows at least as many workgroups per compute unit -- the second network may cost time, not occupancy."""
import pytest

import isa

pytestmark = isa.needs_compiler()
LDS_PER_CU = 163840
PAIRS = [('decoder_gated_kernelILi164ELi25ELi6ELi2ELi15E', 'decoder_split_kernelILi25ELi16ELi3ELi14E'),
         ('decoder2d_gated_kernelILi164ELi25ELi6ELi2ELi15E', 'decoder2d_split_kernelILi25ELi16ELi3ELi14E')]


@pytest.mark.parametrize('gated,single', PAIRS)
def test_scratch_registers_and_lds_against_the_one_network_decoder(gated, single):
    g, s = (isa.kernel('decoder_kernel.hip', r'_ZN4msmp\d+' + name) for name in (gated, single))
    print(f'{g}; {s}')
    assert g.scratch == 0, g
    assert g.vgpr <= s.vgpr, (g, s)
    assert g.lds > 0 and LDS_PER_CU // g.lds >= LDS_PER_CU // s.lds, (g, s)
