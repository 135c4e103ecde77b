"""Static check of the gfx950 code of the width-generic layer backward's glue kernels (no GPU: hipcc cross-compiles here, as in
test_isa_lem_wide_train.py): every kernel of wide_layer_bwd_kernel.hip uses no scratch.  The grid-stride kernels (a thread = a row and a
16-byte channel group, a few 16-byte values live) stay within 64 vector registers: eight waves per SIMD, the occupancy that hides HBM
latency.  The two per-graph kernels (one 256-thread workgroup per graph and column group, unrolled row loops between block-wide
reductions) stay within 256: at least two workgroups per CU, so one graph's barriers overlap another's loads.  From the code-object
metadata's register and scratch fields only."""
import re

import pytest

import isa

pytestmark = isa.needs_compiler()
KERNELS = ('pad_weights', 'node_feat', 'gather_swish', 'swish_mean', 'cat_node', 'swish', 'dswish_mul', 'mean_bwd_dswish', 'segsum', 'norm_bwd',
           'blend_bwd', 'assemble')
PER_GRAPH = ('norm_bwd', 'blend_bwd')


def test_the_list_names_every_kernel_of_the_file():
    found = {re.match(r'_ZN4msmp\d+wide_bwd_(\w+?)_kernelE', n).group(1) for n in isa.kernels('wide_layer_bwd_kernel.hip')}
    assert found == set(KERNELS), sorted(found ^ set(KERNELS))


@pytest.mark.parametrize('name', KERNELS)
def test_registers_and_scratch(name):
    k = isa.kernel('wide_layer_bwd_kernel.hip', r'_ZN4msmp\d+wide_bwd_' + name + '_kernelE')
    print(name, 'registers', k.vgpr)
    assert k.scratch == 0, k
    assert k.vgpr <= (256 if name in PER_GRAPH else 64), k
