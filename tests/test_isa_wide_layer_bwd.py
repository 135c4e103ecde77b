"""Static check of the gfx950 code of the width-generic layer backward's glue kernels (no GPU: hipcc cross-compiles here, as in
test_isa_lem_wide_train.py): every kernel of wide_layer_bwd_kernel.hip uses no scratch.  The grid-stride kernels (a thread = a row and a
16-byte channel group, a few 16-byte values live) stay within 64 vector registers: eight waves per SIMD, the occupancy that hides HBM
latency.  The two per-graph kernels (one 256-thread workgroup per graph and column group, unrolled row loops between block-wide
reductions) stay within 256: at least two workgroups per CU, so one graph's barriers overlap another's loads.  From the code-object
metadata's register and scratch fields only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'msmp-pde_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
KERNELS = ('pad_weights', 'node_feat', 'gather_swish', 'swish_mean', 'cat_node', 'swish', 'dswish_mul', 'mean_bwd_dswish', 'segsum', 'norm_bwd',
           'blend_bwd', 'assemble')
PER_GRAPH = ('norm_bwd', 'blend_bwd')


@pytest.fixture(scope='module')
def isa(tmp_path_factory):
    d = tmp_path_factory.mktemp('isa_wide_layer_bwd')
    s = d / 'wide_layer_bwd_kernel.s'
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-I', CSRC, '-S', '--cuda-device-only',
                    '-o', str(s), os.path.join(CSRC, 'wide_layer_bwd_kernel.hip')], check=True, capture_output=True, cwd=str(d))
    return open(s).read()


def test_the_list_names_every_kernel_of_the_file(isa):
    found = set(re.findall(r'^_ZN4msmp\d+wide_bwd_(\w+?)_kernelE\w*:', isa, re.M))
    assert found == set(KERNELS), sorted(found ^ set(KERNELS))


@pytest.mark.parametrize('name', KERNELS)
def test_registers_and_scratch(isa, name):
    k = re.search(r'^_ZN4msmp\d+wide_bwd_' + name + r'_kernelE\w*:.*?\.end_amdhsa_kernel', isa, re.S | re.M)
    assert k, name
    body = k.group(0)
    num = lambda key: int(re.search(r'\.amdhsa_' + key + r'\s+(\d+)', body).group(1))
    print(name, 'registers', num('next_free_vgpr'))
    assert num('private_segment_fixed_size') == 0, (name, num('private_segment_fixed_size'))
    assert num('next_free_vgpr') <= (256 if name in PER_GRAPH else 64), (name, num('next_free_vgpr'))
