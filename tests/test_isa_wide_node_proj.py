"""Static check of the gfx950 code of the fused wide projection kernel (no GPU: hipcc cross-compiles here, as in test_isa_wide_node_tail.py):
the instantiations for the GLU classes' width 164 (KT = 6) and for width 256 (KT = 8), at every number of tail steps, stay within the 256
vector registers of two waves per SIMD, use no scratch, and fit the 160 KB of LDS of a compute unit."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'msmp-pde_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')


@pytest.fixture(scope='module')
def isa(tmp_path_factory):
    d = tmp_path_factory.mktemp('isa_wide_node_proj')
    s = d / 'wide_node_proj_kernel.s'
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-I', CSRC, '-S', '--cuda-device-only',
                    '-o', str(s), os.path.join(CSRC, 'wide_node_proj_kernel.hip')], check=True, capture_output=True, cwd=str(d))
    return open(s).read()


@pytest.mark.parametrize('kt', [6, 8])
def test_registers_scratch_and_lds(isa, kt):
    for ts in range(1, 9):
        k = re.search(r'^_ZN4msmp21wide_node_proj_kernelILi%dELi%dE\w*:.*?\.end_amdhsa_kernel' % (kt, ts), isa, re.S | re.M)
        assert k, (kt, ts)
        num = lambda key: int(re.search(r'\.amdhsa_' + key + r'\s+(\d+)', k.group(0)).group(1))
        assert num('next_free_vgpr') <= 256, (kt, ts, num('next_free_vgpr'))
        assert num('private_segment_fixed_size') == 0, (kt, ts, num('private_segment_fixed_size'))
        assert num('group_segment_fixed_size') <= 163840, (kt, ts, num('group_segment_fixed_size'))
