"""Static check of the gfx950 code of the fused wide message kernel (no GPU: hipcc cross-compiles here, as in test_isa_budgets.py): the
instantiations that hold the most weights in registers (KT = 6: the GLU classes' width 164; KT = 8: width 256) stay within the 256 vector
registers of two waves per SIMD and use no scratch."""
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
    d = tmp_path_factory.mktemp('isa_wide_message')
    s = d / 'wide_message_kernel.s'
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-I', CSRC, '-S', '--cuda-device-only',
                    '-o', str(s), os.path.join(CSRC, 'wide_message_kernel.hip')], check=True, capture_output=True, cwd=str(d))
    return open(s).read()


@pytest.mark.parametrize('kt', [6, 8])
def test_registers_and_scratch(isa, kt):
    k = re.search(r'^_ZN4msmp19wide_message_kernelILi%dE\w*:.*?\.end_amdhsa_kernel' % kt, isa, re.S | re.M)
    assert k, kt
    num = lambda key: int(re.search(r'\.amdhsa_' + key + r'\s+(\d+)', k.group(0)).group(1))
    assert num('next_free_vgpr') <= 256, (kt, num('next_free_vgpr'))
    assert num('private_segment_fixed_size') == 0, (kt, num('private_segment_fixed_size'))
