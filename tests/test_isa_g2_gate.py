"""Static check of the gfx950 code of the gradient-gate kernels (no GPU: hipcc cross-compiles here, as in test_isa_gated_decoder.py).  The
forward and both backward passes are latency-bound gathers: no scratch, and at most 128 vector registers, i.e. four waves per SIMD.  Reads
the kernels' resource blocks only."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'msmp-pde_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
KERNELS = ['g2_gate_blend_kernelILb1E', 'g2_gate_blend_kernelILb0E', 'g2_gate_bwd_node_kernel', 'g2_gate_bwd_gather_kernel']


@pytest.fixture(scope='module')
def isa(tmp_path_factory):
    d = tmp_path_factory.mktemp('isa_g2_gate')
    s = d / 'g2_gate_kernel.s'
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-I', CSRC, '-S', '--cuda-device-only',
                    '-o', str(s), os.path.join(CSRC, 'g2_gate_kernel.hip')], check=True, capture_output=True, cwd=str(d))
    return open(s).read()


def resources(isa, kernel):
    k = re.search(r'^_ZN4msmp\d+%s\w*:.*?\.end_amdhsa_kernel' % kernel, isa, re.S | re.M)
    assert k, kernel
    num = lambda key: int(re.search(r'\.amdhsa_' + key + r'\s+(\d+)', k.group(0)).group(1))
    return {'vgpr': num('next_free_vgpr'), 'scratch': num('private_segment_fixed_size'), 'lds': num('group_segment_fixed_size')}


@pytest.mark.parametrize('kernel', KERNELS)
def test_no_scratch_and_four_waves_per_simd(isa, kernel):
    r = resources(isa, kernel)
    print(f'{kernel}: {r}')
    assert r['scratch'] == 0, r
    assert r['vgpr'] <= 128, r
    assert r['lds'] == 0, r       # no cross-lane step: every thread runs its node's edge lists on its own
