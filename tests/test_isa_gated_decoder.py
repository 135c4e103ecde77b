"""Static check of the gfx950 code of the gated decoder kernels of the GLU classes (no GPU: hipcc cross-compiles here, as in
test_isa_wide_node_proj.py).  Each is held to the one-network decoder of the same build that it stands beside at time_window 25
(decoder_split_kernel<25,16,3,14> / decoder2d_split_kernel<25,16,3,14>): no scratch, no more vector registers, and an LDS table that
allows at least as many workgroups per compute unit -- the second network may cost time, not occupancy."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'msmp-pde_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
LDS_PER_CU = 163840
PAIRS = [('decoder_gated_kernelILi164ELi25ELi6ELi2ELi15E', 'decoder_split_kernelILi25ELi16ELi3ELi14E'),
         ('decoder2d_gated_kernelILi164ELi25ELi6ELi2ELi15E', 'decoder2d_split_kernelILi25ELi16ELi3ELi14E')]


@pytest.fixture(scope='module')
def isa(tmp_path_factory):
    d = tmp_path_factory.mktemp('isa_gated_decoder')
    s = d / 'decoder_kernel.s'
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-I', CSRC, '-S', '--cuda-device-only',
                    '-o', str(s), os.path.join(CSRC, 'decoder_kernel.hip')], check=True, capture_output=True, cwd=str(d))
    return open(s).read()


def resources(isa, kernel):
    k = re.search(r'^_ZN4msmp\d+%s\w*:.*?\.end_amdhsa_kernel' % kernel, isa, re.S | re.M)
    assert k, kernel
    num = lambda key: int(re.search(r'\.amdhsa_' + key + r'\s+(\d+)', k.group(0)).group(1))
    return {'vgpr': num('next_free_vgpr'), 'scratch': num('private_segment_fixed_size'), 'lds': num('group_segment_fixed_size')}


@pytest.mark.parametrize('gated,single', PAIRS)
def test_scratch_registers_and_lds_against_the_one_network_decoder(isa, gated, single):
    g, s = resources(isa, gated), resources(isa, single)
    print(f'{gated}: {g}; {single}: {s}')
    assert g['scratch'] == 0, g
    assert g['vgpr'] <= s['vgpr'], (g, s)
    assert g['lds'] > 0 and LDS_PER_CU // g['lds'] >= LDS_PER_CU // s['lds'], (g, s)
