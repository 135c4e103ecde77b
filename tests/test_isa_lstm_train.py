"""Static check of the gfx950 code of the LSTM kernels (no GPU: hipcc cross-compiles here, as in test_isa_lem_wide_train.py): for every
KT = 1 .. 8 the forward (at KT = 4 one kernel holding the four NS = ceil(ninp / 2) bodies) and the BPTT instantiation use no scratch, stay
within the vector registers that 64 KT threads leave a wave (512 per SIMD lane over ceil(KT / 4) waves per SIMD: 256 at KT = 5 .. 8), hold
one published operand tensor of 6 KT KB in LDS, and multiply on the bf16 matrix pipe only (no fp16 MFMA: the
fp32-exact path has no range).

At KT = 4 (width 128, the only width the reference's LSTM classes use) the measured register counts are pinned as upper bounds (DESIGN.md
section 4.26): the forward at <= 140, the BPTT at <= 152; both are below 168, i.e. three four-wave workgroups per CU."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'msmp-pde_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
KERNELS = {'fwd': '_ZN4msmp21lstm_train_fwd_kernelILi%dEE', 'bptt': '_ZN4msmp16lstm_bptt_kernelILi%dEE'}
KT4_REGISTERS = {'fwd': 140, 'bptt': 152}        # measured; DESIGN.md section 4.26


@pytest.fixture(scope='module')
def isa(tmp_path_factory):
    d = tmp_path_factory.mktemp('isa_lstm_train')
    s = d / 'lstm_train_kernel.s'
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-I', CSRC, '-S', '--cuda-device-only',
                    '-o', str(s), os.path.join(CSRC, 'lstm_train_kernel.hip')], check=True, capture_output=True, cwd=str(d))
    return open(s).read()


@pytest.mark.parametrize('kt', range(1, 9))
@pytest.mark.parametrize('which', sorted(KERNELS))
def test_registers_scratch_and_lds(isa, which, kt):
    k = re.search(r'^' + KERNELS[which] % kt + r'\w*:.*?\.end_amdhsa_kernel', isa, re.S | re.M)
    assert k, (which, kt)
    body = k.group(0)
    num = lambda key: int(re.search(r'\.amdhsa_' + key + r'\s+(\d+)', body).group(1))
    budget = min(512, 512 // ((kt + 3) // 4))
    if kt == 4:
        budget = min(budget, KT4_REGISTERS[which])
    print(which, kt, 'registers', num('next_free_vgpr'), 'lds', num('group_segment_fixed_size'))
    assert num('private_segment_fixed_size') == 0, (which, kt, num('private_segment_fixed_size'))
    assert num('next_free_vgpr') <= budget, (which, kt, num('next_free_vgpr'), budget)
    assert num('group_segment_fixed_size') == 6144 * kt, (which, kt, num('group_segment_fixed_size'))
    assert len(re.findall(r'v_mfma_f32_32x32x16_bf16', body)) >= 4 * kt * 12, (which, kt)       # 4 gates x KT k-tiles x 2 k-steps x 6 products
    assert not re.search(r'v_mfma_\w+_f16', body), (which, kt)
