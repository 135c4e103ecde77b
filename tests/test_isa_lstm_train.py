"""Static check of the gfx950 code of the LSTM kernels (no GPU: hipcc cross-compiles here, as in test_isa_lem_wide_train.py): for every
KT = 1 .. 8 the forward (at KT = 4 one kernel holding the four NS = ceil(ninp / 2) bodies) and the BPTT instantiation use no scratch, stay
within the vector registers that 64 KT threads leave a wave (512 per SIMD lane over ceil(KT / 4) waves per SIMD: 256 at KT = 5 .. 8), hold
one published operand tensor of 6 KT KB in LDS, and multiply on the bf16 matrix pipe only (no fp16 MFMA: the
fp32-exact path has no range).

At KT = 4 (width 128, the only width the reference's LSTM classes use) the measured register counts are pinned as upper bounds (DESIGN.md
section 4.26): the forward at <= 140, the BPTT at <= 152; both are below 168, i.e. three four-wave workgroups per CU."""
import pytest

import isa

pytestmark = isa.needs_compiler()
KERNELS = {'fwd': '_ZN4msmp21lstm_train_fwd_kernelILi%dEE', 'bptt': '_ZN4msmp16lstm_bptt_kernelILi%dEE'}
KT4_REGISTERS = {'fwd': 140, 'bptt': 152}        # measured; DESIGN.md section 4.26


@pytest.mark.parametrize('kt', range(1, 9))
@pytest.mark.parametrize('which', sorted(KERNELS))
def test_registers_scratch_and_lds(which, kt):
    k = isa.kernel('lstm_train_kernel.hip', KERNELS[which] % kt)
    budget = min(512, 512 // ((kt + 3) // 4))
    if kt == 4:
        budget = min(budget, KT4_REGISTERS[which])
    print(which, kt, 'registers', k.vgpr, 'lds', k.lds)
    assert k.scratch == 0, k
    assert k.vgpr <= budget, (k, budget)
    assert k.lds == 6144 * kt, k
    assert k.count(r'v_mfma_f32_32x32x16_bf16') >= 4 * kt * 12, k       # 4 gates x KT k-tiles x 2 k-steps x 6 products
    assert not k.count(r'v_mfma_\w+_f16'), k
