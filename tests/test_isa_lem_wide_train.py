"""Static check of the gfx950 code of the LEM training kernels (no GPU: hipcc cross-compiles here, as in test_isa_wide_node_proj.py): for
every KT = 1 .. 8 the forward-with-saving (at KT = 4 one kernel holding the four NS = ceil(ninp / 2) bodies) and the BPTT instantiation use no scratch, stay within the
vector registers that 64 KT threads leave a wave (512 per SIMD lane over ceil(KT / 4) waves per SIMD: 256 at KT = 5 .. 8), hold one
published operand tensor of 6 KT KB in LDS, and multiply on the bf16 matrix pipe only (no fp16 MFMA: the fp32-exact path has no range).

At KT = 4 (width 128, the flagship classes) the register counts are pinned (profiles/r19a_one_lem_training_pair.md):
the forward at <= 168, which is three workgroups per CU -- NEEDED: at 176 registers (two workgroups) the forward with saving of 51 200
nodes took 1.74 ms against 1.63 ms of the retired 128-wide kernel (163 registers); the BPTT at <= 180, its MEASURED count as an upper
bound -- two workgroups per CU there take the time of the retired kernel's three (1.90 - 1.93 ms against 1.94 - 1.95 ms).
At KT = 5 .. 7 (KT = 6: width 164, the GLU classes) both kernels stay at <= 168: three waves per SIMD (512 / 3, allocated in eights), which at
KT = 6 is two six-wave workgroups per CU; above it only one fits."""
import pytest

import isa

pytestmark = isa.needs_compiler()
KERNELS = {'fwd': '_ZN4msmp25lem_wide_train_fwd_kernelILi%dEE', 'bptt': '_ZN4msmp20lem_wide_bptt_kernelILi%dEE'}
KT4_REGISTERS = {'fwd': 168, 'bptt': 180}
THREE_WAVES_PER_SIMD = 168


@pytest.mark.parametrize('kt', range(1, 9))
@pytest.mark.parametrize('which', sorted(KERNELS))
def test_registers_scratch_and_lds(which, kt):
    k = isa.kernel('lem_wide_train_kernel.hip', KERNELS[which] % kt)
    budget = KT4_REGISTERS[which] if kt == 4 else THREE_WAVES_PER_SIMD if kt in (5, 6, 7) else min(512, 512 // ((kt + 3) // 4))
    print(which, kt, 'registers', k.vgpr, 'lds', k.lds)
    assert k.scratch == 0, k
    assert k.vgpr <= budget, (k, budget)
    assert k.lds == 6144 * kt, k
    assert k.count(r'v_mfma_f32_32x32x16_bf16') >= 4 * kt * 12, k       # 4 GEMMs x KT k-tiles x 2 k-steps x 6 products
    assert not k.count(r'v_mfma_\w+_f16'), k
