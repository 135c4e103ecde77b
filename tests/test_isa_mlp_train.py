"""Static check of the gfx950 code of the Swish-MLP training kernels (no GPU: hipcc cross-compiles here, as in test_isa_lem_wide_train.py):
for every KT = 1 .. 8 the forward-with-saving and the backward instantiation of both forms (two layers; one layer of 1 or 2 heads) use no
scratch, stay within the vector registers that 64 KT threads leave a wave (512 per SIMD lane over ceil(KT / 4) waves per SIMD: 256 at
KT = 5 .. 8), hold one published operand tensor of 6 KT KB in LDS, and multiply on the bf16 matrix pipe only (no
fp16 MFMA: the fp32-exact path has no input range).

At KT = 4 (width 128) and KT = 6 (width 164, the GLU classes) the register counts are pinned to what the kernels compile to, as upper bounds
(profiles/r21a_mlp_train.md): at most 128 registers everywhere, i.e. four waves per SIMD and LDS (24 / 36 KB per workgroup), not registers,
decides how many workgroups a CU holds."""
import pytest

import isa

pytestmark = isa.needs_compiler()
KERNELS = {'fwd': '_ZN4msmp20mlp_train_fwd_kernelILi%dELi%dEE', 'bwd': '_ZN4msmp20mlp_train_bwd_kernelILi%dELi%dEE'}
PINNED = {('fwd', 4, 2): 84, ('fwd', 4, 1): 84, ('bwd', 4, 2): 112, ('bwd', 4, 1): 116,
          ('fwd', 6, 2): 80, ('fwd', 6, 1): 80, ('bwd', 6, 2): 96, ('bwd', 6, 1): 87}
# bf16 MFMAs at least: per GEMM with a compile-time trip count, KT k-tiles x 2 k-steps x 6 products; the loops over x chunks and dx tiles
# have run-time trip counts, so their body counts once
MIN_MFMA = {('fwd', 2): lambda kt: 12 + 12 * kt, ('fwd', 1): lambda kt: 12, ('bwd', 2): lambda kt: 12 * kt + 12, ('bwd', 1): lambda kt: 12}


@pytest.mark.parametrize('kt', range(1, 9))
@pytest.mark.parametrize('layers', (2, 1))
@pytest.mark.parametrize('which', sorted(KERNELS))
def test_registers_scratch_and_lds(which, layers, kt):
    k = isa.kernel('mlp_train_kernel.hip', KERNELS[which] % (kt, layers))
    budget = PINNED.get((which, kt, layers), min(512, 512 // ((kt + 3) // 4)))
    print(which, 'layers', layers, 'KT', kt, 'registers', k.vgpr, 'lds', k.lds)
    assert k.scratch == 0, k
    assert k.vgpr <= budget, (k, budget)
    assert k.lds == 6144 * kt, k
    assert k.count(r'v_mfma_f32_32x32x16_bf16') >= MIN_MFMA[which, layers](kt), k
    assert not k.count(r'v_mfma_\w+_f16'), k
