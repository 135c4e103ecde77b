"""Static check of the gfx950 code of eval_window_kernel (no GPU: hipcc cross-compiles here, as in test_isa_decoder_bwd.py).  Hard
limits: no scratch memory (the per-thread prediction registers of a chunk, pv[16], must stay registers), the LDS footprint the source
declares, and a vector-register count that lets four workgroups share a compute unit.  Nothing is asserted about instruction kinds."""
import pytest

import isa

pytestmark = isa.needs_compiler()
LDS_BYTES = 64 * 65 * 4 + 2 * 256 * 8        # the [64, 65] float tile and the two [256] float64 partial tables
# The compiler reports 117 vector registers (hipcc -O3: sixteen prediction values, eight row segments in flight and their 64-bit
# addresses).  The bound asserted is the occupancy step above it: up to 128 registers a SIMD holds four waves, i.e. four resident
# 256-thread workgroups per compute unit.  A launch has batch * comps workgroups -- 16 or 32 at the evaluation batch sizes, on 256
# compute units -- so residency beyond that buys nothing; the next step down (96 registers, five waves) is not asserted.
VGPR_REPORTED, VGPR_LIMIT = 117, 128


def test_one_kernel_without_scratch_within_its_register_and_lds_budget():
    r = isa.kernel('eval_kernel.hip', r'_ZN4msmp\d+eval_window_kernel')         # (one: kernel() refuses several)
    print(f'eval_window_kernel: {r.vgpr} vector registers (reported when this test was written: {VGPR_REPORTED}), {r.lds} bytes of LDS, '
          f'scratch {r.scratch}')
    assert r.scratch == 0, r
    assert r.lds == LDS_BYTES, r
    assert r.vgpr <= VGPR_LIMIT, r
