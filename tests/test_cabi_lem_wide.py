"""CPU tests (no kernel launched) of the width-generic LEM recurrence entry: the header declares its three prototypes, the built library
exports them, the blob size follows the padded width, bad shapes are refused by return value, and the gfx950 code object of the kernel
(tests/isa.py) uses no scratch and stays within the register budget of its __launch_bounds__."""
import os
import re

import pytest

import isa
from helpers import L, abi_versions_agree        # noqa: F401  (L: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('msmp_packed_lem_wide_floats', 'msmp_pack_lem_wide_f32', 'msmp_lem_encoder_wide_f32')


def test_header_declares_and_library_exports_the_entry(L):
    header = open(os.path.join(ROOT, 'include', 'msmp_pde.h')).read()
    for name in NAMES:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert getattr(L, name) is not None
    assert abi_versions_agree(header, L)


@pytest.mark.parametrize('width,kt', [(1, 1), (32, 1), (33, 2), (96, 3), (128, 4), (164, 6), (192, 6), (256, 8)])
def test_blob_size_follows_the_padded_width(L, width, kt):
    for ninp in (1, 8):
        assert L.msmp_packed_lem_wide_floats(ninp, width) == 8 + 4096 * kt * kt + 2048 * kt      # scales | 4 gates hi + lo | input slots


@pytest.mark.parametrize('ninp,width', [(4, 0), (4, -3), (4, 257), (0, 164), (9, 164)])
def test_bad_shapes_are_refused_by_value(L, ninp, width):
    assert L.msmp_packed_lem_wide_floats(ninp, width) == 0
    assert L.msmp_last_error()
    assert L.msmp_pack_lem_wide_f32(None, None, None, None, ninp, width, None, None) < 0
    assert L.msmp_lem_encoder_wide_f32(None, 4, 1, ninp, width, 1.0, None, None, None, None, None, None) < 0


def test_null_pointers_and_sizes_are_refused_before_any_launch(L):
    assert L.msmp_pack_lem_wide_f32(None, None, None, None, 4, 164, None, None) < 0
    assert b'null' in L.msmp_last_error()
    assert L.msmp_lem_encoder_wide_f32(None, 4, 1, 4, 164, 1.0, None, None, None, None, None, None) < 0
    assert b'null' in L.msmp_last_error()
    assert L.msmp_lem_encoder_wide_f32(None, 4, 0, 4, 164, 1.0, None, None, None, None, None, None) < 0
    assert b't_len' in L.msmp_last_error()
    assert L.msmp_tune_query(b'lem_wide') == 1
    assert L.msmp_tune(b'lem_wide', 0) == 0 and L.msmp_tune_query(b'lem_wide') == 0
    assert L.msmp_tune(b'lem_wide', 1) == 0


@isa.needs_compiler()
def test_kernel_has_no_scratch_and_fits_its_register_budget():
    seen = 0
    for kt in range(1, 9):
        for m in (1, 2):
            k = isa.kernel('lem_wide_kernel.hip', '_ZN4msmp15lem_wide_kernelILi%dELi%dE' % (kt, m))
            # __launch_bounds__(64 kt): kt waves on four SIMDs of 512 registers per lane
            budget = 512 // ((kt + 3) // 4)
            assert k.scratch == 0, k
            assert k.vgpr <= budget, (k, budget)
            assert k.lds <= 160 * 1024, k
            seen += 1
    assert seen == 16
