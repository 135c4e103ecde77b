"""CPU tests (no kernel launched) of the width-generic LEM recurrence entry: the header declares its three prototypes, the built library
exports them, the blob size follows the padded width, bad shapes are refused by return value, and the gfx950 code object of the kernel
(cross-compiled as in test_isa_budgets.py) uses no scratch and stays within the register budget of its __launch_bounds__."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from helpers import abi_versions_agree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'msmp-pde_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
NAMES = ('msmp_packed_lem_wide_floats', 'msmp_pack_lem_wide_f32', 'msmp_lem_encoder_wide_f32')


@pytest.fixture(scope='module')
def L():
    import msmp_pde_amd
    if not os.path.exists(msmp_pde_amd.LIB_PATH):       # hipcc cross-compiles gfx950 without a GPU
        sys.path.insert(0, ROOT)
        import __graft_entry__
        __graft_entry__.build()
    return msmp_pde_amd.lib()


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


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='hipcc not found')
def test_kernel_has_no_scratch_and_fits_its_register_budget(tmp_path):
    s = tmp_path / 'lem_wide_kernel.s'
    subprocess.run([HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I', os.path.join(ROOT, 'include'), '-I', CSRC, '-S', '--cuda-device-only',
                    '-o', str(s), os.path.join(CSRC, 'lem_wide_kernel.hip')], check=True, capture_output=True, cwd=str(tmp_path))
    text = open(s).read()
    seen = 0
    for kt in range(1, 9):
        for m in (1, 2):
            k = re.search(r'^_ZN4msmp15lem_wide_kernelILi%dELi%dE\w*:.*?\.end_amdhsa_kernel' % (kt, m), text, re.S | re.M)
            assert k, (kt, m)
            num = lambda key: int(re.search(r'\.amdhsa_' + key + r'\s+(\d+)', k.group(0)).group(1))
            # __launch_bounds__(64 kt): kt waves on four SIMDs of 512 registers per lane
            budget = 512 // ((kt + 3) // 4)
            assert num('private_segment_fixed_size') == 0, (kt, m, num('private_segment_fixed_size'))
            assert num('next_free_vgpr') <= budget, (kt, m, num('next_free_vgpr'), budget)
            assert num('group_segment_fixed_size') <= 160 * 1024, (kt, m)
            seen += 1
    assert seen == 16
