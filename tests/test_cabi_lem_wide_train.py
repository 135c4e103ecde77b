"""CPU tests (no kernel launched) of the LEM TRAINING entries (lem_wide_train_kernel.hip, every width 1 .. 256): the header declares them, the
built library exports them with the signatures the ctypes binding lists, the size entries follow the documented formulas and refuse shapes
outside the range, pack and launch entries refuse null pointers by return value, the switch "lem_wide_train" is documented, listed
and stores the value it is given, and the retired 128-wide entries and their section of the inference blob are gone."""
import os
import re

import pytest

from helpers import L, abi_versions_agree        # noqa: F401  (L: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('msmp_packed_lem_wide_train_floats', 'msmp_pack_lem_wide_train_f32', 'msmp_packed_lem_wide_bwd_floats', 'msmp_pack_lem_wide_bwd_f32',
         'msmp_lem_wide_saved_floats', 'msmp_lem_wide_dg_floats', 'msmp_lem_train_fwd_wide_f32', 'msmp_lem_train_bwd_wide_f32')
RETIRED = ('msmp_lem_saved_floats', 'msmp_lem_train_fwd_f32', 'msmp_packed_lem_bwd_floats', 'msmp_pack_lem_bwd_f32', 'msmp_lem_train_bwd_f32')


def _header():
    return open(os.path.join(ROOT, 'include', 'msmp_pde.h')).read()


def test_header_declares_and_library_exports_the_entries(L):
    """Every entry is declared once, exported, and bound with as many arguments as its prototype has."""
    from msmp_pde_amd._lib import SIGNATURES
    header = _header()
    for name in NAMES:
        protos = re.findall(r'\b' + name + r'\s*\(([^)]*)\)\s*;', header)
        assert len(protos) == 1, name
        n_args = 0 if protos[0].strip() == 'void' else len(protos[0].split(','))
        assert getattr(L, name) is not None
        assert len(SIGNATURES[name][1]) == n_args, (name, n_args)
    assert abi_versions_agree(header, L)


def test_the_128_wide_entries_are_retired(L):
    """The five entries of the 128-wide pair are in neither the header, the binding's table nor the built library, and the blob of
    msmp_pack_lem_f32 is the sum of its remaining sections (the bf16x3 copy of the recurrent chunks, which only that pair read, is gone)."""
    from msmp_pde_amd._lib import SIGNATURES
    header = _header()
    for name in RETIRED:
        assert not re.search(r'\b' + name + r'\b', header), name
        assert name not in SIGNATURES, name
        assert not hasattr(L, name), name
    chunk, h, max_inp = 128 * 32, 128, 8
    fp32 = 16 * chunk + 8 * chunk + 4 * h + 4 * h * max_inp + 2 * h       # rec | mlp | bias | wx | mlp bias
    split = 8 + fp32                                                      # scales | the same five, fp16-split
    wx_h = 4 * 4 * 2 * 64 * 8 // 2                                        # input columns as fp16 slot fragments
    assert L.msmp_packed_lem_floats() == fp32 + split + wx_h == 214536


@pytest.mark.parametrize('width,kt,blk', [(33, 2, 1), (128, 4, 1), (129, 5, 2), (164, 6, 2), (256, 8, 2)])
def test_size_entries_follow_the_documented_formulas(L, width, kt, blk):
    for ninp in (1, 8):
        # rec: 4 gates x kt x kt k-tiles of [s 2][plane 3][lane 64][8 bf16] = 1536 floats | wx 4 x kt x 256 | bias 4 x 32 kt
        assert L.msmp_packed_lem_wide_train_floats(ninp, width) == 6144 * kt * kt + 1024 * kt + 128 * kt
        assert L.msmp_packed_lem_wide_bwd_floats(ninp, width) == 6144 * kt * kt
    for n, t in ((1, 1), (97, 25), (102400, 25)):
        assert L.msmp_lem_wide_saved_floats(n, t, width) == 6 * n * t * 32 * kt
        assert L.msmp_lem_wide_dg_floats(n, t, width) == 4 * n * t * 128 * blk
    assert L.msmp_lem_wide_saved_floats(0, 3, width) == 0 and L.msmp_lem_wide_dg_floats(0, 3, width) == 0


@pytest.mark.parametrize('ninp,width', [(4, 0), (4, 257), (0, 164), (9, 164)])
def test_shapes_outside_the_range_are_refused_by_value(L, ninp, width):
    for size in (L.msmp_packed_lem_wide_train_floats, L.msmp_packed_lem_wide_bwd_floats):
        L.msmp_tune(b'no such key', 0)                   # leaves another message behind
        assert size(ninp, width) == 0
        assert (b'width' if width != 164 else b'ninp') in L.msmp_last_error()
    if width != 164:
        assert L.msmp_lem_wide_saved_floats(4, 2, width) == 0 and b'width' in L.msmp_last_error()
        assert L.msmp_lem_wide_dg_floats(4, 2, width) == 0 and b'width' in L.msmp_last_error()
        assert L.msmp_lem_train_bwd_wide_f32(None, None, None, None, 4, 1, width, 1.0, None, None, None) == -2
    assert L.msmp_pack_lem_wide_train_f32(None, None, None, None, ninp, width, None, None) == -2
    assert L.msmp_pack_lem_wide_bwd_f32(None, None, ninp, width, None, None) == -2
    assert L.msmp_lem_train_fwd_wide_f32(None, 4, 1, ninp, width, 1.0, None, None, None, None, None, None, None) == -2


def test_null_pointers_and_sizes_are_refused_before_any_launch(L):
    assert L.msmp_pack_lem_wide_train_f32(None, None, None, None, 4, 164, None, None) == -1 and b'null' in L.msmp_last_error()
    assert L.msmp_pack_lem_wide_bwd_f32(None, None, 4, 164, None, None) == -1 and b'null' in L.msmp_last_error()
    assert L.msmp_lem_train_fwd_wide_f32(None, 4, 1, 4, 164, 1.0, None, None, None, None, None, None, None) == -1 and b'null' in L.msmp_last_error()
    assert L.msmp_lem_train_fwd_wide_f32(None, 4, 0, 4, 164, 1.0, None, None, None, None, None, None, None) == -1 and b't_len' in L.msmp_last_error()
    assert L.msmp_lem_train_bwd_wide_f32(None, None, None, None, 4, 1, 164, 1.0, None, None, None) == -1 and b'null' in L.msmp_last_error()
    assert L.msmp_lem_train_bwd_wide_f32(None, None, None, None, 4, 0, 164, 1.0, None, None, None) == -1 and b't_len' in L.msmp_last_error()
    assert L.msmp_lem_train_bwd_wide_f32(None, None, None, None, 4, 1, 164, 0.0, None, None, None) == -1 and b'dt' in L.msmp_last_error()
    assert L.msmp_lem_wide_saved_floats(-1, 2, 164) == 0 and L.msmp_lem_wide_saved_floats(4, 0, 164) == 0


def test_the_switch_is_documented_listed_and_stores_its_value(L):
    header = _header()
    knobs = header[header.index('/* Knobs for A/B measurements'):header.index('int msmp_tune(const char* key, int value);')]
    entry = re.search(r'\n \*   "lem_wide_train" (.*?)(?=\n \*   ")', knobs, re.S)
    assert entry and re.search(r'\b1( \(default\))?: ', entry.group(1)) and re.search(r'\b0( \(default\))?: ', entry.group(1)), \
        'the knob list documents "lem_wide_train" as "1: ... 0: ..." and names one of them the default'
    default = int(re.search(r'(\d) \(default\)', entry.group(1)).group(1))
    assert default == 1           # shipped on: profiles/r16a_glu_lem_wide_train.md
    assert L.msmp_tune_query(b'lem_wide_train') == default
    try:
        for value in (0, 1, 2, 5):
            assert L.msmp_tune(b'lem_wide_train', value) == 0 and L.msmp_tune_query(b'lem_wide_train') == value
    finally:
        L.msmp_tune(b'lem_wide_train', default)
    assert L.msmp_tune_query(b'lem_wide_train') == default
