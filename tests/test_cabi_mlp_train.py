"""CPU tests (no kernel launched) of the Swish-MLP TRAINING entries (mlp_train_kernel.hip: the two-layer and the one-layer form at input
and hidden widths 1 .. 256): the header declares them, the built library exports them with the signatures the ctypes binding lists, the
size entries follow the documented formulas and refuse shapes outside the range, the pack and launch entries refuse shapes and null
pointers by return value before anything is launched, and the switch "mlp_train" is documented, listed and stores the value it is given."""
import os
import re

import pytest

from helpers import L, abi_versions_agree        # noqa: F401  (L: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('msmp_packed_mlp_train_floats', 'msmp_pack_mlp_train_f32', 'msmp_mlp_train_saved_floats', 'msmp_mlp_train_fwd_f32',
         'msmp_mlp_train_bwd_workspace_bytes', 'msmp_mlp_train_bwd_f32')
FORMS = ((2, 1), (1, 1), (1, 2))        # (layers, heads)


def _header():
    return open(os.path.join(ROOT, 'include', 'msmp_pde.h')).read()


def pack(L, layers, heads, k, w):
    return L.msmp_pack_mlp_train_f32(None, None, None, None, layers, heads, k, w, None, None)


def fwd(L, layers, heads, k, w, n=4):
    return L.msmp_mlp_train_fwd_f32(None, k, n, layers, heads, k, w, None, None, None, heads * w, None)


def bwd(L, layers, heads, k, w, n=4):
    return L.msmp_mlp_train_bwd_f32(None, heads * w, None, k, None, n, layers, heads, k, w, None, None, k, None, None, None, None, None, 0, None)


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


@pytest.mark.parametrize('width,kt,blk', [(33, 2, 1), (128, 4, 1), (129, 5, 2), (164, 6, 2), (256, 8, 2)])
def test_size_entries_follow_the_documented_formulas(L, width, kt, blk):
    tile = 2 * 3 * 64 * 4               # one k-tile: [s 2][plane 3][lane 64] 16-byte fragments, in floats
    for k_in in (1, 31, 105, width, 256):
        kk = (k_in + 31) // 32
        for layers, heads in FORMS:
            # forward and transposed fragments of w1 per head (kt x kk k-tiles each way), of w2 (kt x kt each way), one bias row per layer and head
            want = tile * (2 * heads * kt * kk + (2 * kt * kt if layers == 2 else 0)) + layers * heads * 32 * kt
            assert L.msmp_packed_mlp_train_floats(layers, heads, k_in, width) == want, (layers, heads, k_in)
    for n in (1, 97, 51200):
        for layers, heads in FORMS:
            assert L.msmp_mlp_train_saved_floats(n, layers, heads, width) == layers * heads * n * 32 * kt
            # dz1 (, dz2, a1) rows of 128 ceil(heads width / 128) (128 ceil(width / 128)) floats are the least the workspace holds
            rows = n * 4 * (128 * ((heads * width + 127) // 128) + (2 * 128 * blk if layers == 2 else 0))
            assert L.msmp_mlp_train_bwd_workspace_bytes(n, layers, heads, 105, width) >= rows
    assert L.msmp_mlp_train_saved_floats(0, 2, 1, width) == 0 and L.msmp_mlp_train_bwd_workspace_bytes(0, 2, 1, 105, width) == 0


@pytest.mark.parametrize('layers,heads,k_in,width,word', [(2, 1, 64, 0, b'width'), (2, 1, 64, 257, b'width'), (1, 2, 64, 257, b'width'),
                                                            (2, 1, 0, 164, b'k_in'), (2, 1, 257, 164, b'k_in'), (1, 0, 64, 164, b'heads'),
                                                            (1, 3, 64, 164, b'heads'), (2, 2, 64, 164, b'heads'), (3, 1, 64, 164, b'layers')])
def test_shapes_outside_the_range_are_refused_by_value(L, layers, heads, k_in, width, word):
    L.msmp_tune(b'no such key', 0)                   # leaves another message behind
    assert L.msmp_packed_mlp_train_floats(layers, heads, k_in, width) == 0 and word in L.msmp_last_error()
    L.msmp_tune(b'no such key', 0)
    assert L.msmp_mlp_train_bwd_workspace_bytes(4, layers, heads, k_in, width) == 0 and word in L.msmp_last_error()
    if word != b'k_in':
        assert L.msmp_mlp_train_saved_floats(4, layers, heads, width) == 0 and word in L.msmp_last_error()
    for entry in (pack, fwd, bwd):
        L.msmp_tune(b'no such key', 0)
        assert entry(L, layers, heads, k_in, width) == -2 and word in L.msmp_last_error(), entry.__name__


def test_null_pointers_and_sizes_are_refused_before_any_launch(L):
    for layers, heads in FORMS:
        for entry in (pack, fwd, bwd):
            assert entry(L, layers, heads, 105, 164) == -1 and b'null' in L.msmp_last_error(), (entry.__name__, layers, heads)
    for n in (0, -1, 1 << 31):                      # with valid pointers the row count would be the refusal: it is checked by the size entries
        assert L.msmp_mlp_train_saved_floats(n, 2, 1, 164) == 0 and b'n_rows' in L.msmp_last_error()
        assert L.msmp_mlp_train_bwd_workspace_bytes(n, 2, 1, 105, 164) == 0


def test_the_switch_is_documented_listed_and_stores_its_value(L):
    header = _header()
    knobs = header[header.index('/* Knobs for A/B measurements'):header.index('int msmp_tune(const char* key, int value);')]
    entry = re.search(r'\n \*   "mlp_train" (.*?)(?=\n \*   ")', knobs, re.S)
    assert entry and re.search(r'\b1( \(default\))?: ', entry.group(1)) and re.search(r'\b0( \(default\))?: ', entry.group(1)), \
        'the knob list documents "mlp_train" as "1: ... 0: ..." and names one of them the default'
    default = int(re.search(r'(\d) \(default\)', entry.group(1)).group(1))
    assert L.msmp_tune_query(b'mlp_train') == default
    try:
        for value in (0, 1, 2, 5):
            assert L.msmp_tune(b'mlp_train', value) == 0 and L.msmp_tune_query(b'mlp_train') == value
    finally:
        L.msmp_tune(b'mlp_train', default)
    assert L.msmp_tune_query(b'mlp_train') == default
