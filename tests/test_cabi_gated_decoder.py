"""CPU tests (no kernel launched) of the gated CNN decoder entries of the GLU classes: the header declares both prototypes and the switch
"wide_dec", the built library exports them at the ABI version of the header, bad arguments are refused by return value with msmp_last_error set, every
(width, time_window) other than (164, 25) is refused by value as unsupported, and the switch stores the value it is given."""
import os
import re

import pytest

from helpers import L, abi_versions_agree        # noqa: F401  (L: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('msmp_decoder_gated_f32', 'msmp_decoder2d_gated_f32')
POINTERS = ('h', 'u', 'gate_w1', 'gate_b1', 'gate_w2', 'gate_b2', 'diff_w1', 'diff_b1', 'diff_w2', 'diff_b2', 'out')


def call(L, name, **kw):
    """the entry on fake (never dereferenced: every case is refused before a launch) 16-byte aligned addresses"""
    d = dict(h=4096, ld=384, u=8192, n=10, width=164, tw=25, gate_w1=12288, gate_b1=16384, gate_w2=20480, gate_b2=24576, diff_w1=28672,
             diff_b1=32768, diff_w2=36864, diff_b2=40960, dt=0.016, out=45056, stream=None)
    d.update(kw)
    return getattr(L, name)(d['h'], d['ld'], d['u'], d['n'], d['width'], d['tw'], d['gate_w1'], d['gate_b1'], d['gate_w2'], d['gate_b2'],
                            d['diff_w1'], d['diff_b1'], d['diff_w2'], d['diff_b2'], d['dt'], d['out'], d['stream'])


def test_header_declares_and_library_exports_the_entries(L):
    header = open(os.path.join(ROOT, 'include', 'msmp_pde.h')).read()
    for name in NAMES:
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert getattr(L, name) is not None
    assert abi_versions_agree(header, L)
    assert '"wide_dec"' in header


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('pointer', POINTERS)
def test_null_pointers_are_argument_errors(L, name, pointer):
    assert call(L, name, **{pointer: None}) == -1, (name, pointer)
    assert b'null' in L.msmp_last_error() and name.encode() in L.msmp_last_error()


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('n', [0, -1, 1 << 31, 1 << 40])
def test_node_counts_outside_the_range_are_argument_errors(L, name, n):
    assert call(L, name, n=n) == -1, (name, n)
    assert b'n_nodes' in L.msmp_last_error()


@pytest.mark.parametrize('name,lds', [('msmp_decoder_gated_f32', (163, 0, -164, 82)), ('msmp_decoder2d_gated_f32', (327, 164, 256, 0, -328))])
def test_a_row_stride_below_the_row_is_an_argument_error(L, name, lds):
    for ld in lds:
        assert call(L, name, ld=ld) == -1, (name, ld)
        assert b'ld' in L.msmp_last_error()


@pytest.mark.parametrize('name', NAMES)
@pytest.mark.parametrize('width,tw', [(128, 25), (164, 50), (164, 20), (166, 25)])
def test_other_sizes_are_unsupported_not_an_error_of_the_arguments(L, name, width, tw):
    assert call(L, name, width=width, tw=tw) == -2, (name, width, tw)
    assert b'width' in L.msmp_last_error() and b'time_window' in L.msmp_last_error()


def test_the_switch_stores_the_value_it_is_given(L):
    before = L.msmp_tune_query(b'wide_dec')
    try:
        for value in (0, 1, 2, 5):
            assert L.msmp_tune(b'wide_dec', value) == 0, (value, L.msmp_last_error())
            assert L.msmp_tune_query(b'wide_dec') == value
    finally:
        L.msmp_tune(b'wide_dec', before)
    assert L.msmp_tune_query(b'wide_dec') == before
