"""CPU tests (no kernel launched) of the decoder backward entries, their forward-for-training twins and the size query: the header
declares the nine prototypes and the switch "dec_bwd", the built library exports them at the ABI version of the header, bad arguments are refused by
return value with msmp_last_error naming the entry, every window / width the reference does not define is refused by value as unsupported
(the size query returns 0 for it), a workspace one byte short is refused, and the switch stores the value it is given."""
import os
import re

import pytest

from helpers import L, abi_versions_agree        # noqa: F401  (L: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN_FWD = ('msmp_decoder_train_fwd_f32', 'msmp_decoder2d_train_fwd_f32', 'msmp_decoder_gated_train_fwd_f32', 'msmp_decoder2d_gated_train_fwd_f32')
BWD = ('msmp_decoder_bwd_f32', 'msmp_decoder2d_bwd_f32', 'msmp_decoder_gated_bwd_f32', 'msmp_decoder2d_gated_bwd_f32')
QUERY = 'msmp_decoder_bwd_workspace_bytes'
NET = ('w1', 'b1', 'w2', 'b2')
# argument order of each backward entry; 'ws_bytes' is filled from the size query
ORDER = {
    'msmp_decoder_bwd_f32': ('grad_out', 'h', 'n', 'tw', 'euler') + NET + ('dt', 'dh') + tuple('d' + k for k in NET) + ('ws', 'ws_bytes', 'stream'),
    'msmp_decoder2d_bwd_f32': ('grad_out', 'h', 'n', 'tw') + NET + ('dt', 'dh') + tuple('d' + k for k in NET) + ('ws', 'ws_bytes', 'stream'),
}
GATED_ORDER = (('grad_out', 'h', 'ld', 'u', 'n', 'width', 'tw') + tuple('gate_' + k for k in NET) + tuple('diff_' + k for k in NET) + ('dt', 'dh')
               + tuple('dgate_' + k for k in NET) + tuple('ddiff_' + k for k in NET) + ('ws', 'ws_bytes', 'stream'))
ORDER['msmp_decoder_gated_bwd_f32'] = ORDER['msmp_decoder2d_gated_bwd_f32'] = GATED_ORDER
SCALARS = ('n', 'tw', 'euler', 'dt', 'ld', 'width', 'ws_bytes', 'stream')
KIND = {'msmp_decoder_bwd_f32': (1, 0), 'msmp_decoder2d_bwd_f32': (2, 0), 'msmp_decoder_gated_bwd_f32': (1, 1), 'msmp_decoder2d_gated_bwd_f32': (2, 1)}


def pointers(name):
    return [k for k in ORDER[name] if k not in SCALARS]


def call(L, name, **kw):
    """the entry on fake (never dereferenced: every case is refused before a launch) 16-byte aligned addresses"""
    comps, gated = KIND[name]
    d = dict(n=10, tw=25, euler=1, dt=0.016, ld=384, width=164 if gated else 128, stream=None)
    d.update({k: 4096 * (i + 1) for i, k in enumerate(pointers(name))})
    d.update(kw)
    if 'ws_bytes' not in d:
        d['ws_bytes'] = L.msmp_decoder_bwd_workspace_bytes(comps, gated, 164 if gated else 128, 25) + d.pop('ws_delta', 0)
    return getattr(L, name)(*[d[k] for k in ORDER[name]])


def test_header_declares_and_library_exports_the_entries(L):
    header = open(os.path.join(ROOT, 'include', 'msmp_pde.h')).read()
    for name in TRAIN_FWD + BWD:
        assert re.search(r'\bint\s+' + name + r'\s*\(', header), name
        assert getattr(L, name) is not None
    assert re.search(r'\bsize_t\s+' + QUERY + r'\s*\(', header) and getattr(L, QUERY) is not None
    assert abi_versions_agree(header, L)
    assert '"dec_bwd"' in header


@pytest.mark.parametrize('name,pointer', [(name, p) for name in BWD for p in pointers(name)])
def test_null_pointers_are_argument_errors(L, name, pointer):
    assert call(L, name, **{pointer: None}) == -1, (name, pointer)
    assert b'null' in L.msmp_last_error() and name.encode() in L.msmp_last_error()


@pytest.mark.parametrize('name', TRAIN_FWD)
def test_forward_for_training_entries_refuse_like_their_twins(L, name):
    gated = 'gated' in name
    args = lambda **kw: ([kw.get('h', 4096), 384, 8192, kw.get('n', 10), kw.get('width', 164), kw.get('tw', 25)] + [12288 + 4096 * i for i in range(8)] + [0.016, 65536, None]
                         if gated else [kw.get('h', 4096), 8192, kw.get('n', 10), kw.get('tw', 25)] + [12288 + 4096 * i for i in range(4)] + [0.016, 65536, None])
    assert getattr(L, name)(*args(h=None)) == -1
    assert b'null' in L.msmp_last_error() and name.encode() in L.msmp_last_error()
    assert getattr(L, name)(*args(n=0)) == -1 and b'n_nodes' in L.msmp_last_error()
    assert getattr(L, name)(*args(tw=30)) == -2
    assert name.encode() in L.msmp_last_error() and b'time_window' in L.msmp_last_error()


@pytest.mark.parametrize('name', BWD)
@pytest.mark.parametrize('n', [0, -1, 1 << 31, 1 << 40])
def test_node_counts_outside_the_range_are_argument_errors(L, name, n):
    assert call(L, name, n=n) == -1, (name, n)
    assert b'n_nodes' in L.msmp_last_error() and name.encode() in L.msmp_last_error()


@pytest.mark.parametrize('name,lds', [('msmp_decoder_gated_bwd_f32', (163, 0, -164, 82)), ('msmp_decoder2d_gated_bwd_f32', (327, 164, 256, 0, -328))])
def test_a_row_stride_below_the_row_is_an_argument_error(L, name, lds):
    for ld in lds:
        assert call(L, name, ld=ld) == -1, (name, ld)
        assert b'ld' in L.msmp_last_error()


UNSUPPORTED = [('msmp_decoder_bwd_f32', dict(tw=t)) for t in (0, 24, 30, 100)] + [('msmp_decoder2d_bwd_f32', dict(tw=t)) for t in (20, 24, 100)] \
    + [(name, dict(width=w, tw=t)) for name in BWD[2:] for w, t in ((128, 25), (164, 50), (164, 20), (166, 25))]


@pytest.mark.parametrize('name,sizes', UNSUPPORTED)
def test_other_sizes_are_unsupported_not_an_error_of_the_arguments(L, name, sizes):
    assert call(L, name, ws_bytes=1 << 30, **sizes) == -2, (name, sizes)
    assert b'time_window' in L.msmp_last_error() and name.encode() in L.msmp_last_error()


@pytest.mark.parametrize('name', BWD)
def test_a_workspace_one_byte_short_is_refused(L, name):
    assert call(L, name, ws_delta=-1) == -3, name
    assert b'workspace' in L.msmp_last_error() and name.encode() in L.msmp_last_error()
    assert call(L, name, ws_bytes=0) == -3


def test_the_size_query(L):
    q = L.msmp_decoder_bwd_workspace_bytes
    entries = lambda comps, k1, k2: 8 * comps * k1 + 8 + comps * 8 * k2 + comps      # dW1 | db1 | dW2 | db2 of a network
    rows = 512                                                                      # the grid cap the header states
    assert q(1, 0, 128, 20) == rows * 4 * entries(1, 15, 10)
    assert q(1, 0, 128, 25) == rows * 4 * entries(1, 16, 14) == rows * 4 * 249
    assert q(1, 0, 128, 50) == rows * 4 * entries(1, 12, 10)
    assert q(2, 0, 128, 25) == rows * 4 * entries(2, 16, 14)
    assert q(2, 0, 128, 50) == rows * 4 * entries(2, 12, 10)
    assert q(1, 1, 164, 25) == rows * 4 * 2 * entries(1, 6, 15)
    assert q(2, 1, 164, 25) == rows * 4 * 2 * entries(2, 6, 15) == rows * 4 * 692
    for comps, gated, width, tw in [(2, 0, 128, 20), (1, 0, 164, 25), (1, 0, 128, 30), (1, 1, 128, 25), (1, 1, 164, 50), (2, 1, 166, 25), (0, 0, 128, 25),
                                    (3, 0, 128, 25), (3, 1, 164, 25)]:
        assert q(comps, gated, width, tw) == 0, (comps, gated, width, tw)


def test_the_switch_stores_the_value_it_is_given(L):
    before = L.msmp_tune_query(b'dec_bwd')
    try:
        for value in (0, 1, 2, 5):
            assert L.msmp_tune(b'dec_bwd', value) == 0, (value, L.msmp_last_error())
            assert L.msmp_tune_query(b'dec_bwd') == value
    finally:
        L.msmp_tune(b'dec_bwd', before)
    assert L.msmp_tune_query(b'dec_bwd') == before
