"""CPU tests (no kernel launched) of the fused width-generic node tail entry: the header declares its four prototypes, the built library
exports them, the blob size follows the padded width, the graph-size cap is 128 at every width, and bad arguments are refused by return
value with msmp_last_error set."""
import os
import re

import pytest

from helpers import L, abi_versions_agree        # noqa: F401  (L: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('msmp_packed_wide_tail_floats', 'msmp_pack_wide_tail_f32', 'msmp_wide_node_tail_max_graph_nodes', 'msmp_wide_node_tail_f32')


def test_header_declares_and_library_exports_the_entry(L):
    header = open(os.path.join(ROOT, 'include', 'msmp_pde.h')).read()
    for name in NAMES:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert getattr(L, name) is not None
    assert abi_versions_agree(header, L)
    assert '"wide_tail"' in header


def test_blob_size_is_positive_inside_the_width_and_nv_range_only(L):
    for width in range(1, 257):
        kt = (width + 31) // 32
        # scales | b3, b4 [Wp] | W3 hi + lo over 4 KT + 1 k-steps (h, agg, one step of variables) | W4 hi + lo over 2 KT k-steps
        want = 8 + 2 * 32 * kt + 512 * kt * (4 * kt + 1) + 1024 * kt * kt
        assert want == 8 + 576 * kt + 3072 * kt * kt
        for nv in range(0, 9):
            assert L.msmp_packed_wide_tail_floats(width, nv) == want, (width, nv)
    for width in (0, 257, -5):
        assert L.msmp_packed_wide_tail_floats(width, 2) == 0
        assert b'width' in L.msmp_last_error()
    for nv in (-1, 9):
        assert L.msmp_packed_wide_tail_floats(164, nv) == 0
        assert b'nv' in L.msmp_last_error()


def test_graph_cap_is_128_at_every_width(L):
    for width in range(1, 257):
        assert L.msmp_wide_node_tail_max_graph_nodes(width) == 128, width
    for width in (0, 257):
        assert L.msmp_wide_node_tail_max_graph_nodes(width) == 0 and b'width' in L.msmp_last_error()


def call(L, **kw):
    """msmp_wide_node_tail_f32 on fake (never dereferenced: every case is refused before a launch) 16-byte aligned addresses"""
    d = dict(h=4096, agg_main=8192, agg_gate=12288, vars=16384, graph_ptr=20480, n=10, g=2, cap=10, nv=2, width=164, ld=256, packed_main=24576,
             packed_gate=28672, eps=1e-5, out=32768, stream=None)
    d.update(kw)
    return L.msmp_wide_node_tail_f32(d['h'], d['agg_main'], d['agg_gate'], d['vars'], d['graph_ptr'], d['n'], d['g'], d['cap'], d['nv'], d['width'],
                                     d['ld'], d['packed_main'], d['packed_gate'], d['eps'], d['out'], d['stream'])


@pytest.mark.parametrize('kw,word', [(dict(ld=160), b'ld'), (dict(ld=166), b'ld'), (dict(ld=4100), b'ld'), (dict(nv=9), b'nv'), (dict(nv=-1), b'nv'),
                                     (dict(h=None), b'null'), (dict(agg_main=None), b'null'), (dict(vars=None), b'null'),
                                     (dict(graph_ptr=None), b'null'), (dict(packed_main=None), b'null'), (dict(out=None), b'null'),
                                     (dict(agg_gate=None), b'gate'), (dict(packed_gate=None), b'gate'), (dict(n=-1), b'sizes'), (dict(g=-1), b'sizes'),
                                     (dict(cap=-1), b'sizes'), (dict(out=32772), b'aligned'), (dict(h=4100), b'aligned'),
                                     (dict(agg_gate=12292), b'aligned'), (dict(packed_main=24584), b'aligned')])
def test_argument_errors_are_return_codes(L, kw, word):
    rc = call(L, **kw)
    assert rc < 0 and rc != -2, kw
    assert word in L.msmp_last_error(), (kw, L.msmp_last_error())


def test_a_graph_or_a_width_outside_the_kernel_is_unsupported_not_an_error_of_the_arguments(L):
    cap = L.msmp_wide_node_tail_max_graph_nodes(164)
    assert call(L, cap=cap + 1) == -2 and b'max_graph_nodes' in L.msmp_last_error()
    assert call(L, width=0, ld=4) == -2 and b'width' in L.msmp_last_error()
    assert call(L, width=257, ld=260) == -2 and b'width' in L.msmp_last_error()
    assert call(L, n=0, g=0, cap=0) == 0                # no nodes: a valid call that launches nothing
    assert call(L, n=0, g=0, cap=0, agg_gate=None, packed_gate=None) == 0


def test_pack_refuses_bad_arguments_and_the_tune_key_exists(L):
    assert L.msmp_pack_wide_tail_f32(4096, 8192, 12288, 16384, 0, 2, 20480, None) < 0 and b'width' in L.msmp_last_error()
    assert L.msmp_pack_wide_tail_f32(4096, 8192, 12288, 16384, 257, 2, 20480, None) < 0
    assert L.msmp_pack_wide_tail_f32(4096, 8192, 12288, 16384, 164, 9, 20480, None) < 0 and b'nv' in L.msmp_last_error()
    assert L.msmp_pack_wide_tail_f32(None, 8192, 12288, 16384, 164, 2, 20480, None) < 0 and b'null' in L.msmp_last_error()
    default = L.msmp_tune_query(b'wide_tail')
    assert default in (0, 1)
    assert L.msmp_tune(b'wide_tail', 1 - default) == 0 and L.msmp_tune_query(b'wide_tail') == 1 - default
    assert L.msmp_tune(b'wide_tail', default) == 0 and L.msmp_tune_query(b'wide_tail') == default
