"""CPU tests (no kernel launched) of the fused width-generic message entry: the header declares its four prototypes, the built library
exports them, the blob size follows the padded width, the in-degree cap covers the reference's radius graphs at every width, and bad
arguments are refused by return value with msmp_last_error set."""
import os
import re

import pytest

from helpers import L, abi_versions_agree        # noqa: F401  (L: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('msmp_packed_wide_msg_floats', 'msmp_pack_wide_msg_f32', 'msmp_wide_message_max_in_degree', 'msmp_wide_message_f32')


def test_header_declares_and_library_exports_the_entry(L):
    header = open(os.path.join(ROOT, 'include', 'msmp_pde.h')).read()
    for name in NAMES:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert getattr(L, name) is not None
    assert abi_versions_agree(header, L)
    assert '"wide_msg"' in header


def test_blob_size_is_positive_inside_the_width_range_only(L):
    for width in range(1, 257):
        kt = (width + 31) // 32
        assert L.msmp_packed_wide_msg_floats(width) == 8 + 32 * kt + 1024 * kt * kt, width     # scales | bias | W2 hi + lo
    for width in (0, 257, -5):
        assert L.msmp_packed_wide_msg_floats(width) == 0
        assert b'width' in L.msmp_last_error()


def test_degree_cap_covers_the_radius_graphs_at_every_width(L):
    for width in range(1, 257):
        assert L.msmp_wide_message_max_in_degree(width) >= 32, width      # torch_cluster's neighbour cap in the reference's radius graphs


def call(L, **kw):
    """msmp_wide_message_f32 on fake (never dereferenced: every case is refused before a launch) 16-byte aligned addresses"""
    d = dict(p=4096, q=8192, rowptr=12288, col=16384, n=10, e=20, deg=4, width=164, ld=256, packed=20480, out=24576, stream=None)
    d.update(kw)
    return L.msmp_wide_message_f32(d['p'], d['q'], d['rowptr'], d['col'], d['n'], d['e'], d['deg'], d['width'], d['ld'], d['packed'], d['out'],
                                   d['stream'])


@pytest.mark.parametrize('kw,word', [(dict(width=0), b'width'), (dict(width=257, ld=260), b'width'), (dict(ld=160), b'ld'), (dict(ld=166), b'ld'),
                                     (dict(packed=None), b'null'), (dict(p=None), b'null'), (dict(out=None), b'null'), (dict(n=-1), b'sizes'),
                                     (dict(out=24580), b'aligned')])
def test_argument_errors_are_return_codes(L, kw, word):
    rc = call(L, **kw)
    assert rc < 0 and rc != -2, kw
    assert word in L.msmp_last_error(), (kw, L.msmp_last_error())


def test_a_degree_above_the_cap_is_unsupported_not_an_error_of_the_arguments(L):
    cap = L.msmp_wide_message_max_in_degree(164)
    assert call(L, deg=cap + 1) == -2 and b'max_in_degree' in L.msmp_last_error()
    assert call(L, n=0, e=0, deg=0) == 0                # no nodes: a valid call that launches nothing


def test_pack_refuses_bad_arguments_and_the_tune_key_exists(L):
    assert L.msmp_pack_wide_msg_f32(4096, 8192, 0, 12288, None) < 0 and b'width' in L.msmp_last_error()
    assert L.msmp_pack_wide_msg_f32(4096, 8192, 257, 12288, None) < 0
    assert L.msmp_pack_wide_msg_f32(None, 8192, 164, 12288, None) < 0 and b'null' in L.msmp_last_error()
    default = L.msmp_tune_query(b'wide_msg')
    assert default in (0, 1)
    assert L.msmp_tune(b'wide_msg', 1 - default) == 0 and L.msmp_tune_query(b'wide_msg') == 1 - default
    assert L.msmp_tune(b'wide_msg', default) == 0
