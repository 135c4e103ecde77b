"""CPU tests (no kernel launched) of the fused width-generic projection entry: the header declares its three prototypes, the built library
exports them, the blob size follows the padded width and the tail's K = 16 steps, and bad arguments are refused by return value with
msmp_last_error set."""
import os
import re

import pytest

from helpers import L, abi_versions_agree        # noqa: F401  (L: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('msmp_packed_wide_proj_floats', 'msmp_pack_wide_proj_f32', 'msmp_wide_node_proj_f32')


def test_header_declares_and_library_exports_the_entry(L):
    header = open(os.path.join(ROOT, 'include', 'msmp_pde.h')).read()
    for name in NAMES:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert getattr(L, name) is not None
    assert abi_versions_agree(header, L)
    assert '"wide_proj"' in header


def test_blob_size_is_positive_and_grows_with_the_width(L):
    last = 0
    for width in range(1, 257):
        kt = (width + 31) // 32
        for tw, nv in ((25, 1), (25, 3), (50, 5), (100, 8), (1, 1), (119, 8)):
            ts = (tw + 1 + nv + 15) // 16
            # scales | b1 [Wp] | per wave (KT) the P and Q streams, hi + lo, over 2 KT + TS k-steps
            assert L.msmp_packed_wide_proj_floats(width, tw, nv) == 8 + 32 * kt + 1024 * kt * (2 * kt + ts), (width, tw, nv)
        size = L.msmp_packed_wide_proj_floats(width, 25, 2)
        assert size > 0 and size >= last and (size > last) == (width % 32 == 1), width
        last = size


@pytest.mark.parametrize('args,word', [((0, 25, 2), b'width'), ((257, 25, 2), b'width'), ((-5, 25, 2), b'width'), ((164, 0, 2), b'tw'),
                                       ((164, 25, 0), b'nv'), ((164, 25, 9), b'nv'), ((164, 120, 8), b'tail'), ((164, 127, 1), b'tail')])
def test_blob_size_is_zero_outside_the_ranges(L, args, word):
    assert L.msmp_packed_wide_proj_floats(164, 126, 1) > 0                  # 128 feature columns: the cap itself
    assert L.msmp_packed_wide_proj_floats(*args) == 0
    assert word in L.msmp_last_error(), (args, L.msmp_last_error())


def call(L, **kw):
    """msmp_wide_node_proj_f32 on fake (never dereferenced: every case is refused before a launch) 16-byte aligned addresses"""
    d = dict(h=4096, feat=8192, n=10, tw=25, nv=2, width=164, ld=256, packed_main=12288, packed_gate=16384, p_main=20480, q_main=24576,
             p_gate=28672, q_gate=32768, stream=None)
    d.update(kw)
    return L.msmp_wide_node_proj_f32(d['h'], d['feat'], d['n'], d['tw'], d['nv'], d['width'], d['ld'], d['packed_main'], d['packed_gate'],
                                     d['p_main'], d['q_main'], d['p_gate'], d['q_gate'], d['stream'])


@pytest.mark.parametrize('kw,word', [(dict(ld=160), b'ld'), (dict(ld=166), b'ld'), (dict(ld=4100), b'ld'), (dict(nv=9), b'nv'), (dict(nv=0), b'nv'),
                                     (dict(tw=0), b'tw'), (dict(h=None), b'null'), (dict(feat=None), b'null'), (dict(packed_main=None), b'null'),
                                     (dict(p_main=None), b'null'), (dict(q_main=None), b'null'), (dict(packed_gate=None), b'gate'),
                                     (dict(p_gate=None), b'gate'), (dict(q_gate=None), b'gate'), (dict(packed_gate=None, p_gate=None), b'gate'),
                                     (dict(n=-1), b'sizes'), (dict(h=4100), b'aligned'), (dict(feat=8196), b'aligned'), (dict(q_main=24580), b'aligned'),
                                     (dict(p_gate=28680), b'aligned'), (dict(packed_main=12296), b'aligned')])
def test_argument_errors_are_return_codes(L, kw, word):
    rc = call(L, **kw)
    assert rc < 0 and rc != -2, kw
    assert word in L.msmp_last_error(), (kw, L.msmp_last_error())


def test_a_width_or_a_tail_outside_the_kernel_is_unsupported_not_an_error_of_the_arguments(L):
    assert call(L, width=0, ld=4) == -2 and b'width' in L.msmp_last_error()
    assert call(L, width=257, ld=260) == -2 and b'width' in L.msmp_last_error()
    assert call(L, tw=120, nv=8) == -2 and b'tail' in L.msmp_last_error()           # 129 feature columns
    assert call(L, n=0) == 0                            # no nodes: a valid call that launches nothing
    assert call(L, n=0, packed_gate=None, p_gate=None, q_gate=None) == 0


def test_pack_refuses_bad_arguments_and_the_tune_key_exists(L):
    assert L.msmp_pack_wide_proj_f32(4096, 8192, 0, 25, 2, 12288, None) < 0 and b'width' in L.msmp_last_error()
    assert L.msmp_pack_wide_proj_f32(4096, 8192, 257, 25, 2, 12288, None) < 0
    assert L.msmp_pack_wide_proj_f32(4096, 8192, 164, 25, 9, 12288, None) < 0 and b'nv' in L.msmp_last_error()
    assert L.msmp_pack_wide_proj_f32(4096, 8192, 164, 120, 8, 12288, None) < 0 and b'tail' in L.msmp_last_error()
    assert L.msmp_pack_wide_proj_f32(None, 8192, 164, 25, 2, 12288, None) < 0 and b'null' in L.msmp_last_error()
    default = L.msmp_tune_query(b'wide_proj')
    assert default in (0, 1)
    assert L.msmp_tune(b'wide_proj', 1 - default) == 0 and L.msmp_tune_query(b'wide_proj') == 1 - default
    assert L.msmp_tune(b'wide_proj', default) == 0 and L.msmp_tune_query(b'wide_proj') == default
