"""CPU tests (no kernel launched) of the width-generic layer backward entry: the header declares its two prototypes, the built library
exports them, the workspace query is positive for the sizes the entry takes and 0 for those it refuses by value, bad arguments are
refused by return value with msmp_last_error set, and the "wide_bwd" switch is documented, listed, settable and queryable."""
import ctypes
import os
import re

import pytest

from helpers import L, abi_versions_agree        # noqa: F401  (L: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('msmp_wide_layer_bwd_workspace_bytes', 'msmp_wide_layer_bwd_f32')


def test_header_declares_and_library_exports_the_entry(L):
    header = open(os.path.join(ROOT, 'include', 'msmp_pde.h')).read()
    for name in NAMES:
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert getattr(L, name) is not None
    assert abi_versions_agree(header, L)


@pytest.mark.parametrize('gated', [0, 1])
def test_workspace_query(L, gated):
    q = L.msmp_wide_layer_bwd_workspace_bytes
    assert q(236, 1000, 25, 3, 164, gated) > 0
    assert q(236, 0, 25, 3, 164, gated) > 0                              # an edgeless batch is a valid call
    assert q(236, 1000, 25, 3, 164, 1) > q(236, 1000, 25, 3, 164, 0)     # the second head has its own rows
    for width in (1, 96, 128, 132, 256):
        assert q(236, 1000, 25, 3, width, gated) > 0, width
    assert q(236, 1000, 119, 8, 256, gated) > 0                          # 128 feature columns at the widest layer: the caps themselves
    for width in (0, 257, -3):
        assert q(236, 1000, 25, 3, width, gated) == 0, width
    assert q(236, 1000, 120, 8, 164, gated) == 0                         # tw + 1 + nv = 129
    assert q(236, 1000, 25, 9, 164, gated) == 0                          # nv above MSMP_MAX_VARS
    assert q(0, 1000, 25, 3, 164, gated) == 0 and q(236, -1, 25, 3, 164, gated) == 0


def call(L, gated=True, **kw):
    """msmp_wide_layer_bwd_f32 on fake (never dereferenced: every case is refused before a launch) 16-byte aligned addresses; the
    parameter / gradient pointer arrays are real host arrays of fake addresses"""
    d = dict(grad_out=4096, h=8192, u=12288, pos=16384, vars=20480, rowptr=24576, col=28672, tgt=32768, src_rowptr=36864, src_perm=40960,
             graph_ptr=45056, n=236, e=1000, graphs=5, tw=25, nv=3, width=164, ld=256, eps=1e-5, dh=49152, ws=53248, ws_bytes=1 << 40,
             stream=None)
    d.update(kw)
    arr = lambda base: (ctypes.c_void_p * 8)(*[base + 4096 * i for i in range(8)])
    d.setdefault('params_main', arr(1 << 20))
    d.setdefault('grads_main', arr(2 << 20))
    d.setdefault('params_gate', arr(3 << 20) if gated else None)
    d.setdefault('grads_gate', arr(4 << 20) if gated else None)
    return L.msmp_wide_layer_bwd_f32(d['grad_out'], d['h'], d['u'], d['pos'], d['vars'], d['rowptr'], d['col'], d['tgt'], d['src_rowptr'],
                                     d['src_perm'], d['graph_ptr'], d['n'], d['e'], d['graphs'], d['tw'], d['nv'], d['width'], d['ld'],
                                     d['params_main'], d['params_gate'], d['eps'], d['dh'], d['grads_main'], d['grads_gate'], d['ws'],
                                     d['ws_bytes'], d['stream'])


@pytest.mark.parametrize('name', ['grad_out', 'h', 'u', 'pos', 'vars', 'rowptr', 'col', 'tgt', 'graph_ptr', 'dh', 'ws', 'params_main', 'grads_main'])
def test_null_pointers_are_argument_errors(L, name):
    assert call(L, **{name: None}) == -1
    assert b'null' in L.msmp_last_error(), (name, L.msmp_last_error())


def test_null_entries_of_the_pointer_arrays_and_half_a_gate(L):
    holed = (ctypes.c_void_p * 8)(*[None if i == 5 else 4096 * (i + 1) for i in range(8)])
    assert call(L, params_main=holed) == -1 and b'null' in L.msmp_last_error()
    assert call(L, grads_gate=holed) == -1 and b'null' in L.msmp_last_error()
    assert call(L, grads_gate=None) == -1 and b'gate' in L.msmp_last_error()


def test_sizes_outside_the_entry_are_unsupported_not_argument_errors(L):
    assert call(L, width=0, ld=128) == -2 and b'width' in L.msmp_last_error()
    assert call(L, width=257, ld=384) == -2 and b'width' in L.msmp_last_error()
    assert call(L, tw=120, nv=8) == -2                                   # 129 feature columns
    assert call(L, nv=9) == -2
    assert call(L, gated=False, width=300, ld=384) == -2


def test_the_by_source_arrays_are_required(L):
    for kw in (dict(src_rowptr=None), dict(src_perm=None), dict(src_rowptr=None, src_perm=None)):
        assert call(L, **kw) == -1, kw
        assert b'src_rowptr' in L.msmp_last_error()
        assert call(L, gated=False, **kw) == -1, kw


@pytest.mark.parametrize('kw,word', [(dict(ld=164), b'ld'), (dict(ld=384), b'ld'), (dict(width=128), b'ld'), (dict(h=8196), b'aligned'),
                                     (dict(grad_out=4100), b'aligned'), (dict(dh=49160), b'aligned'), (dict(n=0), b'sizes'), (dict(e=-1), b'sizes'),
                                     (dict(graphs=0), b'sizes'), (dict(tw=0), b'sizes'), (dict(nv=0), b'sizes'), (dict(ws_bytes=1024), b'workspace')])
def test_argument_errors_are_return_codes(L, kw, word):
    rc = call(L, **kw)
    assert rc < 0 and rc != -2, kw
    assert word in L.msmp_last_error(), (kw, L.msmp_last_error())


def test_the_switch_is_documented_listed_settable_and_queryable(L):
    header = open(os.path.join(ROOT, 'include', 'msmp_pde.h')).read()
    knobs = header[header.index('/* Knobs for A/B measurements'):header.index('int msmp_tune(const char* key, int value);')]
    entry = re.search(r'\n \*   "wide_bwd" (-?\d+) \(default\)', knobs)
    assert entry, 'the knob list does not document "wide_bwd" with its default'
    default = int(entry.group(1))
    assert L.msmp_tune_query(b'wide_bwd') == default
    try:
        for value in (0, 1, 2, 5):                      # any integer: != 0 selects the native backward
            assert L.msmp_tune(b'wide_bwd', value) == 0 and L.msmp_tune_query(b'wide_bwd') == value
    finally:
        L.msmp_tune(b'wide_bwd', default)
    assert L.msmp_tune_query(b'wide_bwd') == default
