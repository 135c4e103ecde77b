"""CPU tests (no kernel launched) of the gradient-gate entries (g2_gate_kernel.hip): the header declares the three prototypes and the switch
"g2_gate", the built library exports them at the ABI version of the header, every bad argument is refused by return value with msmp_last_error
naming the entry and the argument, widths that are no multiple of 4 in 4 .. 256 are refused by value as unsupported, and the switch stores
the value it is given."""
import os
import re
import sys

import pytest

from helpers import L, abi_versions_agree        # noqa: F401  (L: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, BWD, WS = 'msmp_g2_gate_blend_f32', 'msmp_g2_gate_blend_bwd_f32', 'msmp_g2_gate_blend_bwd_workspace_bytes'
FWD_POINTERS = ('h', 'gate', 'main', 'out_rowptr', 'out_nbr', 'out')           # tau_out may be NULL: tau is then not saved
BWD_POINTERS = ('grad_out', 'h', 'gate', 'main', 'tau', 'out_rowptr', 'out_nbr', 'in_rowptr', 'in_col', 'dh', 'da', 'db', 'workspace')


def call(L, name, **kw):
    """the entry on fake (never dereferenced: every case is refused before a launch) 16-byte aligned addresses"""
    d = dict(grad_out=4096, h=8192, gate=12288, main=16384, tau=20480, ld=128, out_rowptr=24576, out_nbr=28672, in_rowptr=32768, in_col=36864,
             n=10, e=30, width=128, out=40960, tau_out=45056, dh=49152, da=53248, db=57344, workspace=61440, workspace_bytes=10 * 128 * 4,
             stream=None)
    d.update(kw)
    if name == FWD:
        return L.msmp_g2_gate_blend_f32(d['h'], d['gate'], d['main'], d['ld'], d['out_rowptr'], d['out_nbr'], d['n'], d['e'], d['width'], d['out'],
                                        d['tau_out'], d['stream'])
    return L.msmp_g2_gate_blend_bwd_f32(d['grad_out'], d['h'], d['gate'], d['main'], d['tau'], d['ld'], d['out_rowptr'], d['out_nbr'],
                                        d['in_rowptr'], d['in_col'], d['n'], d['e'], d['width'], d['dh'], d['da'], d['db'], d['workspace'],
                                        d['workspace_bytes'], d['stream'])


def test_header_declares_and_library_exports_the_entries(L):
    header = open(os.path.join(ROOT, 'include', 'msmp_pde.h')).read()
    for name in (FWD, BWD, WS):
        assert re.search(r'\b(int|size_t)\s+' + name + r'\s*\(', header), name
        assert getattr(L, name) is not None
    assert abi_versions_agree(header, L)
    knobs = header[header.index('/* Knobs for A/B measurements'):header.index('int msmp_tune(const char* key, int value);')]
    assert re.search(r'"g2_gate" (-?\d+) \(default\)', knobs).group(1) == '1'        # documented with its default ...
    import subprocess
    child = 'import ctypes, sys; print(ctypes.CDLL(sys.argv[1]).msmp_tune_query(b"g2_gate"))'
    import msmp_pde_amd
    fresh = subprocess.run([sys.executable, '-c', child, msmp_pde_amd.LIB_PATH], capture_output=True, text=True, timeout=120)
    assert fresh.returncode == 0 and fresh.stdout.split()[-1] == '1', fresh.stderr[-2000:]      # ... which a fresh library reports


@pytest.mark.parametrize('name,pointer', [(FWD, p) for p in FWD_POINTERS] + [(BWD, p) for p in BWD_POINTERS])
def test_null_pointers_are_argument_errors(L, name, pointer):
    assert call(L, name, **{pointer: None}) == -1, (name, pointer)
    err = L.msmp_last_error()
    assert b'null' in err and err.startswith(name.encode() + b':') and pointer.encode() in err, err


def test_tau_out_may_be_null_but_not_misaligned(L):
    assert call(L, FWD, tau_out=45060) == -1 and b'tau_out' in L.msmp_last_error()
    assert call(L, FWD, tau_out=None, n=0) == -1 and b'n_nodes' in L.msmp_last_error()        # NULL itself is accepted: refused for n_nodes


@pytest.mark.parametrize('name', [FWD, BWD])
@pytest.mark.parametrize('n', [0, -1, 1 << 31, 1 << 40])
def test_node_counts_outside_the_range_are_argument_errors(L, name, n):
    assert call(L, name, n=n) == -1, (name, n)
    assert b'n_nodes' in L.msmp_last_error() and name.encode() in L.msmp_last_error()


@pytest.mark.parametrize('name', [FWD, BWD])
@pytest.mark.parametrize('e', [-1, 1 << 31])
def test_edge_counts_outside_the_range_are_argument_errors(L, name, e):
    assert call(L, name, e=e) == -1, (name, e)
    assert b'n_edges' in L.msmp_last_error()


@pytest.mark.parametrize('name', [FWD, BWD])
@pytest.mark.parametrize('width,ld', [(128, 124), (128, 0), (128, -128), (128, 130), (164, 166), (4, 2), (256, 252)])
def test_a_row_stride_below_the_row_or_no_multiple_of_four_is_an_argument_error(L, name, width, ld):
    assert call(L, name, width=width, ld=ld) == -1, (name, width, ld)
    assert b'ld' in L.msmp_last_error() and name.encode() in L.msmp_last_error()


@pytest.mark.parametrize('name', [FWD, BWD])
@pytest.mark.parametrize('width', [0, 2, 130, 260, -4])
def test_other_widths_are_unsupported_not_an_error_of_the_arguments(L, name, width):
    assert call(L, name, width=width, ld=512) == -2, (name, width)
    assert b'width' in L.msmp_last_error() and name.encode() in L.msmp_last_error()
    assert L.msmp_g2_gate_blend_bwd_workspace_bytes(10, width) == 0


def test_the_workspace_is_one_node_sized_tensor_and_a_smaller_one_is_refused(L):
    assert L.msmp_g2_gate_blend_bwd_workspace_bytes(10, 128) == 10 * 128 * 4
    assert L.msmp_g2_gate_blend_bwd_workspace_bytes(7, 164) == 7 * 164 * 4
    assert L.msmp_g2_gate_blend_bwd_workspace_bytes(0, 128) == 0 and L.msmp_g2_gate_blend_bwd_workspace_bytes(1 << 31, 128) == 0
    assert call(L, BWD, workspace_bytes=10 * 128 * 4 - 1) == -3 and b'workspace' in L.msmp_last_error()


def test_the_switch_stores_the_value_it_is_given(L):
    before = L.msmp_tune_query(b'g2_gate')
    try:
        for value in (0, 1, 2, 5):
            assert L.msmp_tune(b'g2_gate', value) == 0, (value, L.msmp_last_error())
            assert L.msmp_tune_query(b'g2_gate') == value
    finally:
        L.msmp_tune(b'g2_gate', before)
    assert L.msmp_tune_query(b'g2_gate') == before
