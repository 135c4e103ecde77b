"""CPU tests (no kernel launched) of the graph builders' C-ABI (msmp_radius_graph_count_f64, msmp_radius_graph_fill_f64,
msmp_knn_graph_f64): a value outside what the kernels are built for is refused by return code before anything is launched, with a message
in msmp_last_error.  The pointers are fake addresses: a call that got as far as a launch would need a device, and the file runs without
one."""
import pytest

from helpers import L        # noqa: F401  (a fixture)

OK, ERR_ARG, ERR_UNSUPPORTED = 0, -1, -2          # include/msmp_pde.h


def call(L, entry, **kw):
    """one of the three builders on fake (never dereferenced) addresses; the defaults are a valid call of every entry"""
    d = dict(x=4096, dim=2, graph_ptr=8192, n_graphs=3, n_nodes=30, r=0.5, max_neighbors=32, k=3, rowptr=12288, n_edges=90, out=16384,
             stream=None)
    d.update(kw)
    if entry == 'count':
        return L.msmp_radius_graph_count_f64(d['x'], d['dim'], d['graph_ptr'], d['n_graphs'], d['n_nodes'], d['r'], d['max_neighbors'],
                                             d['rowptr'], d['stream'])
    if entry == 'fill':
        return L.msmp_radius_graph_fill_f64(d['x'], d['dim'], d['graph_ptr'], d['n_graphs'], d['n_nodes'], d['r'], d['max_neighbors'],
                                            d['rowptr'], d['n_edges'], d['out'], d['stream'])
    assert entry == 'knn'
    return L.msmp_knn_graph_f64(d['x'], d['dim'], d['graph_ptr'], d['n_graphs'], d['n_nodes'], d['k'], d['n_edges'], d['rowptr'], d['out'],
                                d['stream'])


def refused(L, entry, code, word, **kw):
    """the call returns `code` and leaves a message of its own (naming the entry and `word`) in msmp_last_error"""
    L.msmp_tune(b'no_such_knob', 1)                    # whatever an earlier refusal left is replaced: the message below is this call's
    assert b'unknown key' in L.msmp_last_error()
    assert call(L, entry, **kw) == code, (entry, kw)
    msg = L.msmp_last_error()
    name = {'count': b'msmp_radius_graph_count_f64', 'fill': b'msmp_radius_graph_fill_f64', 'knn': b'msmp_knn_graph_f64'}[entry]
    assert name in msg and word in msg, (entry, kw, msg)


ENTRIES = ('count', 'fill', 'knn')


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('dim', [0, 4, -1])
def test_a_dim_outside_1_to_3_is_an_argument_error(L, entry, dim):
    refused(L, entry, ERR_ARG, b'bad sizes', dim=dim)


@pytest.mark.parametrize('k', [0, 33, -1])
def test_a_k_outside_1_to_32_is_unsupported(L, k):
    refused(L, 'knn', ERR_UNSUPPORTED, b'k=%d outside 1..32' % k, k=k)


@pytest.mark.parametrize('entry,name', [(e, n) for e in ENTRIES for n in ('n_nodes', 'n_graphs', 'max_neighbors')
                                        if (e, n) != ('knn', 'max_neighbors')])          # msmp_knn_graph_f64 has no max_neighbors
def test_a_zero_count_is_an_argument_error(L, entry, name):
    refused(L, entry, ERR_ARG, b'bad sizes', **{name: 0})


@pytest.mark.parametrize('entry', ENTRIES)
@pytest.mark.parametrize('name', ['x', 'graph_ptr', 'rowptr'])
def test_a_null_input_is_an_argument_error(L, entry, name):
    refused(L, entry, ERR_ARG, b'null pointer', **{name: None})


@pytest.mark.parametrize('entry', ['fill', 'knn'])
def test_a_null_output_with_edges_to_write_is_an_argument_error(L, entry):
    refused(L, entry, ERR_ARG, b'null output', out=None, n_edges=1)
    refused(L, entry, ERR_ARG, b'null output', out=None)


def test_a_negative_edge_count_is_an_argument_error(L):
    refused(L, 'fill', ERR_ARG, b'bad sizes', n_edges=-1)
    refused(L, 'knn', ERR_ARG, b'bad sizes', n_edges=-1)


def test_radius_fill_of_no_edges_needs_no_output(L):
    """not a refusal: the count found no pair, there is nothing to write and nothing is launched"""
    assert call(L, 'fill', n_edges=0, out=None) == OK
    assert call(L, 'fill', n_edges=0) == OK
