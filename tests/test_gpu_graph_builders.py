"""The graph side against brute force (run with -m gpu on the MI355X): every kernel reads the graph through rowptr / col / tgt / graph_ptr,
so a wrong or missing edge gives a model that runs, stays finite and is silently wrong.

  * radius_graph / knn_graph (radius_kernel, knn_kernel, knn_degree_kernel, exclusive_scan_inplace_kernel of csrc/graph_kernels.hip) against
    the numpy oracle O.radius_graph / O.knn_graph (float64 per graph, stable sort, lower index on ties);
  * GraphStructure (msmp_build_csr: rocprim radix sort + csr_finish_kernel) and by_source() against a stable np.argsort;
  * the host-side caches of graph.py (structure_of, GraphCreator._edge_cache).

Every expectation is an integer array: every comparison is np.array_equal on the whole array, order included, and no tolerance exists.
The table of cases is in DESIGN.md section 4.9 ("Graph side")."""
import numpy as np
import pytest
import torch

from oracle import msmp_oracle as O
from helpers import mp       # noqa: F401  (module-scoped fixture: the built library on a GPU)

pytestmark = pytest.mark.gpu


def dev(a, dtype=None):
    t = torch.as_tensor(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def host(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------------------------
# 1. builders against the oracle
# ---------------------------------------------------------------------------------------------------------------------------------------
RADIUS = {1: 0.02, 2: 0.11, 3: 0.22}      # on uniform points of the unit cube: about 0.04 x (graph size) neighbours, ~4 at 100 nodes


def ragged_sizes(total, seed):
    """Graph sizes that sum to `total`: drawn from 1..139 with a 1-node and a 2-node graph near the front, the last graph trimmed to hit
    the total; some graph straddles every multiple of 1024 below the total (the chunk boundaries of the single-workgroup scan).  The
    seed is advanced until that holds, so the property is a fact of the returned sizes and not luck."""
    for s in range(seed, seed + 64):
        rng = np.random.default_rng(s)
        sizes = []
        while sum(sizes) < total:
            sizes.append(1 if len(sizes) == 1 else 2 if len(sizes) == 3 else int(rng.integers(1, 140)))
        sizes[-1] -= sum(sizes) - total
        ends = np.cumsum(sizes)
        starts = ends - np.array(sizes)
        if len(sizes) >= 4 and all(((starts < m) & (ends > m)).any() for m in range(1024, total, 1024)):
            return sizes
    raise AssertionError(f'no ragged partition of {total} nodes straddles every multiple of 1024')


def both_builders_equal_the_oracle(mp, x, batch, dim, ks=(1, 3, 6)):
    """(nodes, radius edges, knn edges per k) after the whole-array comparisons"""
    xd, bd = dev(x), dev(batch)
    want = O.radius_graph(x, RADIUS[dim], batch)
    got = host(mp.radius_graph(xd, RADIUS[dim], batch=bd))
    assert got.dtype == np.int64 and np.array_equal(got, want), ('radius', dim)
    assert want.shape[1] > len(x) // 2, 'the radius must give the nodes some neighbours'
    counts = [want.shape[1]]
    for k in ks:
        want = O.knn_graph(x, k, batch)
        got = host(mp.knn_graph(xd, k, batch=bd))
        assert got.dtype == np.int64 and np.array_equal(got, want), ('knn', k, dim)
        counts.append(want.shape[1])
    return counts


@pytest.mark.parametrize('dim', [1, 2])
@pytest.mark.parametrize('total', [255, 256, 257, 1023, 1024, 1025, 2048, 2049, 3 * 1024 + 517])
def test_builders_equal_the_oracle_around_the_scan_chunks(mp, total, dim):
    """Node counts around the 256-thread blocks of the per-node kernels and around the 1024-element chunks of the scan (one, two and four
    chunks: the carry between chunks decides where every later node's edges go), ragged graphs that straddle the chunk boundaries."""
    sizes = ragged_sizes(total, seed=total)
    assert sum(sizes) == total and 1 in sizes[:-1] and 2 in sizes[:-1]
    rng = np.random.default_rng(total + dim)
    x = rng.uniform(0, 1, (total, dim))
    batch = np.repeat(np.arange(len(sizes)), sizes)
    counts = both_builders_equal_the_oracle(mp, x, batch, dim)
    print(f'scan chunks: {total} nodes, {len(sizes)} graphs, dim {dim}: edges radius / knn 1, 3, 6 = {counts}')


def test_builders_equal_the_oracle_in_three_dimensions(mp):
    sizes = [17, 100, 3, 64, 1, 139, 2, 50]
    rng = np.random.default_rng(33)
    x = rng.uniform(0, 1, (sum(sizes), 3))
    counts = both_builders_equal_the_oracle(mp, x, np.repeat(np.arange(len(sizes)), sizes), 3)
    print(f'dim 3: {sum(sizes)} nodes: edges radius / knn 1, 3, 6 = {counts}')


CAP_SIZES = [5, 0, 1, 2, 7, 1, 33, 34, 35]


@pytest.mark.parametrize('dim', [1, 2, 3])
@pytest.mark.parametrize('k', [31, 32])
def test_knn_at_the_largest_k_with_graphs_smaller_than_k(mp, k, dim):
    """k at MAX_K and one below, graphs of fewer than k + 1 nodes (every other node is a neighbour), an empty graph (sizes=) whose id is
    simply absent from batch=: both forms equal the oracle."""
    n = sum(CAP_SIZES)
    batch = np.repeat(np.arange(len(CAP_SIZES)), CAP_SIZES)
    assert 1 not in batch
    x = np.random.default_rng(100 * k + dim).uniform(0, 1, (n, dim))
    want = O.knn_graph(x, k, batch)
    n_edges = sum(s * min(k, s - 1) for s in CAP_SIZES)
    assert n_edges == {31: 3226, 32: 3328}[k] and want.shape == (2, n_edges)
    by_sizes = host(mp.knn_graph(dev(x), k, sizes=CAP_SIZES))
    by_batch = host(mp.knn_graph(dev(x), k, batch=dev(batch)))
    assert by_sizes.shape == (2, n_edges) and np.array_equal(by_sizes, want)
    assert by_batch.shape == (2, n_edges) and np.array_equal(by_batch, want)


def test_knn_ties_and_coincident_points_take_the_lower_index(mp):
    lattice = np.array([[i, j] for i in range(4) for j in range(4)], dtype=np.float64)
    zeros = np.zeros(16, dtype=np.int64)
    for k in (2, 3):
        want = O.knn_graph(lattice, k, zeros)
        got = host(mp.knn_graph(dev(lattice), k, batch=dev(zeros)))
        assert np.array_equal(got, want), k
    assert want[0, want[1] == 0].tolist() == [1, 4, 5] and got[0, got[1] == 0].tolist() == [1, 4, 5]      # two at distance 1, then the diagonal
    x = np.array([0., 0., 0., 1., 1.])
    want = O.knn_graph(x, 2, np.zeros(5, dtype=np.int64))
    assert want[0].tolist() == [1, 2, 0, 2, 0, 1, 4, 0, 3, 0]       # coincident points are each other's nearest, lower index first
    assert np.array_equal(host(mp.knn_graph(dev(x), 2, batch=dev(np.zeros(5, dtype=np.int64)))), want)
    x = np.arange(10, dtype=np.float64)                             # equal distances left and right at every k
    for k in (2, 4, 6):
        want = O.knn_graph(x, k, np.zeros(10, dtype=np.int64))
        assert np.array_equal(host(mp.knn_graph(dev(x), k, batch=dev(np.zeros(10, dtype=np.int64)))), want), k


def test_a_pair_exactly_on_the_radius_is_excluded(mp):
    x = np.arange(6, dtype=np.float64)
    zeros = np.zeros(6, dtype=np.int64)
    want = O.radius_graph(x, 2.0, zeros)
    assert want.shape == (2, 10) and (np.abs(want[0] - want[1]) == 1).all()          # distance 2 is not < 2: the unit pairs only
    assert np.array_equal(host(mp.radius_graph(dev(x), 2.0, batch=dev(zeros))), want)
    want = O.radius_graph(x, 2.0 + 1e-12, zeros)
    assert want.shape == (2, 18)                                                     # ... and just above, the eight pairs at distance 2 too
    assert np.array_equal(host(mp.radius_graph(dev(x), 2.0 + 1e-12, batch=dev(zeros))), want)


@pytest.mark.parametrize('cap', [1, 4, 32])
def test_the_neighbour_cap_keeps_the_lowest_indices(mp, cap):
    """dense graphs (the radius covers a whole graph): every node has size - 1 candidates, the cap keeps the first `cap` of them"""
    sizes = [5, 33, 34, 40, 1, 12]
    batch = np.repeat(np.arange(len(sizes)), sizes)
    for dim in (1, 2):
        x = np.random.default_rng(cap + dim).uniform(0, 1, (sum(sizes), dim))
        want = O.radius_graph(x, 10.0, batch, max_num_neighbors=cap)
        assert want.shape[1] == sum(s * min(cap, s - 1) for s in sizes)
        got = host(mp.radius_graph(dev(x), 10.0, batch=dev(batch), max_num_neighbors=cap))
        assert np.array_equal(got, want), dim


def test_batches_without_any_edge(mp):
    from msmp_pde_amd.graph import GraphStructure
    rng = np.random.default_rng(9)
    sizes = [17, 1, 30]
    batch = np.repeat(np.arange(len(sizes)), sizes)
    x = rng.uniform(0, 1, (sum(sizes), 2))
    assert O.radius_graph(x, 1e-9, batch).shape == (2, 0)
    ones = np.arange(29)                                 # 29 graphs of one node each
    assert O.knn_graph(x[:29], 3, ones).shape == (2, 0)
    for ei, b in ((mp.radius_graph(dev(x), 1e-9, batch=dev(batch)), batch), (mp.knn_graph(dev(x[:29]), 3, batch=dev(ones)), ones)):
        assert ei.dtype == torch.int64 and tuple(ei.shape) == (2, 0) and ei.is_cuda
        gs = GraphStructure(ei, dev(b), len(b))
        assert np.array_equal(host(gs.rowptr), np.zeros(len(b) + 1, dtype=np.int32))
        assert gs.n_edges == 0 and gs.max_in_degree == 0 and gs.tiles() is None
        assert np.array_equal(host(gs.graph_ptr), np.concatenate(([0], np.cumsum(np.bincount(b)))))


def one_graph_pattern(exp, x0):
    """the oracle's edge_index of ONE graph of the experiment's grid (what O.create_graph builds per graph, common/utils.py:343-380)"""
    zeros = np.zeros(len(x0), dtype=np.int64)
    if exp == 'E2':
        return O.radius_graph(x0, 3 * (x0[1] - x0[0]) + 0.0001, zeros)
    if exp == 'WE3':
        return O.knn_graph(x0, 3, zeros)
    assert exp == 'RPU'
    xx = 2 * np.pi * x0 / (x0.max() - 1e-3)
    return O.knn_graph(np.stack([np.cos(xx), np.sin(xx)], 1), 3, zeros)


@pytest.mark.parametrize('exp', ['E2', 'WE3', 'RPU'])
def test_the_workload_size_edge_index_is_the_oracle_pattern_repeated(mp, exp):
    """2048 graphs of 100 nodes: 204 800 nodes are 200 chunks of the scan, so every carry is compared.  The oracle treats the graphs of a
    batch independently, so for identical graphs it returns one graph's pattern shifted by the node offsets: that array is built here
    without the oracle's Python loop over 204 800 nodes, and the WHOLE edge_index is compared with it."""
    from msmp_pde_amd.synthetic import make_pde, make_grid
    bsz, nx = 2048, 100
    x0 = torch.tensor(make_grid(exp, nx)).float().double()            # the grid of synthetic.make_case
    creator = mp.GraphCreator(make_pde(exp, 250, nx), neighbors=3, time_window=25, device='cuda')
    got = host(creator.build_edge_index(x0, bsz, 'cuda'))
    pattern = one_graph_pattern(exp, x0.numpy())
    want = (pattern[:, None, :] + nx * np.arange(bsz, dtype=np.int64)[None, :, None]).reshape(2, -1)
    print(f'workload size {exp}: {bsz * nx} nodes, {want.shape[1]} edges ({pattern.shape[1]} per graph)')
    assert got.shape == want.shape and np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------------------------------------------
# 2. msmp_build_csr / GraphStructure against numpy
# ---------------------------------------------------------------------------------------------------------------------------------------
def shuffled_edges(n_nodes, n_edges, seed):
    """[2, n_edges] int64 in arbitrary order with repeated pairs; the first 3, the last 4 and a middle band of the nodes are no edge's
    target (isolated rows at the start, in the middle and -- the `e == n_edges - 1` branch of csr_finish_kernel -- at the end)"""
    rng = np.random.default_rng(seed)
    mid = range(n_nodes // 2, n_nodes // 2 + max(2, n_nodes // 16))
    targets = np.array([v for v in range(3, n_nodes - 4) if v not in mid], dtype=np.int64)
    fresh = n_edges - n_edges // 8
    src = rng.integers(0, n_nodes, fresh)
    dst = targets[rng.integers(0, len(targets), fresh)]
    again = rng.integers(0, fresh, n_edges - fresh)                # every eighth edge repeats an earlier pair
    src, dst = np.concatenate([src, src[again]]), np.concatenate([dst, dst[again]])
    order = rng.permutation(n_edges)
    return np.stack([src[order], dst[order]]).astype(np.int64)


def ragged_batch(n_nodes, seed, largest=139):
    rng = np.random.default_rng(seed)
    sizes = []
    while sum(sizes) < n_nodes:
        sizes.append(int(rng.integers(1, largest + 1)))
    sizes[-1] -= sum(sizes) - n_nodes
    return np.repeat(np.arange(len(sizes)), sizes)


def csr_reference(ei, batch, n_nodes):
    order = np.argsort(ei[1], kind='stable')
    counts = np.bincount(batch)
    return dict(col=ei[0][order], tgt=ei[1][order], rowptr=np.concatenate(([0], np.cumsum(np.bincount(ei[1], minlength=n_nodes)))),
                max_in_degree=int(np.bincount(ei[1], minlength=n_nodes).max()), n_graphs=len(counts),
                graph_ptr=np.concatenate(([0], np.cumsum(counts))), max_graph_nodes=int(counts.max()))


def assert_structure(gs, ref):
    e = len(ref['col'])
    assert gs.n_edges == e
    for name in ('col', 'tgt'):
        got = host(getattr(gs, name))[:e]
        assert got.dtype == np.int32 and np.array_equal(got, ref[name]), name
    for name in ('rowptr', 'graph_ptr'):
        got = host(getattr(gs, name))
        assert got.dtype == np.int32 and np.array_equal(got, ref[name]), name
    assert (gs.max_in_degree, gs.n_graphs, gs.max_graph_nodes) == (ref['max_in_degree'], ref['n_graphs'], ref['max_graph_nodes'])


CSR_CASES = [(1, 9), (255, 40), (256, 300), (257, 64), (5000, 700), (1 << 20, 1 << 17)]


@pytest.fixture(scope='module', params=CSR_CASES, ids=lambda c: f'{c[0]}-edges-{c[1]}-nodes')
def csr_case(request):
    """(edge_index, batch, n_nodes, numpy reference), made once per size and shared; nobody changes it"""
    n_edges, n_nodes = request.param
    ei = shuffled_edges(n_nodes, n_edges, seed=n_edges)
    batch = ragged_batch(n_nodes, seed=n_nodes, largest=max(2, min(255, n_nodes // 3)))
    ref = csr_reference(ei, batch, n_nodes)
    if n_edges > 1:
        assert (np.diff(ei[1]) < 0).any() and ref['max_in_degree'] >= 2          # unsorted, and some target has several in-edges
        assert len(np.unique(ei.T, axis=0)) < n_edges                            # multi-edges
    assert ref['rowptr'][3] == 0 and ref['rowptr'][-5] == ref['rowptr'][-1] == n_edges      # isolated rows at both ends
    return ei, batch, n_nodes, ref


def test_csr_of_shuffled_edges_equals_a_stable_argsort(mp, csr_case):
    from msmp_pde_amd.graph import GraphStructure
    ei, batch, n, ref = csr_case
    gs = GraphStructure(dev(ei), dev(batch), n)
    print(f'csr: {ei.shape[1]} edges, {n} nodes, {ref["n_graphs"]} graphs, max in-degree {ref["max_in_degree"]}')
    assert_structure(gs, ref)


def test_by_source_regroups_the_csr_edges_stably(mp, csr_case):
    from msmp_pde_amd.graph import GraphStructure
    ei, batch, n, ref = csr_case
    gs = GraphStructure(dev(ei), dev(batch), n)
    perm, rowptr = gs.by_source()
    assert perm.dtype == torch.int64 and np.array_equal(host(perm), np.argsort(ref['col'], kind='stable'))
    want_rowptr = np.concatenate(([0], np.cumsum(np.bincount(ei[0], minlength=n))))
    assert rowptr.dtype == torch.int32 and np.array_equal(host(rowptr), want_rowptr)
    perm32, rowptr32 = gs.by_source32()
    assert perm32.dtype == torch.int32 and perm32.is_contiguous() and np.array_equal(host(perm32), host(perm))
    assert rowptr32.dtype == torch.int32 and np.array_equal(host(rowptr32), want_rowptr)
    assert gs.by_source()[0] is perm and gs.by_source32()[0] is perm32         # made once


def test_csr_of_int32_and_non_contiguous_edge_index(mp, csr_case):
    from msmp_pde_amd.graph import GraphStructure
    ei, batch, n, ref = csr_case
    if ei.shape[1] > 5000:
        ei, batch, n = ei[:, :5000], batch, n           # the input forms are host-side conversions: the large sort is covered above
        ref = csr_reference(ei, batch, n)
    assert_structure(GraphStructure(dev(ei, torch.int32), dev(batch), n), ref)
    transposed = dev(ei.T)                               # [E, 2] contiguous: its .t() is [2, E] with strides (1, 2)
    view = transposed.t()
    assert tuple(view.shape) == (2, ei.shape[1]) and (ei.shape[1] == 1 or not view.is_contiguous())
    assert_structure(GraphStructure(view, dev(batch), n), ref)
    assert_structure(GraphStructure(dev(ei.T, torch.int32).t(), dev(batch), n), ref)


def test_an_undersized_csr_workspace_is_refused_and_nothing_is_written(mp):
    from msmp_pde_amd._lib import ptr, current_stream
    L = mp.lib()
    n_edges, n_nodes = 257, 64
    ei = dev(shuffled_edges(n_nodes, n_edges, seed=1))
    need = L.msmp_build_csr_workspace_bytes(n_edges, n_nodes)
    assert need > 4 * 4 * n_edges
    sentinel = 0x5A5A5A5A
    rowptr = torch.full((n_nodes + 1,), sentinel, dtype=torch.int32, device='cuda')
    col = torch.full((n_edges,), sentinel, dtype=torch.int32, device='cuda')
    tgt = torch.full((n_edges,), sentinel, dtype=torch.int32, device='cuda')
    ws = torch.full((need,), 0x5A, dtype=torch.uint8, device='cuda')
    rc = L.msmp_build_csr(ptr(ei), n_edges, n_nodes, ptr(rowptr), ptr(col), ptr(tgt), ptr(ws), need - 1, current_stream())
    torch.cuda.synchronize()
    assert rc == -3 and b'workspace too small' in L.msmp_last_error()            # MSMP_ERR_WORKSPACE
    for t in (rowptr, col, tgt):
        assert bool((t == sentinel).all())
    assert bool((ws == 0x5A).all())
    rc = L.msmp_build_csr(ptr(ei), n_edges, n_nodes, ptr(rowptr), ptr(col), ptr(tgt), ptr(ws), need, current_stream())      # the exact size is enough
    assert rc == 0
    ref = csr_reference(host(ei), np.zeros(n_nodes, dtype=np.int64), n_nodes)
    assert np.array_equal(host(col), ref['col']) and np.array_equal(host(tgt), ref['tgt']) and np.array_equal(host(rowptr), ref['rowptr'])


# ---------------------------------------------------------------------------------------------------------------------------------------
# 4. host-side caches
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_structure_of_is_cached_and_rebuilt_when_the_graph_changes(mp):
    from msmp_pde_amd.graph import Data, structure_of
    n = 64
    ei = shuffled_edges(n, 257, seed=4)
    batch = ragged_batch(n, seed=4, largest=20)
    data = Data(x=torch.zeros(n, 1, device='cuda'), edge_index=dev(ei), batch=dev(batch))
    gs = structure_of(data)
    assert_structure(gs, csr_reference(ei, batch, n))
    assert structure_of(data) is gs                                  # nothing changed: the same object
    a, b = 0, int(np.nonzero(ei[1] != ei[1][0])[0][0])               # two columns with different targets
    data.edge_index[:, [a, b]] = data.edge_index[:, [b, a]]          # in place: same address, same shape
    ei2 = ei.copy()
    ei2[:, [a, b]] = ei[:, [b, a]]
    assert np.array_equal(host(data.edge_index), ei2) and not np.array_equal(ei2, ei)
    gs2 = structure_of(data)
    assert gs2 is not gs
    assert_structure(gs2, csr_reference(ei2, batch, n))
    assert structure_of(data) is gs2
    batch2 = ragged_batch(n, seed=5, largest=9)
    assert not np.array_equal(batch2, batch)
    data.batch = dev(batch2)                                         # replaced by another tensor
    gs3 = structure_of(data)
    assert gs3 is not gs2
    assert_structure(gs3, csr_reference(ei2, batch2, n))
    assert structure_of(data) is gs3


@pytest.mark.parametrize('exp', ['E2', 'WE3', 'RPU'])
def test_build_edge_index_serves_nothing_from_a_stale_key(mp, exp):
    """one grid, another grid of the same length, the first again, then the first at another batch size: each result is the oracle's for
    its own arguments (the cache keeps the last key only, and the key carries the grid's bytes and the batch size)"""
    from msmp_pde_amd.synthetic import make_pde
    nx = 23
    rng = np.random.default_rng(17)
    grid_a, grid_b = (np.linspace(0, 16, nx) + rng.uniform(-0.3, 0.3, nx) for _ in range(2))      # jittered, still ascending (spacing 0.73)
    assert (np.diff(grid_a) > 0).all() and (np.diff(grid_b) > 0).all()
    creator = mp.GraphCreator(make_pde(exp, 250, nx), neighbors=3, time_window=25, device='cuda')
    for grid, bsz in ((grid_a, 3), (grid_b, 3), (grid_a, 3), (grid_a, 5), (grid_a, 3)):
        pattern = one_graph_pattern(exp, grid)
        want = (pattern[:, None, :] + nx * np.arange(bsz, dtype=np.int64)[None, :, None]).reshape(2, -1)
        batch = np.repeat(np.arange(bsz), nx)
        x = np.tile(grid, bsz)
        if exp == 'E2':
            assert np.array_equal(want, O.radius_graph(x, 3 * (grid[1] - grid[0]) + 0.0001, batch))      # the oracle on the whole batch
        elif exp == 'WE3':
            assert np.array_equal(want, O.knn_graph(x, 3, batch))
        first = creator.build_edge_index(torch.tensor(grid), bsz, 'cuda')
        assert np.array_equal(host(first), want), bsz
        assert creator.build_edge_index(torch.tensor(grid), bsz, 'cuda') is first          # the same arguments again: cached
    assert not np.array_equal(one_graph_pattern(exp, grid_a), one_graph_pattern(exp, grid_b))
