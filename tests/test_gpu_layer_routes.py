"""Every route of msmp_mp_layer_f32 (the 128-wide layer entry point, csrc/aux_kernels.hip) against the float64 oracle.

The entry point is a dispatcher: from the tune switches, the largest in-degree, the largest graph, the edges-per-tile ratio, the
DENSE_MESSAGE flag and whether the layer is gated it picks one of about a dozen kernel chains, and places every intermediate in
one workspace by pointer arithmetic.  The pieces have tests of their own (test_gpu_kernels.py); here the COMPOSITION is held to
the oracle on the smallest structures that separate the routes, and the library's own launch counters (helpers.launch_counts)
witness which chain ran.  DESIGN.md section 4.9 carries the same route table.

Bars (taken from the project as they stand): 2e-5 absolute on a composite layer (test_fused_aggregate_degree_limits,
test_wide_layer_pieces_vs_oracle), 2e-4 where the batch holds a graph of 2 to 29 nodes (test_node_tail_vs_oracle: InstanceNorm
over a few nodes divides by a standard deviation that can be tiny, which amplifies the fp32 rounding of the pre-norm values)."""
import numpy as np
import pytest
import torch

from oracle import msmp_oracle as O
from helpers import mp, tuned, launch_counts, banded_batch, hub_batch, oracle_layer, record_parity      # noqa: F401  (mp: fixture)

pytestmark = pytest.mark.gpu

H, TW, NV = 128, 25, 2
BAR, BAR_SMALL_GRAPH = 2e-5, 2e-4
FAMILIES = ('EDGE_MLP', 'NODE_PROJ', 'SCATTER_MEAN', 'NODE_UPDATE', 'NORM')        # the order of the count tuples below
CUT = 76        # edges per tile below which msmp_mp_layer_f32 leaves the tiles ("tile" 2)


def bar_of(sizes):
    return BAR_SMALL_GRAPH if any(2 <= s <= 29 for s in sizes) else BAR


# ---------------------------------------------------------------------------------------------------------------------------
# Structures: name -> (sizes, builder).  Built once per module, with their inputs; never modified afterwards.
# ---------------------------------------------------------------------------------------------------------------------------
A_SIZES = (100, 37, 64, 1, 128, 105)
STRUCTURES = {
    'A': (A_SIZES, lambda: banded_batch(A_SIZES, 3)),                                  # dense tiles: in-degree 6, largest graph 128, not periodic
    'A105': ((100, 37, 64, 1, 105), lambda: banded_batch((100, 37, 64, 1, 105), 3)),   # A with largest graph 105: the first size of RPT = 16
    'B': (A_SIZES, lambda: banded_batch(A_SIZES, 1)),                                  # sparse tiles: in-degree 2, under the cut of 76 edges per tile
    'C': ((100, 256, 37), lambda: hub_batch((100, 256, 37), 3, 1, 200)[:2]),           # hub of in-degree 200, distinct sources, largest graph 256
    'C128': ((100, 128, 37), lambda: hub_batch((100, 128, 37), 3, 1, 200)[:2]),        # the same hub inside a 128-node graph (multi-edges)
    'D': ((100, 128, 37), lambda: hub_batch((100, 128, 37), 3, 1, 300)[:2]),           # hub of in-degree 300 (multi-edges), graphs <= 128
    'D400': ((400, 37), lambda: hub_batch((400, 37), 3, 0, 300)[:2]),                  # hub of in-degree 300, distinct sources, a 400-node graph
    'E': ((5, 1, 30), lambda: banded_batch((5, 1, 30), 0)),                            # no edges at all
    'F': ((33,) * 9, lambda: banded_batch((33,) * 9, 3)),                              # periodic; a tile straddles graphs unless tile_align
}
MAX_IN_DEGREE = {'A': 6, 'A105': 6, 'B': 2, 'C': 200, 'C128': 200, 'D': 300, 'D400': 300, 'E': 0, 'F': 6}
_cache = {}


class _Structure(object):
    pass


def structure(mp_, name, align=0):
    """The named structure with its GraphStructure (tiles built under tile_align = align) and fp32 inputs on the GPU."""
    key = ('structure', name, align)
    if key not in _cache:
        from msmp_pde_amd.graph import GraphStructure
        s = _Structure()
        s.name = name
        s.sizes, build = STRUCTURES[name]
        s.ei, s.batch = build()
        s.n = len(s.batch)
        s.gs = GraphStructure(torch.tensor(s.ei).cuda(), torch.tensor(s.batch).cuda(), s.n)
        with tuned(mp_.lib(), tile_align=align):
            s.tiles = s.gs.tiles()
        s.args = inputs(s.n, seed=17 + len(name) + 31 * sum(s.sizes))
        _cache[key] = s
    return _cache[key]


def inputs(n, seed):
    """like the tiled-kernel tests: h standard normal, u 0.3 x standard normal, pos and vars uniform in [0, 1)"""
    rng = np.random.default_rng(seed)
    f = lambda a: torch.tensor(a, dtype=torch.float32).cuda()
    return (f(rng.standard_normal((n, H))), f(rng.standard_normal((n, TW)) * 0.3), f(rng.uniform(0, 1, (n, 1))),
            f(rng.uniform(0, 1, (n, NV))))


def layers_of(mp_, form):
    """(main, gate) of a layer form, default-initialised from a fixed seed; the same modules in every cell"""
    key = ('layers', form)
    if key not in _cache:
        torch.manual_seed({'residual': 101, 'lin': 102, 'gated': 103}[form])
        main = (mp_.GNN_Layer if form == 'residual' else mp_.GNN_LayerLin)(H, H, H, TW, NV).cuda()
        gate = mp_.GNN_LayerLin(H, H, H, TW, NV).cuda() if form == 'gated' else None
        _cache[key] = (main, gate)
    return _cache[key]


def reference(mp_, form, s):
    """float64 oracle on the same fp32 inputs and weights, once per (form, structure)"""
    key = ('reference', form, s.name)
    if key not in _cache:
        main, gate = layers_of(mp_, form)
        if form == 'residual':
            sd = {k: v.detach().double().cpu().numpy() for k, v in main.state_dict().items()}
            ref = O.mp_layer(O.layer_params(sd, ''), *[t.double().cpu().numpy() for t in s.args], s.ei, s.batch, lin=False)
        else:
            ref = oracle_layer(main, gate, s.args, s.ei, s.batch)
        ref.setflags(write=False)
        _cache[key] = ref
    return _cache[key]


def run_layer(mp_, form, s):
    """one mp_layer call under the switches in force: (output, launch counts in the order of FAMILIES, range status)"""
    main, gate = layers_of(mp_, form)
    main.packed()
    if gate is not None:
        gate.packed()           # the pack kernels are no part of the layer's chain: run them before the counters start
    L = mp_.lib()
    torch.empty_like(s.args[0]).fill_(float('nan'))     # freed at once: the block the layer's output most likely takes starts as NaN, not as an earlier cell's result
    with torch.no_grad(), launch_counts(L) as counts:
        out = mp_.mp_layer(*s.args, s.gs, main, gate)
    torch.cuda.synchronize()
    assert counts['LEM'] == 0 and counts['DECODER'] == 0
    return out, tuple(counts[f] for f in FAMILIES), mp_.last_status(reset=True)


# ---------------------------------------------------------------------------------------------------------------------------
# The route matrix.  One row per (structure, switches): the launches EDGE_MLP / NODE_PROJ / SCATTER_MEAN / NODE_UPDATE / NORM of the
# gated pair and of a plain layer (None: the form is not run on that row), read from msmp_mp_layer_f32 and the timing_begin sites
# of mlp_kernels.hip / tile_kernels.hip, with the reason.  `same`: further switch settings whose output the code promises to be
# bit-identical to the row's (gated form only where they are pair settings).
# msmp_edge_aggregate_tiled_f32 launches no feature-packing kernel of its own: with feat = NULL the folded kernel reads u / pos / vars.
# ---------------------------------------------------------------------------------------------------------------------------
class Row(object):
    def __init__(self, id, name, switches, gated, plain, why, same=(), same_gated=(), align=0):
        self.id, self.name, self.switches, self.gated, self.plain, self.why = id, name, switches, gated, plain, why
        self.same, self.same_gated, self.align = same, same_gated, align


TILED_PAIR, TILED_HEADS, TILED_PLAIN = (1, 0, 0, 1, 0), (2, 0, 0, 1, 0), (1, 0, 0, 1, 0)
GATHER_PAIR, GATHER_HEADS, GATHER_PLAIN = (1, 1, 0, 1, 0), (2, 2, 0, 1, 0), (1, 1, 0, 1, 0)
ROWS = [
    Row('A-defaults', 'A', {}, TILED_PAIR, TILED_PLAIN, 'tile 2 at >= 76 edges per tile: folded tile kernel, both heads in one launch; fused tail',
        same_gated=({'pair': 2},)),
    Row('A-pair0', 'A', {'pair': 0}, TILED_HEADS, None, 'the folded tile kernel once per head', same_gated=({'pair': 1}, {'pair': 2})),
    Row('A-tile1', 'A', {'tile': 1}, (2, 2, 0, 1, 0), (1, 1, 0, 1, 0), 'staged P / Q rows (pbuf, qbuf) per head: no pair route for tile 1'),
    Row('A-tile0', 'A', {'tile': 0}, GATHER_PAIR, GATHER_PLAIN, 'gather kernels; the pair projects both heads in one launch, aggregates in one',
        same_gated=({'tile': 0, 'pair': 2},)),
    Row('A-tile0-pair0', 'A', {'tile': 0, 'pair': 0}, GATHER_HEADS, None, 'projection + message kernel per head',
        same_gated=({'tile': 0, 'pair': 1}, {'tile': 0, 'pair': 2})),
    Row('A-tile0-edge_nb2', 'A', {'tile': 0, 'edge_nb': 2}, GATHER_HEADS, GATHER_PLAIN, '256-edge tiles; the pair route refuses edge_nb 2'),
    Row('A-tile_arith0', 'A', {'tile_arith': 0}, TILED_PAIR, TILED_PLAIN, 'ranged tiles read through the node list', same=({'tile_arith': 1},)),
    Row('A-tail0', 'A', {'tail': 0}, (2, 0, 0, 2, 1), (1, 0, 0, 1, 1),
        'chain: the pair routes sit inside the tail branch, so per head tile kernel + node_update, then gate_blend / instance_norm <16>'),
    Row('A105-tail0', 'A105', {'tail': 0}, (2, 0, 0, 2, 1), (1, 0, 0, 1, 1), 'the chain with the norm kernels at their first RPT = 16 size'),
    Row('A-dense', 'A', {'DENSE_MESSAGE': True}, (2, 0, 0, 1, 0), (1, 0, 0, 1, 0), 'per-edge message_net_1 (msmp_edge_aggregate_f32) per head; fused tail'),
    Row('A-split0', 'A', {'split': 0}, (2, 2, 0, 2, 1), (1, 1, 0, 1, 1), 'fp32-MFMA kernels: no tiles, no tail, no pair'),
    Row('B-defaults', 'B', {}, GATHER_PAIR, GATHER_PLAIN, 'under 76 edges per tile the tiles are left: as A tile 0'),
    Row('B-tile3', 'B', {'tile': 3}, TILED_PAIR, TILED_PLAIN, 'tile 3 forces the tiles below the cut: as A defaults'),
    Row('C-defaults', 'C', {}, (2, 2, 0, 2, 1), (1, 1, 0, 1, 1), 'in-degree 200 does not tile; 256-node graph: chain; 256-edge gather kernel per head'),
    Row('C128-defaults', 'C128', {}, GATHER_HEADS, GATHER_PLAIN, 'the pair route refuses in-degree above 128: per-head gather kernels, fused tail'),
    Row('D-defaults', 'D', {}, (2, 0, 2, 1, 0), (1, 0, 1, 1, 0), 'in-degree above 256: message tensor + scatter into pre_gate and agg (workspace shifted by msg), fused tail'),
    Row('D400-defaults', 'D400', {}, None, (1, 0, 1, 1, 1), 'message tensor + scatter, 400-node graph: chain'),
    Row('E-defaults', 'E', {}, (0, 2, 0, 1, 0), (0, 1, 0, 1, 0), 'no edges: the aggregate is a memset, but the projection ahead of it is still launched per head'),
    Row('F-align0', 'F', {}, TILED_PAIR, TILED_PLAIN, 'tiles straddle the 33-node graphs'),
    Row('F-align1', 'F', {}, TILED_PAIR, TILED_PLAIN, 'periodic descriptor, tiles cut at graph boundaries', align=1),
]


def test_structures_are_what_the_rows_assume(mp):
    """Preconditions of the matrix, from the descriptors: the largest in-degrees and graphs, which structures tile, and on which side
    of the 76-edges-per-tile cut they are."""
    for name, (sizes, _) in STRUCTURES.items():
        s = structure(mp, name)
        assert s.gs.max_in_degree == MAX_IN_DEGREE[name] and s.gs.max_graph_nodes == max(sizes) and s.gs.n_graphs == len(sizes), name
        assert np.array_equal(s.batch[s.ei[0]], s.batch[s.ei[1]]), 'every edge stays inside its graph'
        deg = np.bincount(s.ei[1], minlength=s.n)
        assert (deg == 0).any() == (1 in sizes or name == 'E'), 'nodes without in-edges: the 1-node graphs, and all of E'
        assert (s.tiles is not None) == (name in ('A', 'A105', 'B', 'F')), name
        print(f'structure {name}: {s.n} nodes, {s.gs.n_edges} edges, in-degree <= {s.gs.max_in_degree}, '
              + (f'{s.tiles[0].n_tiles} tiles of {s.tiles[0].tile_nodes} nodes' if s.tiles is not None else 'does not tile'))
    for name in ('A', 'A105', 'F'):
        s = structure(mp, name)
        assert s.gs.n_edges >= CUT * s.tiles[0].n_tiles, (name, s.gs.n_edges, s.tiles[0].n_tiles)
    b = structure(mp, 'B')
    assert b.gs.n_edges < CUT * b.tiles[0].n_tiles, (b.gs.n_edges, b.tiles[0].n_tiles)
    for name in ('A', 'A105', 'B'):
        assert structure(mp, name).gs.period() is None
    f0, f1 = structure(mp, 'F', 0), structure(mp, 'F', 1)
    assert f0.gs.period() is not None and f0.tiles[0].period_tiles == 0 and f1.tiles[0].period_tiles > 0
    assert 33 % f0.tiles[0].tile_nodes != 0 and f1.gs.n_edges >= CUT * f1.tiles[0].n_tiles
    c = structure(mp, 'C')          # distinct sources in C, repeated ones in C128 and D
    hub = int(np.argmax(np.bincount(c.ei[1])))
    assert len(set(c.ei[0][c.ei[1] == hub].tolist())) == 200
    for name in ('C128', 'D'):
        s = structure(mp, name)
        hub = int(np.argmax(np.bincount(s.ei[1])))
        assert len(set(s.ei[0][s.ei[1] == hub].tolist())) == 127


def check_cell(mp, form, row):
    L = mp.lib()
    want = row.gated if form == 'gated' else row.plain
    assert want is not None, 'the parametrisation leaves out the cells a row does not run'
    s = structure(mp, row.name, row.align)
    ref = reference(mp, form, s)
    tol = bar_of(s.sizes)
    with tuned(L, **row.switches):
        out, counts, status = run_layer(mp, form, s)
        again, counts2, _ = run_layer(mp, form, s)
    err = float(np.abs(out.double().cpu().numpy() - ref).max())
    print(f'route {form}/{row.id}: launches {counts}, max|hip - oracle| = {err:.3e} (bar {tol:.0e})')
    record_parity('layer_routes', f'{form}/{row.id}', max_abs=err, bar=tol, launches='/'.join(str(c) for c in counts))
    assert counts == want and counts2 == want, (row.id, row.why, counts, want)
    assert torch.isfinite(out).all()
    assert err < tol, (row.id, err)
    assert status == 0, f'range status {status}'
    assert torch.equal(out, again), 'a repeated launch is bit-identical'
    for other in tuple(row.same) + (tuple(row.same_gated) if form == 'gated' else ()):
        with tuned(L, **other):
            o2, _, _ = run_layer(mp, form, s)
        assert torch.equal(out, o2), (row.id, other)
    for k in row.switches:       # the context put every switch back
        if k != 'DENSE_MESSAGE':
            assert L.msmp_tune_query(k.encode()) == {'split': 1, 'edge_nb': 0, 'pair': 1, 'tile': 2, 'tile_arith': 1, 'tail': 1}[k]


@pytest.mark.parametrize('row', [r for r in ROWS if r.gated is not None], ids=lambda r: r.id)
def test_gated_pair_routes(mp, row):
    """A pair of GNN_LayerLin (gate, main) through mp_layer: launch counts, float64 oracle, finiteness, range status, bit-identities."""
    check_cell(mp, 'gated', row)


@pytest.mark.parametrize('row', [r for r in ROWS if r.plain is not None], ids=lambda r: r.id)
def test_lin_layer_routes(mp, row):
    """GNN_LayerLin alone through mp_layer."""
    check_cell(mp, 'lin', row)


@pytest.mark.parametrize('row', [r for r in ROWS if r.plain is not None], ids=lambda r: r.id)
def test_residual_layer_routes(mp, row):
    """GNN_Layer (residual, Swish on the last linear) through mp_layer."""
    check_cell(mp, 'residual', row)


def test_tuned_restores_after_a_failure(mp):
    L = mp.lib()
    from msmp_pde_amd import layers
    with pytest.raises(ZeroDivisionError):
        with tuned(L, tile=0, pair=2, DENSE_MESSAGE=True):
            assert L.msmp_tune_query(b'tile') == 0 and L.msmp_tune_query(b'pair') == 2 and layers.DENSE_MESSAGE is True
            1 / 0
    assert L.msmp_tune_query(b'tile') == 2 and L.msmp_tune_query(b'pair') == 1 and layers.DENSE_MESSAGE is False


# ---------------------------------------------------------------------------------------------------------------------------
# PAIR_MAX_NODES: "pair" 1 pairs the heads up to 65536 nodes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('graphs', [1024, 1025])
def test_pair_switches_at_65536_nodes(mp, graphs):
    """One periodic batch of banded 64-node graphs at 65536 nodes and at 65600, the first size above: "pair" 1 makes one message
    launch for both heads up to 65536 nodes and one per head above, on the tiled and on the gather route; "pair" 2 and 0 are bitwise
    equal to it at both sizes.  The oracle runs on the first and the last graph alone (graphs are independent)."""
    from msmp_pde_amd.graph import GraphStructure
    L = mp.lib()
    m = 64
    ei, batch = banded_batch((m,) * graphs, 3)
    s = _Structure()
    s.n = n = m * graphs
    s.gs = GraphStructure(torch.tensor(ei).cuda(), torch.tensor(batch).cuda(), n)
    s.args = inputs(n, seed=graphs)
    assert s.gs.period() is not None and s.gs.max_graph_nodes == m and (n <= 65536) == (graphs == 1024)
    tiles = s.gs.tiles()
    assert tiles is not None and s.gs.n_edges >= CUT * tiles[0].n_tiles
    main, gate = layers_of(mp, 'gated')
    ei1, batch1 = banded_batch((m,), 3)
    paired = graphs == 1024
    for tile, one, two in ((2, (1, 0, 0, 1, 0), (2, 0, 0, 1, 0)), (0, (1, 1, 0, 1, 0), (2, 2, 0, 1, 0))):
        outs = {}
        for pair in (1, 2, 0):
            with tuned(L, tile=tile, pair=pair):
                outs[pair], counts, status = run_layer(mp, 'gated', s)
            assert counts == (one if pair == 2 or (pair == 1 and paired) else two), (tile, pair, counts)
            assert status == 0
        assert torch.equal(outs[1], outs[2]) and torch.equal(outs[1], outs[0]), tile
        assert torch.isfinite(outs[1]).all()
        for lo in (0, n - m):
            ref = oracle_layer(main, gate, [t[lo:lo + m] for t in s.args], ei1, batch1)
            err = float(np.abs(outs[1][lo:lo + m].double().cpu().numpy() - ref).max())
            print(f'pair switch, {graphs} graphs, tile {tile}, nodes {lo}..{lo + m - 1}: max|hip - oracle| = {err:.3e} (bar {BAR:.0e})')
            record_parity('layer_routes', f'pair_max_nodes/{graphs}/tile{tile}/node{lo}', max_abs=err, bar=BAR)
            assert err < BAR, (tile, lo, err)


# ---------------------------------------------------------------------------------------------------------------------------
# The norm kernels at their switch points: generic / register-resident <13> up to 104 nodes / <16> up to 128
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('largest', [103, 104, 105, 112, 127, 128, 129])
def test_norm_kernels_at_their_switch_points(mp, largest):
    """msmp_instance_norm_f32 and msmp_gate_blend_f32 with the true largest graph as the hint (register-resident editions: 13 rows per
    thread up to 104 nodes, 16 up to 128, the generic kernel above) and with hint 0 (generic), on a batch that also holds a 1-node, an
    8-node and a 9-node graph (row slices without a row; node counts 0 and 1 modulo the 8 row slices).  Against the oracle at 5e-6 and
    between the editions at 2e-6, the bars of test_layer_pieces_vs_oracle; the inputs are given in fp32, so the small graphs have no
    rounding of pre-norm values to amplify and take the same bar.  Outputs start as NaN: a row that a kernel leaves out fails."""
    from msmp_pde_amd._lib import check, ptr, current_stream
    from msmp_pde_amd.graph import GraphStructure
    L = mp.lib()
    sizes = (8, largest, 1, 9)
    n = sum(sizes)
    batch = np.repeat(np.arange(len(sizes)), sizes)
    gs = GraphStructure(torch.zeros((2, 0), dtype=torch.int64).cuda(), torch.tensor(batch).cuda(), n)
    assert gs.max_graph_nodes == largest and gs.n_graphs == len(sizes)
    assert np.array_equal(gs.graph_ptr.cpu().numpy(), np.concatenate([[0], np.cumsum(sizes)]))
    rng = np.random.default_rng(largest)
    f = lambda a: torch.tensor(a, dtype=torch.float32).cuda()
    x = f(rng.standard_normal((n, H)) * 0.3 + 1.0)
    h, g_pre, m_pre = (f(rng.standard_normal((n, H))) for _ in range(3))
    st = current_stream()
    nan = lambda: torch.full((n, H), float('nan'), device='cuda')
    y0, y1, b0, b1 = nan(), nan(), nan(), nan()
    with launch_counts(L) as counts:
        check(L.msmp_instance_norm_f32(ptr(x), ptr(gs.graph_ptr), len(sizes), 0, 1e-5, ptr(y0), st), 'norm generic')
        check(L.msmp_instance_norm_f32(ptr(x), ptr(gs.graph_ptr), len(sizes), gs.max_graph_nodes, 1e-5, ptr(y1), st), 'norm hinted')
        check(L.msmp_gate_blend_f32(ptr(h), ptr(g_pre), ptr(m_pre), ptr(gs.graph_ptr), len(sizes), 0, 1e-5, ptr(b0), st), 'blend generic')
        check(L.msmp_gate_blend_f32(ptr(h), ptr(g_pre), ptr(m_pre), ptr(gs.graph_ptr), len(sizes), gs.max_graph_nodes, 1e-5, ptr(b1), st),
              'blend hinted')
    torch.cuda.synchronize()
    assert counts['NORM'] == 4 and sum(counts.values()) == 4
    ref_y = O.instance_norm(x.double().cpu().numpy(), batch)
    tau = O.sigmoid(O.instance_norm(g_pre.double().cpu().numpy(), batch))
    ref_b = (1 - tau) * h.double().cpu().numpy() + tau * O.swish(O.instance_norm(m_pre.double().cpu().numpy(), batch))
    for what, generic, hinted, ref in (('instance_norm', y0, y1, ref_y), ('gate_blend', b0, b1, ref_b)):
        assert torch.isfinite(generic).all() and torch.isfinite(hinted).all(), what
        e0 = float(np.abs(generic.double().cpu().numpy() - ref).max())
        e1 = float(np.abs(hinted.double().cpu().numpy() - ref).max())
        between = (hinted - generic).abs().max().item()
        print(f'{what}, largest graph {largest}: generic {e0:.2e}, hinted {e1:.2e} vs oracle (bar 5e-6); between the editions {between:.2e} (bar 2e-6)')
        record_parity('norm_switch_points', f'{what}/{largest}', generic=e0, hinted=e1, between=between, bar=5e-6, bar_between=2e-6)
        assert e0 < 5e-6 and e1 < 5e-6, (what, e0, e1)
        assert between < 2e-6, (what, between)
        if largest > 128:
            assert torch.equal(hinted, generic), 'above 128 nodes the hint selects the generic kernel too'
    assert mp.last_status(reset=True) == 0


# ---------------------------------------------------------------------------------------------------------------------------
# The timing counters themselves
# ---------------------------------------------------------------------------------------------------------------------------
def test_timing_counters(mp):
    """msmp_timing_enable / _reset / _read: nothing is counted at mask 0, one enabled family counts alone, reset zeroes, the summed
    time is finite and not negative, a family index outside 0..6 is MSMP_ERR_ARG, and the layer output does not depend on timing."""
    import ctypes
    import math
    from msmp_pde_amd import _lib
    L = mp.lib()
    s = structure(mp, 'A')
    main, gate = layers_of(mp, 'gated')
    call = lambda: mp.mp_layer(*s.args, s.gs, main, gate)
    read_all = lambda: [_lib.timing_read(k) for k in range(7)]
    try:
        with torch.no_grad(), tuned(L, tile=0):           # projection + message + tail: three families, one launch each
            assert L.msmp_timing_enable(0) == 0 and L.msmp_timing_reset() == 0
            off = call()
            assert all(c == 0 and ms == 0.0 for c, ms in read_all())
            assert L.msmp_timing_enable(1 << _lib.K_NODE_PROJ) == 0
            one = call()
            got = read_all()
            assert [c for c, _ in got] == [1 if k == _lib.K_NODE_PROJ else 0 for k in range(7)]
            assert L.msmp_timing_enable(0b1111111) == 0
            call()
            got = read_all()
            assert [c for c, _ in got] == [1, 0, 1, 0, 0, 2, 0]       # counts add up until the reset
            assert all(math.isfinite(ms) and ms >= 0.0 for _, ms in got)
            assert L.msmp_timing_enable(0b1111111 | 1 << 7 | 1 << 20) == 0      # bits above the families are dropped
            every = call()
            assert [c for c, _ in read_all()] == [2, 0, 2, 0, 0, 3, 0]
            assert L.msmp_timing_reset() == 0
            assert all(c == 0 and ms == 0.0 for c, ms in read_all())
            assert torch.equal(off, one) and torch.equal(off, every)
        n_, ms_ = ctypes.c_int64(5), ctypes.c_double(5.0)
        for bad in (-1, 7, 1 << 20):
            assert L.msmp_timing_read(bad, ctypes.byref(n_), ctypes.byref(ms_)) == -1      # MSMP_ERR_ARG
            assert b'msmp_timing_read' in L.msmp_last_error() and n_.value == 5
        assert L.msmp_timing_read(0, None, ctypes.byref(ms_)) == -1 and L.msmp_timing_read(0, ctypes.byref(n_), None) == -1
    finally:
        L.msmp_timing_enable(0)
        L.msmp_timing_reset()
    with launch_counts(L) as counts:
        pass
    assert counts == dict.fromkeys(('EDGE_MLP', 'SCATTER_MEAN', 'NODE_UPDATE', 'NORM', 'LEM', 'NODE_PROJ', 'DECODER'), 0)
