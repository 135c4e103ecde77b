"""GPU tests of the fused width-generic projection kernel (msmp_wide_node_proj_f32, wide_node_proj_kernel.hip): the per-node projections P, Q of
the factorised message_net_1 of GNN_LayerLin (experiments/models_gnn.py:132-138) for both heads of a gated pair in one launch at any hidden
width up to 256, against the two formulas in numpy float64 from the same fp32 inputs; its bitwise properties (run to run, independent of the
nodes around a node and of where the node falls into the tiles), the bounds of its writes, the range status, the refusals by value, and the
host paths that reach it: wide._mp_layer_wide and the two GLU solver classes.
Bar: 1e-6 max(1, K / 156) on max|got - ref| / max(1, max|ref|) with K = W + tw + 1 + nv (1e-6 is the bar test_layer_pieces_vs_oracle holds
this fp16-split arithmetic to at the 128-wide projection's K of about 156; the rounding sum grows at most linearly in K)."""
import numpy as np
import pytest
import torch

from helpers import synthetic_case, ld_of, ragged_edges, layer_inputs, oracle_layer, counted
from helpers import mp, restore_wide_switches       # noqa: F401  (fixtures)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('restore_wide_switches')]

WIDTHS = [33, 96, 128, 130, 164, 192, 256]          # KT 2, 3, 4, 5, 6, 6, 8
TAILS = [(25, 1), (25, 3), (50, 5), (100, 8)]       # 27, 29, 56, 109 feature columns: 2, 2, 4, 7 K = 16 steps (the cap is 128 columns)
NODES = [1, 31, 64, 65, 200]                        # ragged last column block, ragged last tile
N_MAX = 240
EPS = 1e-5


class Case(object):
    """message_net_1 of two GNN_LayerLin heads at width W (the reference's initialisation) and their packed blobs; h standard normal with row
    stride ld, u standard normal, pos and vars uniform in [0, 1), and their packed feature rows"""

    def __init__(self, mp, W, tw, nv, n, ld, seed=0):
        from msmp_pde_amd._lib import ptr, current_stream
        torch.manual_seed(1000 * W + 10 * tw + nv + seed)
        self.mp, self.W, self.tw, self.nv, self.n, self.ld = mp, W, tw, nv, n, ld
        L = mp.lib()
        self.w1, self.b1, self.blobs = [], [], []
        for _ in range(2):
            layer = mp.GNN_LayerLin(W, W, W, tw, nv).cuda()
            sd = layer.state_dict()
            w1, b1 = sd['message_net_1.0.weight'].detach().contiguous(), sd['message_net_1.0.bias'].detach().contiguous()
            assert w1.shape == (W, 2 * W + tw + 1 + nv)
            nf = L.msmp_packed_wide_proj_floats(W, tw, nv)
            assert nf > 0
            blob = torch.empty(nf, dtype=torch.float32, device='cuda')
            assert L.msmp_pack_wide_proj_f32(ptr(w1), ptr(b1), W, tw, nv, ptr(blob), current_stream()) == 0
            self.w1.append(w1); self.b1.append(b1); self.blobs.append(blob)
        torch.cuda.synchronize()
        self.h = torch.randn(n, ld, device='cuda')
        self.u = torch.randn(n, tw, device='cuda')
        self.pos = torch.rand(n, device='cuda')
        self.var = torch.rand(n, nv, device='cuda')
        self.pack_features()
        self._ref = None

    def pack_features(self):
        from msmp_pde_amd.layers import node_features
        self.feat = node_features(self.u, self.pos, self.var)
        assert self.feat.shape[1] == self.mp.lib().msmp_node_feature_stride(self.tw, self.nv)
        torch.cuda.synchronize()

    def reference(self):
        """float64 from the fp32 inputs, computed once: [(P, Q) main, (P, Q) gate], each [n, W]"""
        if self._ref is None:
            W, tw = self.W, self.tw
            h = self.h.double().cpu().numpy()[:, :W]
            f = np.concatenate([self.u.double().cpu().numpy(), self.pos.double().cpu().numpy()[:, None], self.var.double().cpu().numpy()], 1)
            self._ref = []
            for w1, b1 in zip(self.w1, self.b1):
                w, b = w1.double().cpu().numpy(), b1.double().cpu().numpy()
                ref_P = h @ w[:, :W].T + f @ w[:, 2 * W:].T + b
                ref_Q = h @ w[:, W:2 * W].T - f[:, :tw + 1] @ w[:, 2 * W:2 * W + tw + 1].T
                self._ref.append((ref_P, ref_Q))
        return self._ref

    def bar(self):
        return 1e-6 * max(1.0, (self.W + self.tw + 1 + self.nv) / 156.0)


def run(mp, case, n=None, gated=True, first=0, outs=None):
    """the call on nodes first .. first + n - 1 (pointer offsets); returns rc and [p_main, q_main, p_gate, q_gate] ([n, ld], NaN-filled before)"""
    from msmp_pde_amd._lib import ptr, current_stream
    n = case.n - first if n is None else n
    if outs is None:
        outs = [torch.full((max(n, 1), case.ld), float('nan'), device='cuda') for _ in range(4 if gated else 2)]
    o = [t.data_ptr() for t in outs] + [None, None]
    rc = mp.lib().msmp_wide_node_proj_f32(case.h[first:].data_ptr(), case.feat[first:].data_ptr(), n, case.tw, case.nv, case.W, case.ld,
                                          ptr(case.blobs[0]), ptr(case.blobs[1]) if gated else None, o[0], o[1], o[2], o[3], current_stream())
    torch.cuda.synchronize()
    return rc, outs


def check(case, outs, n, what, first=0):
    W = case.W
    refs = [m[first:first + n] for pq in case.reference() for m in pq]
    for name, out, ref in zip(('P main', 'Q main', 'P gate', 'Q gate'), outs, refs):
        got = out.double().cpu().numpy()[:n]
        e, bar = float(np.abs(got[:, :W] - ref).max() / max(1.0, np.abs(ref).max())), case.bar()
        print(f'{what} {name}: max err {e:.2e} (bar {bar:.2e})')
        assert e < bar, (what, name, e, bar)
        assert (got[:, W:] == 0).all(), (what, name)


@pytest.mark.parametrize('tw,nv', TAILS)
@pytest.mark.parametrize('W,extra', [(w, 0) for w in WIDTHS] + [(164, 8)])
def test_parity(mp, W, extra, tw, nv):
    case = Case(mp, W, tw, nv, max(NODES), ld_of(W) + extra)
    mp.last_status(reset=True)
    for n in NODES:
        for gated in (True, False):
            rc, outs = run(mp, case, n, gated)
            assert rc == 0
            check(case, outs, n, f'W={W} ld={case.ld} tw={tw} nv={nv} n={n} {"pair" if gated else "one head"}')
    assert mp.last_status() == 0


def test_more_tiles_than_resident_workgroups(mp):
    """600 tiles of 64 nodes at width 164: more than a persistent launch has workgroups (one per CU), so every workgroup loops"""
    case = Case(mp, 164, 25, 2, 600 * 64, 256, seed=1)
    for gated in (True, False):
        rc, outs = run(mp, case, gated=gated)
        assert rc == 0
        check(case, outs, case.n, '600 tiles')


@pytest.mark.parametrize('W', [33, 164, 256])
def test_runs_repeat_and_nodes_do_not_depend_on_their_tile_or_batch(mp, W):
    case = Case(mp, W, 25, 2, N_MAX, ld_of(W), seed=2)
    rc1, a = run(mp, case)
    rc2, b = run(mp, case)
    assert rc1 == 0 and rc2 == 0 and all(torch.equal(x, y) for x, y in zip(a, b))
    rc, sub = run(mp, case, n=100)                              # fewer nodes: another grid, a ragged last tile elsewhere
    assert rc == 0 and all(torch.equal(x, y[:100]) for x, y in zip(sub, a))
    rc, off = run(mp, case, first=37)                           # started at node 37: every node in another tile, column block and lane
    assert rc == 0 and all(torch.equal(x, y[37:]) for x, y in zip(off, a))
    rc, one = run(mp, case, gated=False)
    assert rc == 0 and torch.equal(one[0], a[0]) and torch.equal(one[1], a[1])


@pytest.mark.parametrize('n', [65, 200])
def test_nothing_outside_the_rows_is_written_and_padding_columns_are_zero(mp, n):
    W, ld = 164, 256 + 8
    case = Case(mp, W, 25, 2, n, ld, seed=3)
    guard = 70                                                  # more rows than a tile behind row n
    for gated in (True, False):
        bufs = [torch.full((guard + n + guard, ld), float('nan'), device='cuda') for _ in range(4 if gated else 2)]
        rc, _ = run(mp, case, n, gated, outs=[b[guard:] for b in bufs])
        assert rc == 0
        for b in bufs:
            assert torch.isnan(b[:guard]).all() and torch.isnan(b[guard + n:]).all()
            assert (b[guard:guard + n, W:] == 0).all() and torch.isfinite(b[guard:guard + n]).all()
        check(case, [b[guard:guard + n] for b in bufs], n, 'guarded buffers')


@pytest.mark.parametrize('where', ['h', 'u'])
def test_out_of_range_element_raises_the_status(mp, where):
    case = Case(mp, 164, 25, 2, 200, 256, seed=5)
    mp.last_status(reset=True)
    rc, _ = run(mp, case)
    assert rc == 0 and mp.last_status() == 0
    if where == 'h':
        case.h[131, 77] = 300.0
    else:
        case.u[131, 7] = 300.0
        case.pack_features()
        mp.last_status(reset=True)                              # (the feature packer reports its own bit)
    rc, _ = run(mp, case)
    assert rc == 0
    assert mp.last_status(reset=True) & mp.MSMP_STATUS_NODE_SATURATED
    assert mp.last_status() == 0


def test_refusals_by_value_launch_nothing(mp):
    from msmp_pde_amd._lib import ptr, current_stream
    L = mp.lib()
    case = Case(mp, 164, 25, 2, 64, 256, seed=6)
    outs = [torch.full((64, 256), 7.5, device='cuda') for _ in range(4)]
    o = [t.data_ptr() for t in outs]
    call = lambda n, tw, nv, W, ld: L.msmp_wide_node_proj_f32(ptr(case.h), ptr(case.feat), n, tw, nv, W, ld, ptr(case.blobs[0]), ptr(case.blobs[1]),
                                                             o[0], o[1], o[2], o[3], current_stream())
    assert call(64, 120, 8, 164, 256) == -2 and b'tail' in L.msmp_last_error()          # 129 feature columns
    assert L.msmp_packed_wide_proj_floats(164, 120, 8) == 0 and L.msmp_packed_wide_proj_floats(164, 119, 8) > 0
    assert call(64, 25, 2, 257, 260) == -2 and b'width' in L.msmp_last_error()
    assert L.msmp_packed_wide_proj_floats(257, 25, 2) == 0
    assert call(0, 25, 2, 164, 256) == 0
    torch.cuda.synchronize()
    assert all((t == 7.5).all() for t in outs)


@pytest.mark.parametrize('wide_tail', [0, 1])
@pytest.mark.parametrize('gated', [False, True])
def test_layer_takes_one_fused_projection_call(mp, gated, wide_tail, monkeypatch):
    from msmp_pde_amd.wide import _mp_layer_wide
    from msmp_pde_amd.graph import GraphStructure
    from msmp_pde_amd import _lib
    W, tw, nv = 164, 25, 2
    ei, batch, n = ragged_edges([1, 37, 100, 128, 5])
    gs = GraphStructure(torch.tensor(ei).cuda(), torch.tensor(batch).cuda(), n)
    torch.manual_seed(5)
    main = mp.GNN_LayerLin(W, W, W, tw, nv).cuda()
    gate = mp.GNN_LayerLin(W, W, W, tw, nv).cuda() if gated else None
    h, u, pos, var = layer_inputs(n, W, tw, nv, 3)
    ref = oracle_layer(main, gate, (h, u, pos, var), ei, batch)
    L = mp.lib()
    proj, lin = counted(mp, monkeypatch, 'msmp_wide_node_proj_f32'), counted(mp, monkeypatch, 'msmp_linear_f32')
    layer = lambda: _mp_layer_wide(h, u, pos.reshape(-1), var, gs, main, gate, EPS)
    with torch.no_grad():
        L.msmp_tune(b'wide_tail', wide_tail)
        L.msmp_tune(b'wide_proj', 1)
        out1 = layer()
        assert len(proj) == 1                                 # one launch for the layer, both heads
        n_lin1 = len(lin)
        e = np.abs(out1.double().cpu().numpy() - ref).max()
        print(f'wide layer ({"gated" if gated else "plain"}, wide_tail {wide_tail}) with wide_proj 1: {e:.2e}')
        assert e < 2e-5
        del proj[:], lin[:]
        L.msmp_tune(b'wide_proj', 0)
        out0 = layer()                                        # concatenation + row GEMMs: the path before this kernel
        assert not proj and len(lin) - n_lin1 == (4 if gated else 2)
        assert np.abs(out0.double().cpu().numpy() - ref).max() < 2e-5
        L.msmp_tune(b'wide_proj', 1)
        with _lib.exact_fp32():
            exact = layer()
        for key in (b'wide_msg', b'lem_wide'):
            L.msmp_tune(key, 0)
            before = layer()
            L.msmp_tune(key, 1)
            assert torch.equal(before, exact)                 # each is the unfused path, bit for bit
        assert not proj                                       # none of the three reaches the fused entry


@pytest.mark.parametrize('kind,exp', [('MP_PDE_SolverLEMLinGatedGLU', 'E2'), ('MP_PDE_Solver2DLEMLinGatedGLU', 'MSWG3')])
def test_glu_solver_forward_on_either_projection_path(mp, kind, exp, monkeypatch):
    torch.manual_seed(7)
    case = synthetic_case(mp, exp, bsz=2, seed=3)
    model = getattr(mp, kind)(case.pde, time_window=25, eq_variables=case.eqv, hidden_layer=2).cuda().eval()
    graph = case.graph.to('cuda')
    L = mp.lib()
    proj, packs = counted(mp, monkeypatch, 'msmp_wide_node_proj_f32'), counted(mp, monkeypatch, 'msmp_pack_node_features_f32')
    with torch.no_grad():
        L.msmp_tune(b'wide_proj', 1)
        out1 = model(graph)
        assert len(proj) == 2                                 # hidden_layer = 2 gated pairs, one launch each
        assert not packs                                      # the feature rows come from the solver's msmp_prepare_nodes, once per forward
        L.msmp_tune(b'wide_proj', 0)
        out0 = model(graph)
        assert len(proj) == 2
        d = (out1 - out0).abs().max().item()
        print(f'{kind}/{exp}: wide_proj 1 vs 0 max abs {d:.2e} (output max {out0.abs().max().item():.2e})')
        assert torch.isfinite(out1).all() and torch.isfinite(out0).all() and d < 1e-5
