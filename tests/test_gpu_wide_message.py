"""GPU tests of the fused width-generic message kernel (msmp_wide_message_f32, wide_message_kernel.hip): the aggregate
mean_j Swish(W2 Swish(P[i] + Q[j]) + b2) of GNN_LayerLin (experiments/models_gnn.py:132-138, :107) in one launch at any hidden width up to
256, against the formula in numpy float64 from the same fp32 inputs; its bitwise properties (run to run, independent of the batch around a
graph and of the tile cut), the padding columns, the in-degree cap and the fall-back above it, the range status, and the host paths that
reach it: wide._mp_layer_wide and the two GLU solver classes.
Bar 1e-6 max(1, max|ref|): the bar of test_layer_pieces_vs_oracle for the 128-wide message and aggregate kernels (same arithmetic)."""
import numpy as np
import pytest
import torch

from oracle import msmp_oracle as O
from helpers import synthetic_case, ld_of, ragged_edges, layer_inputs, oracle_layer, counted
from helpers import mp, restore_wide_switches       # noqa: F401  (fixtures)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('restore_wide_switches')]

WIDTHS = [33, 96, 130, 164, 192, 256]          # KT 2, 3, 5, 6, 6, 8
SIZES = [1, 37, 100, 130, 5]


def csr_of(ei, n):
    """(rowptr, col) by target; ei's targets are sorted"""
    deg = np.bincount(ei[1], minlength=n)
    return np.concatenate(([0], np.cumsum(deg))).astype(np.int32), ei[0].astype(np.int32)


def reference(P, Q, w2, b2, rowptr, col, W):
    """the formula in float64 from the fp32 inputs: [n, W]"""
    n = len(rowptr) - 1
    deg = np.diff(rowptr)
    tgt = np.repeat(np.arange(n), deg)
    P, Q = P.double().cpu().numpy()[:, :W], Q.double().cpu().numpy()[:, :W]
    msg = O.swish(O.swish(P[tgt] + Q[col]) @ w2.T + b2)
    agg = np.zeros((n, W))
    np.add.at(agg, tgt, msg)
    return agg / np.maximum(deg, 1)[:, None]


class Case(object):
    """message_net_2 of a GNN_LayerLin at width W (the reference's initialisation), its packed blob, random P / Q with row stride ld"""

    def __init__(self, mp, W, n, ld, seed=0, scale=1.0):
        from msmp_pde_amd._lib import ptr, current_stream
        torch.manual_seed(100 * W + seed)
        lin = mp.GNN_LayerLin(W, W, W, 25, 2).message_net_2[0].cuda()
        self.W, self.ld, self.n = W, ld, n
        self.w2, self.b2 = lin.weight.detach().contiguous(), lin.bias.detach().contiguous()
        self.w2_64, self.b2_64 = self.w2.double().cpu().numpy(), self.b2.double().cpu().numpy()
        L = mp.lib()
        nf = L.msmp_packed_wide_msg_floats(W)
        assert nf > 0
        self.blob = torch.empty(nf, dtype=torch.float32, device='cuda')
        assert L.msmp_pack_wide_msg_f32(ptr(self.w2), ptr(self.b2), W, ptr(self.blob), current_stream()) == 0
        self.P = torch.randn(n, ld, device='cuda') * scale
        self.Q = torch.randn(n, ld, device='cuda')


def run(mp, case, rowptr, col, max_deg, n=None, out=None, ld=None):
    from msmp_pde_amd._lib import ptr, current_stream
    n = case.n if n is None else n
    ld = case.ld if ld is None else ld
    rp = torch.tensor(rowptr, dtype=torch.int32, device='cuda')
    cl = torch.tensor(col if len(col) else [0], dtype=torch.int32, device='cuda')
    if out is None:
        out = torch.empty(n, ld, dtype=torch.float32, device='cuda')
    rc = mp.lib().msmp_wide_message_f32(ptr(case.P), ptr(case.Q), ptr(rp), ptr(cl), n, len(col), max_deg, case.W, ld, ptr(case.blob),
                                        out.data_ptr(), current_stream())
    torch.cuda.synchronize()
    return rc, out


def check(out, ref, W, what):
    got = out.double().cpu().numpy()
    e, bar = float(np.abs(got[:, :W] - ref).max()), 1e-6 * max(1.0, float(np.abs(ref).max()))
    print(f'{what}: max abs err {e:.2e} (bar {bar:.2e}, max |ref| {np.abs(ref).max():.2e})')
    assert e < bar, (what, e, bar)
    assert (got[:, W:] == 0).all(), what


@pytest.mark.parametrize('W,extra', [(w, 0) for w in WIDTHS] + [(164, 8)])
def test_parity_on_the_ragged_batch(mp, W, extra):
    ei, _, n = ragged_edges()
    rowptr, col = csr_of(ei, n)
    ld = ld_of(W) + extra
    case = Case(mp, W, n, ld)
    rc, out = run(mp, case, rowptr, col, int(np.diff(rowptr).max()))
    assert rc == 0
    ref = reference(case.P, case.Q, case.w2_64, case.b2_64, rowptr, col, W)
    check(out, ref, W, f'W={W} ld={ld}')
    assert (out[np.diff(rowptr) == 0] == 0).all()           # zero in-degree: an exact 0


def hub_graph(n, hub_degree, seed=1):
    """node 0 takes `hub_degree` in-edges (sources 1 .. hub_degree), every other node two"""
    rng = np.random.default_rng(seed)
    src = list(range(1, hub_degree + 1))
    dst = [0] * hub_degree
    for t in range(1, n):
        for s_ in rng.choice(n, size=2, replace=False):
            src.append(int(s_)); dst.append(t)
    return np.stack([np.array(src), np.array(dst)])


def test_hub_at_the_degree_cap_runs_fused(mp):
    W = 164
    cap = mp.lib().msmp_wide_message_max_in_degree(W)
    assert cap >= 32
    n = cap + 40
    ei = hub_graph(n, cap)
    rowptr, col = csr_of(ei, n)
    case = Case(mp, W, n, 256, seed=1)
    rc, out = run(mp, case, rowptr, col, cap)
    assert rc == 0
    check(out, reference(case.P, case.Q, case.w2_64, case.b2_64, rowptr, col, W), W, f'hub of in-degree {cap}')


def test_hub_above_the_cap_is_refused_and_the_layer_takes_the_three_launches(mp):
    from msmp_pde_amd.wide import _mp_layer_wide
    from msmp_pde_amd.graph import GraphStructure
    from msmp_pde_amd import _lib
    W, tw, nv = 164, 25, 2
    cap = mp.lib().msmp_wide_message_max_in_degree(W)
    n = cap + 40
    ei = hub_graph(n, cap + 1)
    rowptr, col = csr_of(ei, n)
    case = Case(mp, W, n, 256, seed=2)
    out = torch.full((n, 256), 7.5, device='cuda')
    rc, out = run(mp, case, rowptr, col, cap + 1, out=out)
    assert rc == _lib.MSMP_ERR_UNSUPPORTED == -2 and mp.lib().msmp_last_error()
    assert (out == 7.5).all()                                 # nothing was launched
    batch = np.zeros(n, dtype=np.int64)
    gs = GraphStructure(torch.tensor(ei).cuda(), torch.tensor(batch).cuda(), n)
    assert gs.max_in_degree == cap + 1
    torch.manual_seed(9)
    main = mp.GNN_LayerLin(W, W, W, tw, nv).cuda()
    h, u, pos, var = layer_inputs(n, W, tw, nv, 4)
    with torch.no_grad():
        got = _mp_layer_wide(h, u, pos.reshape(-1), var, gs, main, None, 1e-5)
    e = np.abs(got.double().cpu().numpy() - oracle_layer(main, None, (h, u, pos, var), ei, batch)).max()
    print(f'layer with a hub of in-degree {cap + 1}: {e:.2e}')
    assert e < 2e-5


def test_no_edges_gives_zeros(mp):
    W, n = 164, 50
    case = Case(mp, W, n, 256, seed=3)
    out = torch.full((n, 256), 3.0, device='cuda')
    rc, out = run(mp, case, np.zeros(n + 1, dtype=np.int32), np.zeros(0, dtype=np.int32), 0, out=out)
    assert rc == 0 and (out == 0).all()
    rc, _ = run(mp, case, np.zeros(1, dtype=np.int32), np.zeros(0, dtype=np.int32), 0, n=0, out=out)
    assert rc == 0                                            # no nodes: a valid call, nothing to do


def test_more_tiles_than_resident_workgroups(mp):
    """6 000 targets of in-degree 6: 600 tiles of ten targets, more than a persistent launch has workgroups at width 164 (one per CU),
    so every workgroup loops, and the last tile is partial in no workgroup's first round"""
    W, n, deg = 164, 6000, 6
    rng = np.random.default_rng(5)
    col = np.concatenate([(t + rng.choice(np.arange(1, 40), size=deg, replace=False)) % n for t in range(n)]).astype(np.int32)
    rowptr = (np.arange(n + 1) * deg).astype(np.int32)
    case = Case(mp, W, n, 256, seed=4)
    rc, out = run(mp, case, rowptr, col, deg)
    assert rc == 0
    check(out, reference(case.P, case.Q, case.w2_64, case.b2_64, rowptr, col, W), W, '6000 nodes of degree 6')


@pytest.mark.parametrize('W', [33, 164, 256])
def test_runs_repeat_and_graphs_do_not_depend_on_the_batch(mp, W):
    ei, _, n = ragged_edges()
    rowptr, col = csr_of(ei, n)
    ld = ld_of(W)
    case = Case(mp, W, n, ld, seed=5)
    d = int(np.diff(rowptr).max())
    rc1, a = run(mp, case, rowptr, col, d)
    rc2, b = run(mp, case, rowptr, col, d)
    assert rc1 == 0 and rc2 == 0 and torch.equal(a, b)
    n2 = SIZES[0] + SIZES[1]                                  # the first two graphs alone, and cut into other tiles (another degree bound)
    for bound in (d, d + 3):
        rc, sub = run(mp, case, rowptr[:n2 + 1], col[:rowptr[n2]], bound, n=n2)
        assert rc == 0 and torch.equal(sub, a[:n2]), bound


def test_padding_columns_are_zero_and_nothing_else_is_written(mp):
    W = 164
    ei, _, n = ragged_edges()
    rowptr, col = csr_of(ei, n)
    ld = 256 + 8
    case = Case(mp, W, n, ld, seed=6)
    poison, pad = 777.25, 4096
    buf = torch.full((pad + n * ld + pad,), poison, device='cuda')
    out = buf[pad:pad + n * ld].view(n, ld)
    rc, _ = run(mp, case, rowptr, col, int(np.diff(rowptr).max()), out=out)
    assert rc == 0
    assert (buf[:pad] == poison).all() and (buf[pad + n * ld:] == poison).all()
    assert (out[:, W:] == 0).all() and not (out[:, :W] == poison).any()
    check(out, reference(case.P, case.Q, case.w2_64, case.b2_64, rowptr, col, W), W, 'poisoned buffer')
    rc, plain = run(mp, case, rowptr, col, int(np.diff(rowptr).max()))       # (a guard-banded allocation: conftest checks its margins)
    assert rc == 0 and torch.equal(plain, out)


def test_out_of_range_activation_raises_the_status(mp):
    W = 164
    ei, _, n = ragged_edges()
    rowptr, col = csr_of(ei, n)
    case = Case(mp, W, n, 256, seed=7)
    rc, _ = run(mp, case, rowptr, col, int(np.diff(rowptr).max()))
    assert rc == 0 and mp.last_status() == 0
    case.P *= 5000.0
    rc, _ = run(mp, case, rowptr, col, int(np.diff(rowptr).max()))
    assert rc == 0
    assert mp.last_status(reset=True) & mp.MSMP_STATUS_NODE_SATURATED
    assert mp.last_status() == 0


@pytest.mark.parametrize('gated', [False, True])
def test_layer_on_either_message_path(mp, gated, monkeypatch):
    from msmp_pde_amd.wide import _mp_layer_wide
    from msmp_pde_amd.graph import GraphStructure
    from msmp_pde_amd import _lib
    W, tw, nv = 164, 25, 2
    ei, batch, n = ragged_edges()
    gs = GraphStructure(torch.tensor(ei).cuda(), torch.tensor(batch).cuda(), n)
    torch.manual_seed(5)
    main = mp.GNN_LayerLin(W, W, W, tw, nv).cuda()
    gate = mp.GNN_LayerLin(W, W, W, tw, nv).cuda() if gated else None
    h, u, pos, var = layer_inputs(n, W, tw, nv, 3)
    ref = oracle_layer(main, gate, (h, u, pos, var), ei, batch)
    L = mp.lib()
    calls = counted(mp, monkeypatch, 'msmp_wide_message_f32')
    layer = lambda: _mp_layer_wide(h, u, pos.reshape(-1), var, gs, main, gate, 1e-5)
    with torch.no_grad():
        out1 = layer()
        assert len(calls) == (2 if gated else 1)              # one fused launch per head
        e = np.abs(out1.double().cpu().numpy() - ref).max()
        print(f'wide layer ({"gated" if gated else "plain"}) with wide_msg 1: {e:.2e}')
        assert e < 2e-5
        del calls[:]
        L.msmp_tune(b'wide_msg', 0)
        out0 = layer()                                        # gather + row GEMM + scatter: the path before this kernel
        L.msmp_tune(b'wide_msg', 1)
        with _lib.exact_fp32():
            out_exact = layer()
        L.msmp_tune(b'lem_wide', 0)                           # the unfused width-generic path as a whole
        out_lem0 = layer()
        L.msmp_tune(b'lem_wide', 1)
        assert not calls                                      # none of the three reaches the fused entry
        assert torch.equal(out_lem0, out0)
    assert np.abs(out0.double().cpu().numpy() - ref).max() < 2e-5
    assert torch.equal(out_exact, out0)


@pytest.mark.parametrize('kind,exp', [('MP_PDE_SolverLEMLinGatedGLU', 'E2'), ('MP_PDE_Solver2DLEMLinGatedGLU', 'MSWG3')])
def test_glu_solver_forward_on_either_message_path(mp, kind, exp):
    torch.manual_seed(7)
    case = synthetic_case(mp, exp, bsz=2, seed=3)
    model = getattr(mp, kind)(case.pde, time_window=25, eq_variables=case.eqv, hidden_layer=2).cuda().eval()
    graph = case.graph.to('cuda')
    L = mp.lib()
    with torch.no_grad():
        out1 = model(graph)
        L.msmp_tune(b'wide_msg', 0)
        try:
            out0 = model(graph)
        finally:
            L.msmp_tune(b'wide_msg', 1)
    d = (out1 - out0).abs().max().item()
    print(f'{kind}/{exp}: wide_msg 1 vs 0 max abs {d:.2e} (output max {out0.abs().max().item():.2e})')
    assert torch.isfinite(out1).all() and d < 1e-5
