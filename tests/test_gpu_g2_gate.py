"""GPU tests of the gradient gate (G2) of MP_PDE_Solver2DLEMLinG2 as one launch (g2_gate_kernel.hip, msmp_pde_amd/g2.py):

  * forward (out, tau) and backward (dh, da, db) against a float64 PyTorch restatement of the formulas (index_add_ mean, as
    oracle/msmp_oracle_torch.py:111-116) on small graphs with every edge case the kernels branch on, at (width, ld) = (128, 128), (164, 256), (4, 4);
  * against the PyTorch-ops route (switch "g2_gate" 0) on an RPU batch; bitwise reproducibility; exact out = h on nodes without out-edges;
  * the class: forward and gradients against the float64 oracle, the number of launches, a captured training step.

Where ld == width the kernels are reached through the host's route (g2.g2_gate_blend and its autograd Function); (164, 256) calls the
entries on rows whose padding columns hold NaN (they are neither read nor written)."""
import numpy as np
import pytest
import torch

from helpers import (TOL, FLOOR_FACTOR, assert_parity, counted, fp32_floors, mp, record_parity, synthetic_case, tuned)     # noqa: F401
from oracle import msmp_oracle as O, msmp_oracle_torch as OT

pytestmark = pytest.mark.gpu
TW = 25
KIND = 'MP_PDE_Solver2DLEMLinG2'
SHAPES = [(128, 128), (164, 256), (4, 4)]


# ---- graphs ------------------------------------------------------------------------------------------------------------------------------
def _edges(name):
    """(edge_index [2, E] int64 numpy: row 0 source, row 1 target; n_nodes)"""
    if name == 'single':            # one node, no edge
        return np.zeros((2, 0), dtype=np.int64), 1
    if name == 'nine':              # node 0: no out-edges; node 8: no in-edges; 3 -> 3 a self-loop; 1 -> 2 twice
        e = [(1, 0), (2, 0), (1, 2), (1, 2), (3, 3), (3, 4), (4, 5), (5, 4), (6, 7), (7, 6), (8, 1), (8, 7), (2, 1), (4, 3), (5, 6), (6, 5), (7, 2)]
        return np.array(e, dtype=np.int64).T.copy(), 9
    if name == 'thirty_seven':      # random directed edges: out-degrees 0 (node 0), 1, 5 and 36 (node 5: every other node)
        rng = np.random.default_rng(5)
        n, e = 37, []
        for s in range(1, n):
            deg = 36 if s == 5 else (1 if s % 3 == 0 else 5)
            for t in rng.choice([v for v in range(n) if v != s], size=deg, replace=False):
                e.append((s, int(t)))
        e = np.array(e, dtype=np.int64)[rng.permutation(len(e))]
        return e.T.copy(), n
    raise KeyError(name)


@pytest.fixture(scope='module')
def graphs(mp):
    """name -> (GraphStructure, edge_index int64 on the CPU).  'rpu': one synthetic_case RPU batch of 2 graphs (knn: not symmetric)."""
    from msmp_pde_amd.graph import GraphStructure, structure_of
    out = {}
    for name in ('single', 'nine', 'thirty_seven'):
        ei, n = _edges(name)
        t = torch.tensor(ei).cuda()
        out[name] = (GraphStructure(t, torch.zeros(n, dtype=torch.int64, device='cuda'), n), torch.tensor(ei))
    case = synthetic_case(mp, 'RPU', bsz=2, seed=4)
    graph = case.graph.to('cuda')
    out['rpu'] = (structure_of(graph), graph.edge_index.cpu())
    out['rpu_case'] = (case, graph)
    return out


GRAPHS = ['single', 'nine', 'thirty_seven', 'rpu']


def _rows(n, w, seed):
    """h, a, b, g: order-one random rows [n, w], float32 on the CPU"""
    rng = np.random.default_rng(seed)
    return [torch.tensor(rng.standard_normal((n, w)), dtype=torch.float32) for _ in range(4)]


# ---- the float64 restatement -----------------------------------------------------------------------------------------------------------
def restate(h, a, b, ei):
    """(out, tau) of the formulas in the dtype and on the device of h; ei [2, E] int64 (row 0 source, row 1 target)"""
    ei = ei.to(h.device)
    swish = lambda x: x * torch.sigmoid(x)
    t = swish(a)
    d2 = (t[ei[0]] - t[ei[1]]).abs() ** 2
    cnt = torch.bincount(ei[0], minlength=t.shape[0]).clamp(min=1).to(t.dtype)
    tau = torch.tanh(torch.zeros_like(t).index_add_(0, ei[0], d2) / cnt[:, None])
    return (1.0 - tau) * h + tau * swish(b), tau


_REF = {}


def reference(graphs, name, w):
    """float64 (out, tau, dh, da, db) and the float32 inputs (h, a, b, g) of one case, computed once and shared"""
    key = (name, w)
    if key not in _REF:
        gs, ei = graphs[name]
        h, a, b, g = _rows(gs.n_nodes, w, seed=100 + w + gs.n_nodes)
        x = [t.double().requires_grad_(True) for t in (h, a, b)]
        out, tau = restate(*x, ei)
        (out * g.double()).sum().backward()
        _REF[key] = dict(inputs=(h, a, b, g), out=out.detach(), tau=tau.detach(), grads=[t.grad for t in x])
    return _REF[key]


# ---- the routes ------------------------------------------------------------------------------------------------------------------------
def _padded(t, ld):
    """[n, w] -> [n, ld] on the GPU with NaN in columns w .. ld - 1, allocated with torch.empty (guard bands around it)"""
    p = torch.empty(t.shape[0], ld, dtype=torch.float32, device='cuda')
    p.fill_(float('nan'))
    p[:, :t.shape[1]] = t.cuda()
    return p


def entry_forward(mp, gs, h, a, b, w, ld, save_tau=True):
    """msmp_g2_gate_blend_f32 on rows of stride ld -> (out, tau)[:, :w]"""
    from msmp_pde_amd._lib import check, ptr, current_stream
    rowptr, nbr = gs.out_edges32()
    hp, ap, bp = (_padded(t, ld) for t in (h, a, b))
    out, tau = _padded(torch.zeros_like(h), ld), (_padded(torch.zeros_like(h), ld) if save_tau else None)
    check(mp.lib().msmp_g2_gate_blend_f32(ptr(hp), ptr(ap), ptr(bp), ld, ptr(rowptr), ptr(nbr), gs.n_nodes, gs.n_edges, w, ptr(out), ptr(tau),
                                          current_stream()), 'msmp_g2_gate_blend_f32')
    assert bool(torch.isnan(out[:, w:]).all())                 # the padding columns are not written
    return out[:, :w].contiguous(), (tau[:, :w].contiguous() if save_tau else None)


def entry_backward(mp, gs, g, h, a, b, tau, w, ld):
    """msmp_g2_gate_blend_bwd_f32 on rows of stride ld -> (dh, da, db)[:, :w]"""
    from msmp_pde_amd._lib import check, ptr, current_stream
    L = mp.lib()
    rowptr, nbr = gs.out_edges32()
    gp, hp, ap, bp, tp = (_padded(t, ld) for t in (g, h, a, b, tau))
    outs = [_padded(torch.zeros_like(h), ld) for _ in range(3)]
    ws = torch.empty(L.msmp_g2_gate_blend_bwd_workspace_bytes(gs.n_nodes, w), dtype=torch.uint8, device='cuda')
    check(L.msmp_g2_gate_blend_bwd_f32(ptr(gp), ptr(hp), ptr(ap), ptr(bp), ptr(tp), ld, ptr(rowptr), ptr(nbr), ptr(gs.rowptr), ptr(gs.col), gs.n_nodes,
                                       gs.n_edges, w, *[ptr(t) for t in outs], ptr(ws), ws.numel(), current_stream()), 'msmp_g2_gate_blend_bwd_f32')
    return [t[:, :w].contiguous() for t in outs]


def hip_route(mp, gs, inputs, w, ld):
    """(out, tau, [dh, da, db]) of the kernels: through g2.g2_gate_blend and autograd where ld == w, through the entries otherwise"""
    from msmp_pde_amd import g2
    h, a, b, g = inputs
    if ld != w:
        out, tau = entry_forward(mp, gs, h, a, b, w, ld)
        return out, tau, entry_backward(mp, gs, g, h, a, b, tau.cpu(), w, ld)
    with tuned(mp.lib(), g2_gate=1):
        x = [t.cuda().requires_grad_(True) for t in (h, a, b)]
        out = g2.g2_gate_blend(*x, gs)
        assert out.grad_fn is not None and type(out.grad_fn).__name__.startswith('_G2GateBlend')
        tau = out.grad_fn.saved_tensors[3]
        (out * g.cuda()).sum().backward()
    return out.detach(), tau, [t.grad for t in x]


def f32_route_grads(mp, gs, ei, inputs, w):
    """dh, da, db of the float32 PyTorch-ops route: at width 128 the route of switch 0 itself (g2.g2_gate_blend, the mean on
    msmp_scatter_mean_f32); that kernel is 128 columns wide, so at other widths the same float32 ops with the mean as index_add_"""
    from msmp_pde_amd import g2
    h, a, b, g = inputs
    x = [t.cuda().requires_grad_(True) for t in (h, a, b)]
    if w == 128 and gs.n_edges:
        with tuned(mp.lib(), g2_gate=0):
            out = g2.g2_gate_blend(*x, gs)
            assert 'G2GateBlend' not in type(out.grad_fn).__name__
            (out * g.cuda()).sum().backward()
    else:
        (restate(*x, ei)[0] * g.cuda()).sum().backward()
    return [t.grad for t in x]


def _rel(x, ref, fallback):
    scale = ref.abs().max().item() or fallback
    return (x.double().cpu() - ref).abs().max().item() / scale


# ---- kernel level ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('w,ld', SHAPES)
@pytest.mark.parametrize('name', GRAPHS)
def test_forward_and_backward_match_the_float64_restatement(mp, graphs, name, w, ld):
    """out and tau within helpers.TOL of float64; out == h exactly on nodes without out-edges; dh, da, db: the error relative to the largest
    reference entry at most max(1e-6, FLOOR_FACTOR x the error of the float32 PyTorch-ops route against the same float64 gradients)."""
    gs, ei = graphs[name]
    ref = reference(graphs, name, w)
    out, tau, grads = hip_route(mp, gs, ref['inputs'], w, ld)
    e_out = (out.double().cpu() - ref['out']).abs().max().item()
    e_tau = (tau.double().cpu() - ref['tau']).abs().max().item()
    print(f'g2_gate[{name}, {w}, {ld}]: max|out - ref| = {e_out:.3e}, max|tau - ref| = {e_tau:.3e} (bar {TOL:.0e})')
    no_out = torch.bincount(ei[0], minlength=gs.n_nodes) == 0
    assert name == 'rpu' or bool(no_out.any())
    exact = torch.equal(out.cpu()[no_out], ref['inputs'][0][no_out]) and bool((tau.cpu()[no_out] == 0).all())
    f32 = f32_route_grads(mp, gs, ei, ref['inputs'], w)
    overall = max(r.abs().max().item() for r in ref['grads'])
    errs = {k: (_rel(x, r, overall), _rel(f, r, overall)) for k, x, f, r in zip(('dh', 'da', 'db'), grads, f32, ref['grads'])}
    for k, (e_hip, e_f32) in errs.items():
        print(f'g2_gate[{name}, {w}, {ld}] {k}: relative error {e_hip:.3e}, float32 PyTorch ops {e_f32:.3e} (bar {max(1e-6, FLOOR_FACTOR * e_f32):.1e})')
    record_parity('g2_gate', f'{name}/{w}/{ld}', out_max_abs=e_out, tau_max_abs=e_tau, bar=TOL,
                  **{f'{k}_{r}': v for k, pair in errs.items() for r, v in zip(('hip', 'f32_ops'), pair)})
    assert e_out <= TOL and e_tau <= TOL, (e_out, e_tau)
    assert exact
    for k, (e_hip, e_f32) in errs.items():
        assert e_hip <= max(1e-6, FLOOR_FACTOR * e_f32), (k, e_hip, e_f32)


@pytest.mark.parametrize('w,ld', SHAPES)
def test_two_runs_are_bitwise_equal_and_tau_null_gives_the_same_out(mp, graphs, w, ld):
    gs, _ = graphs['thirty_seven']
    h, a, b, g = reference(graphs, 'thirty_seven', w)['inputs']
    runs = []
    for _ in range(2):
        out, tau = entry_forward(mp, gs, h, a, b, w, ld)
        runs.append([out, tau] + entry_backward(mp, gs, g, h, a, b, tau.cpu(), w, ld))
    for x, y in zip(*runs):
        assert torch.equal(x, y)
    assert torch.equal(entry_forward(mp, gs, h, a, b, w, ld, save_tau=False)[0], runs[0][0])


def test_out_edge_lists_are_the_targets_regrouped_by_source(mp, graphs):
    """GraphStructure.out_edges32(): out_nbr = tgt[perm] of by_source32(), its rowptr; built once."""
    for name in GRAPHS:
        gs, ei = graphs[name]
        rowptr, nbr = gs.out_edges32()
        assert gs.out_edges32()[1] is nbr and rowptr.dtype == nbr.dtype == torch.int32 and nbr.numel() == max(gs.n_edges, 1)
        src, tgt = gs.col[:gs.n_edges].cpu().numpy(), gs.tgt[:gs.n_edges].cpu().numpy()
        order = np.argsort(src, kind='stable')
        assert np.array_equal(nbr[:gs.n_edges].cpu().numpy(), tgt[order])
        assert np.array_equal(rowptr.cpu().numpy(), np.concatenate(([0], np.cumsum(np.bincount(src, minlength=gs.n_nodes)))))


# ---- the pair of the class ---------------------------------------------------------------------------------------------------------------
def _pair_inputs(mp, graphs, hidden, seed):
    from msmp_pde_amd.layers import mp_layer
    case, graph = graphs['rpu_case']
    gs, ei = graphs['rpu']
    torch.manual_seed(seed)
    model = getattr(mp, KIND)(case.pde, time_window=TW, eq_variables=case.eqv, hidden_layer=1, hidden_features=hidden).cuda().eval()
    u, pos_x, _, variables, _ = model._prepare(graph, False)
    h = torch.tensor(np.random.default_rng(seed).standard_normal((gs.n_nodes, hidden)), dtype=torch.float32).cuda()
    with torch.no_grad():
        a = mp_layer(h, u, pos_x, variables, gs, model.gnn_layers_gate[0], None)
        b = mp_layer(h, u, pos_x, variables, gs, model.gnn_layers[0], None)
    ref = restate(h.double().cpu(), a.double().cpu(), b.double().cpu(), ei)[0]
    return model, (h, u, pos_x, variables, gs, 0), ref


def test_pair_against_the_pytorch_ops_route(mp, graphs):
    """_g2_pair on the RPU batch with the switch at 0 and at 1: both within TOL of the float64 restatement on the two layers' outputs; their
    difference (tanh and Swish rounding only) is printed and recorded."""
    model, args, ref = _pair_inputs(mp, graphs, 128, seed=7)
    outs = {}
    for key in (0, 1):
        with tuned(mp.lib(), g2_gate=key), torch.no_grad():
            outs[key] = model._g2_pair(*args)
    errs = {key: (o.double().cpu() - ref).abs().max().item() for key, o in outs.items()}
    diff = (outs[0] - outs[1]).abs().max().item()
    print(f'g2 pair RPU x 2: max|key 0 - float64| = {errs[0]:.3e}, max|key 1 - float64| = {errs[1]:.3e}, max|key 0 - key 1| = {diff:.3e}')
    record_parity('g2_gate_pair', 'RPU/2', key0_max_abs=errs[0], key1_max_abs=errs[1], key0_vs_key1_max_abs=diff, bar=TOL)
    assert errs[0] <= TOL and errs[1] <= TOL, errs


def test_pair_at_width_164_takes_the_launch(mp, graphs, monkeypatch):
    """The pair of a 164-wide model (the width-generic layers) runs through the one launch and meets TOL against the float64 restatement on the
    two layers' outputs.  (The class as a whole cannot run at 164: its decoder CNN yields time_window steps from 128 features only.)"""
    model, args, ref = _pair_inputs(mp, graphs, 164, seed=8)
    calls = counted(mp, monkeypatch, 'msmp_g2_gate_blend_f32')
    with tuned(mp.lib(), g2_gate=1), torch.no_grad():
        out = model._g2_pair(*args)
    err = (out.double().cpu() - ref).abs().max().item()
    print(f'g2 pair RPU x 2 at width 164: max|hip - float64| = {err:.3e}')
    assert len(calls) == 1 and out.shape == (args[4].n_nodes, 164)
    assert err <= TOL, err


# ---- the class ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('exp', ['RPU', 'MSWG3'])
def test_class_forward_and_gradients_match_the_float64_oracle(mp, exp, monkeypatch):
    """MP_PDE_Solver2DLEMLinG2 with hidden_layer=2 on 3 graphs, switch 1: exactly hidden_layer launches under no_grad; the forward through
    assert_parity with the float32 floors; the parameter gradients by the procedure and bars of test_gradients_match_float64_oracle."""
    torch.manual_seed(2)
    case = synthetic_case(mp, exp, bsz=3, seed=4)
    model = getattr(mp, KIND)(case.pde, time_window=TW, eq_variables=case.eqv, hidden_layer=2).cuda()
    graph = case.graph.to('cuda')
    fwd, bwd = counted(mp, monkeypatch, 'msmp_g2_gate_blend_f32'), counted(mp, monkeypatch, 'msmp_g2_gate_blend_bwd_f32')
    with tuned(mp.lib(), g2_gate=1):
        with torch.no_grad():
            out = model(graph)
            assert len(fwd) == 2 and not bwd
            assert torch.equal(out, model(graph))
        pred = model(graph)
        loss = torch.sqrt(((pred - graph.y.to(pred.dtype)) ** 2).sum())
        loss.backward()
        assert len(fwd) == 6 and len(bwd) == 2
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    g = case.graph_np()
    ref = O.solver_forward(KIND, sd, g, case.pde, TW, case.eqv, 2)
    assert_parity('g2_gate_class', f'{KIND}/{exp}', out.double().cpu().numpy(), ref, fp32_floors(KIND, sd, g, case.pde, TW, case.eqv, 2))

    sd64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    out64 = OT.solver_forward(KIND, sd64, g, case.pde, TW, case.eqv, 2, as_numpy=False)
    ref_loss = torch.sqrt(((out64 - torch.tensor(g.y).double()) ** 2).sum())
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 1e-4 * ref_loss.item()
    scale = max(sd64[name].grad.abs().max().item() for name, _ in model.named_parameters())
    worst = 0.0
    for name, p in model.named_parameters():
        gr, r = p.grad.double().cpu(), sd64[name].grad
        if name.endswith('update_net_2.0.bias'):        # analytically zero (feeds an InstanceNorm): an absolute bound
            assert (gr - r).abs().max().item() < 1e-4 * scale, (name, (gr - r).abs().max().item(), scale)
            continue
        rel = (gr - r).abs().max().item() / max(r.abs().max().item(), 1e-3 * scale)
        worst = max(worst, rel)
        assert rel < 2e-3, (name, rel)
    print(f'{KIND}/{exp} g2_gate 1: loss {loss.item():.6f} (oracle {ref_loss.item():.6f}); worst relative gradient error {worst:.2e}')
    record_parity('g2_gate_class_gradients', f'{KIND}/{exp}', worst_rel=worst, bar=2e-3)


@pytest.mark.parametrize('exp', ['RPU', 'MSWG3'])
def test_packed_feature_rows_leave_the_class_output_bitwise_equal(mp, exp, monkeypatch):
    """_g2_pair hands the packed feature rows that _forward builds to both layer calls: the no-grad output of the class is bitwise what it is
    when the layers assemble those columns themselves (feat = None), and the rows do reach the layers."""
    from msmp_pde_amd import solvers
    torch.manual_seed(3)
    case = synthetic_case(mp, exp, bsz=3, seed=5)
    model = getattr(mp, KIND)(case.pde, time_window=TW, eq_variables=case.eqv, hidden_layer=2).cuda().eval()
    graph = case.graph.to('cuda')
    real, seen = solvers.mp_layer, []

    def without_feat(*a, feat=None, **kw):
        seen.append(feat is not None)
        return real(*a, feat=None, **kw)
    with torch.no_grad():
        out = model(graph)
        monkeypatch.setattr(solvers, 'mp_layer', without_feat)
        out_none = model(graph)
    from msmp_pde_amd.graph import structure_of
    tiled = structure_of(graph).tiles() is not None            # _forward packs the rows for the tile kernel only
    assert seen == [tiled] * 4 and (tiled or exp != 'MSWG3')
    assert torch.equal(out, out_none)


def test_captured_training_step_follows_the_eager_trajectory(mp, monkeypatch):
    """train.CapturedTrainStep of MSG2-PDE2D at batch 2 with the switch on: bit-identical losses and parameters over 3 steps of changing batches."""
    from msmp_pde_amd import train as T
    from msmp_pde_amd.synthetic import make_case
    bsz = 2
    c = make_case('RPU', bsz, seed=9, device='cuda', dtype=torch.float32)
    gs = []
    for i in range(3):
        steps = [40 + 7 * i + j for j in range(bsz)]
        data, labels = c.creator.create_data(c.u_super, steps)
        gs.append(c.creator.create_graph(data, labels, c.x, c.variables, steps))
    fwd, bwd = counted(mp, monkeypatch, 'msmp_g2_gate_blend_f32'), counted(mp, monkeypatch, 'msmp_g2_gate_blend_bwd_f32')

    def run_steps(captured):
        torch.manual_seed(11)
        model = mp.MODEL_NAMES['MSG2-PDE2D'](c.pde, time_window=25, eq_variables=c.eqv, hidden_layer=2).cuda()
        opt = mp.optim.AdamW(model.parameters(), lr=1e-3, capturable=True)
        losses = []
        step = T.CapturedTrainStep(model, opt, gs[0], warmup=3) if captured else None
        for g in gs:
            if captured:
                losses.append(step(g))
            else:
                opt.zero_grad(set_to_none=True)
                losses.append(T.dp_loss_backward(model, g).detach().clone())
                opt.step()
        torch.cuda.synchronize()
        return losses, [p.detach().clone() for p in model.parameters()]

    with tuned(mp.lib(), g2_gate=1):
        le, we = run_steps(False)
        assert len(fwd) == 2 * 3 and len(bwd) == 2 * 3                 # both pairs, every eager step
        lc, wc = run_steps(True)
    assert all(torch.isfinite(l) for l in lc) and float(lc[-1]) != float(lc[0])
    for i in range(3):
        assert torch.equal(le[i], lc[i]), (i, float(le[i]), float(lc[i]))
    for a, b in zip(we, wc):
        assert torch.equal(a, b)
