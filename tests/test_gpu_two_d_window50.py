"""The 2-D solvers at time_window 50 (experiments/models_gnn2D.py accepts 25 or 50): u then has 100 columns, so message_net_1's tail
[u_i - u_j | pos_i - pos_j | vars_i] is 102-109 columns wide, i.e. four 32-column chunks (two at time_window 25).  Forward at full depth,
one rollout step, the captured forward, both message paths of one layer, the exact-fp32 kernels, gradients and captured training,
each against the float64 oracle or the eager path."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import msmp_oracle as O
from oracle import msmp_oracle_torch as OT
from helpers import EXPERIMENTS, fp32_floors, assert_parity, err_stats, record_parity

pytestmark = pytest.mark.gpu
TW = 50
H = 128


@pytest.fixture(scope='module')
def mp():
    import msmp_pde_amd
    assert torch.cuda.is_available()
    return msmp_pde_amd


def case50(mp, exp, bsz, seed, step=50, dtype=torch.float64):
    """helpers.synthetic_case at time_window 50: graphs built by the product's GraphCreator from synthetic trajectories."""
    from types import SimpleNamespace
    from msmp_pde_amd.synthetic import make_case
    c = make_case(exp, bsz, seed=seed, device='cuda', tw=TW, dtype=dtype)
    steps = [step] * bsz
    data, labels = c.creator.create_data(c.u_super, steps)
    c.graph = c.creator.create_graph(data, labels, c.x, c.variables, steps)

    def graph_np():
        g = SimpleNamespace()
        for k, v in c.graph.__dict__.items():
            if torch.is_tensor(v):
                setattr(g, k, v.detach().cpu().numpy())
        return g
    c.graph_np = graph_np
    return c


FORWARD_CASES = [(kind, exp) for kind in ('MP_PDE_Solver2DLEMLinGated', 'MP_PDE_Solver2DGated', 'MP_PDE_Solver2D', 'MP_PDE_Solver2DLEMLin',
                                          'MP_PDE_Solver2DLEMLinG2', 'MP_PDE_Solver2DLSTMLin') for exp in ('MSWG3', 'RPU')]


@pytest.mark.parametrize('kind,exp', FORWARD_CASES)
def test_full_depth_window50_vs_oracle(mp, kind, exp):
    """Six layers / six gated pairs on 8 graphs at time_window 50 against the float64 oracle (bar: helpers.assert_parity);
    two calls are bitwise equal."""
    torch.manual_seed(3)
    c = case50(mp, exp, bsz=8, seed=11)
    model = getattr(mp, kind)(c.pde, time_window=TW, eq_variables=c.eqv, hidden_layer=6).cuda().eval()
    data = c.graph.to('cuda')
    with torch.no_grad():
        out = model(data)
        out2 = model(data)
    assert out.shape == (data.x.shape[0], data.x.shape[1])
    assert torch.equal(out, out2)
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    g = c.graph_np()
    ref = O.solver_forward(kind, sd, g, c.pde, TW, c.eqv, 6)
    floor = fp32_floors(kind, sd, g, c.pde, TW, c.eqv, 6)
    assert_parity('two_d_window50', f'{kind}/{exp}', out.double().cpu().numpy(), ref, floor)


@pytest.mark.parametrize('kind,exp', [('MP_PDE_Solver2DLEMLinGated', 'MSWG3'), ('MP_PDE_Solver2DGated', 'RPU')])
def test_window50_rollout_and_capture(mp, kind, exp):
    """One unrolled step (create_next_graph) against O.rollout, and the hipGraph replay of Solver.capture() against eager, bit for bit."""
    torch.manual_seed(5)
    c = case50(mp, exp, bsz=4, seed=7)
    model = getattr(mp, kind)(c.pde, time_window=TW, eq_variables=c.eqv, hidden_layer=6).cuda().eval()
    data = c.graph.to('cuda')
    g0 = c.graph_np()                 # (create_next_graph updates the graph in place)
    same = [50 + TW] * 4
    with torch.no_grad():
        out = model(data)
        _, labels = c.creator.create_data(c.u_super, same)
        data2 = c.creator.create_next_graph(data, out, labels, same)
        pred = model(data2)
        step = model.capture(data2)
        assert torch.equal(step(data2), pred)
    sd = {k: v.detach().cpu().numpy().astype(np.float64) for k, v in model.state_dict().items()}
    traj = c.u_super.double().cpu().numpy()
    pde_name = EXPERIMENTS[exp][0]
    refs = O.rollout(kind, sd, g0, pde_name, c.pde, TW, c.eqv, 6, traj, 50, 1)
    f32 = O.rollout(kind, sd, g0, pde_name, c.pde, TW, c.eqv, 6, traj, 50, 1, dtype=np.float32)
    assert_parity('two_d_window50', f'{kind}/{exp}/rollout0', out.double().cpu().numpy(), refs[0], f32[0])
    assert_parity('two_d_window50', f'{kind}/{exp}/rollout1', pred.double().cpu().numpy(), refs[1], f32[1])


def _rand_layer_sd(rng, tw, nv):
    k1, k3 = 2 * H + tw + 1 + nv, 2 * H + nv
    u = lambda *s, fan: (rng.uniform(-1, 1, s) / np.sqrt(fan)).astype(np.float32)
    return {'message_net_1.0.weight': u(H, k1, fan=k1), 'message_net_1.0.bias': u(H, fan=k1),
            'message_net_2.0.weight': u(H, H, fan=H), 'message_net_2.0.bias': u(H, fan=H),
            'update_net_1.0.weight': u(H, k3, fan=k3), 'update_net_1.0.bias': u(H, fan=k3),
            'update_net_2.0.weight': u(H, H, fan=H), 'update_net_2.0.bias': u(H, fan=H)}


def _pack(mp, sd, tw, nv):
    from msmp_pde_amd._lib import check, ptr, current_stream
    L = mp.lib()
    blob = torch.empty(L.msmp_packed_layer_floats(tw, nv), dtype=torch.float32, device='cuda')
    keys = ['message_net_1.0.weight', 'message_net_1.0.bias', 'message_net_2.0.weight', 'message_net_2.0.bias',
            'update_net_1.0.weight', 'update_net_1.0.bias', 'update_net_2.0.weight', 'update_net_2.0.bias']
    ts = [torch.tensor(sd[k]).cuda().contiguous() for k in keys]
    check(L.msmp_pack_layer_f32(*[ptr(t) for t in ts], tw, nv, ptr(blob), current_stream()), 'pack')
    torch.cuda.synchronize()
    return blob


@pytest.mark.parametrize('exp,tw,nv,bsz,nx', [('MSWG3', 100, 3, 3, 100), ('RPU', 100, 3, 4, 100), ('RPU', 100, 8, 2, 100),
                                              ('MSWG3', 70, 3, 2, 100), ('RPU', 100, 3, 3, 40)])
def test_wide_tail_tiled_message_kernel_vs_gather_kernels_and_oracle(mp, exp, tw, nv, bsz, nx):
    """A layer with three or four tail chunks: msmp_edge_aggregate_tiled_f32 folded (P / Q projected in the workgroup; with and
    without the packed feature rows) and staged (P / Q rows from msmp_node_project_f32) against the gather kernels and the
    float64 oracle; repeated launches are bitwise identical."""
    from msmp_pde_amd._lib import check, ptr, current_stream
    from msmp_pde_amd.synthetic import make_case
    from msmp_pde_amd.graph import structure_of
    from msmp_pde_amd.layers import node_features
    L = mp.lib()
    c = make_case(exp, bsz, seed=3, device='cuda', nx=nx, dtype=torch.float64)
    data, labels = c.creator.create_data(c.u_super, [50] * bsz)
    gs = structure_of(c.creator.create_graph(data, labels, c.x, c.variables, [50] * bsz))
    t = gs.tiles()
    assert t is not None
    n, e = gs.n_nodes, gs.n_edges
    rng = np.random.default_rng(11)
    sd = _rand_layer_sd(rng, tw, nv)
    blob = _pack(mp, sd, tw, nv)
    h = torch.tensor(rng.standard_normal((n, H)), dtype=torch.float32).cuda()
    u = torch.tensor(rng.standard_normal((n, tw)).cumsum(0) * 0.05, dtype=torch.float32).cuda()
    pos = torch.tensor(rng.uniform(0, 1, n), dtype=torch.float32).cuda()
    var = torch.tensor(rng.uniform(0, 1, (n, nv)), dtype=torch.float32).cuda()
    P, Q = torch.empty(n, H, device='cuda'), torch.empty(n, H, device='cuda')
    ref, staged, folded, folded2, again = (torch.empty(n, H, device='cuda') for _ in range(5))
    st = current_stream()
    check(L.msmp_node_project_f32(ptr(h), ptr(u), ptr(pos), ptr(var), n, tw, nv, ptr(blob), ptr(P), ptr(Q), st), 'proj')
    check(L.msmp_edge_aggregate_projected_f32(ptr(P), ptr(Q), ptr(gs.rowptr), ptr(gs.col), ptr(gs.tgt), n, e, gs.max_in_degree, tw, nv,
                                              ptr(blob), ptr(ref), st), 'gather')
    check(L.msmp_edge_aggregate_tiled_f32(None, None, None, None, None, ptr(P), ptr(Q), ptr(gs.rowptr), ctypes.byref(t[0]), n, e, tw, nv,
                                          ptr(blob), ptr(staged), st), 'tiled staged')
    check(L.msmp_edge_aggregate_tiled_f32(ptr(h), ptr(u), ptr(pos), ptr(var), None, None, None, ptr(gs.rowptr), ctypes.byref(t[0]), n, e, tw, nv,
                                          ptr(blob), ptr(folded), st), 'tiled folded')
    feat = node_features(u, pos, var)
    assert feat.shape[1] == L.msmp_node_feature_stride(tw, nv) == 32 * ((tw + 1 + nv + 31) // 32)
    for out in (folded2, again):
        check(L.msmp_edge_aggregate_tiled_f32(ptr(h), ptr(u), ptr(pos), ptr(var), ptr(feat), None, None, ptr(gs.rowptr), ctypes.byref(t[0]), n, e,
                                              tw, nv, ptr(blob), ptr(out), st), 'tiled folded + feat')
    torch.cuda.synchronize()
    assert torch.equal(folded, folded2) and torch.equal(folded2, again)
    scale = ref.abs().max().item()
    assert (staged - ref).abs().max().item() < 2e-6 * scale and (folded - ref).abs().max().item() < 2e-6 * scale
    p64 = O.layer_params({k: v.astype(np.float64) for k, v in sd.items()}, '')
    ei = np.stack([gs.col.cpu().numpy()[:e], gs.tgt.cpu().numpy()[:e]])
    msg = O.edge_messages(p64, h.double().cpu().numpy(), u.double().cpu().numpy(), pos.double().cpu().numpy()[:, None],
                          var.double().cpu().numpy(), ei)
    agg = O.scatter_mean(msg, ei[1], n)
    den = max(np.abs(agg).max(), 1e-30)
    err = np.abs(folded.double().cpu().numpy() - agg).max() / den
    err_st = np.abs(staged.double().cpu().numpy() - agg).max() / den
    err_ga = np.abs(ref.double().cpu().numpy() - agg).max() / den
    print(f'{exp} tw={tw} nv={nv}: relative max error vs float64 oracle: folded {err:.2e}, staged {err_st:.2e}, gather {err_ga:.2e}')
    assert err < 1e-6 and err_st < 1e-6 and err_ga < 1e-6


@pytest.mark.parametrize('kind,exp', [('MP_PDE_Solver2DLEMLinGated', 'MSWG3'), ('MP_PDE_Solver2DGated', 'RPU')])
def test_window50_exact_fp32_kernels_vs_oracle(mp, kind, exp):
    """The same forward on the exact-fp32 kernels (msmp_tune("split", 0)) against the float64 oracle.  These kernels are held to
    5e-5 on the max error and to the parity bar on the rms error, not to the split path's max bar of twice the float32 floor
    (measured at full depth on MSWG3: 2.1e-5 max / 6.4e-7 rms against a floor of 3.7e-6 / 1.5e-7); a wrong tail misses both by
    orders of magnitude."""
    from msmp_pde_amd._lib import exact_fp32
    torch.manual_seed(3)
    c = case50(mp, exp, bsz=4, seed=13)
    model = getattr(mp, kind)(c.pde, time_window=TW, eq_variables=c.eqv, hidden_layer=6).cuda().eval()
    data = c.graph.to('cuda')
    with torch.no_grad(), exact_fp32():
        out = model(data)
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    g = c.graph_np()
    ref = O.solver_forward(kind, sd, g, c.pde, TW, c.eqv, 6)
    floors = fp32_floors(kind, sd, g, c.pde, TW, c.eqv, 6)
    err, rms = err_stats(out.double().cpu().numpy(), ref)
    floor_rms = max(err_stats(v, ref)[1] for v in floors.values())
    record_parity('two_d_window50', f'{kind}/{exp}/exact_fp32', max_err=err, rms_err=rms, floor_rms=floor_rms)
    assert err <= 5e-5 and rms <= max(1e-5, 2.0 * floor_rms), (err, rms, floor_rms)


@pytest.mark.parametrize('kind,exp', [('MP_PDE_Solver2DLEMLinGated', 'RPU'), ('MP_PDE_Solver2DLEMLinGated', 'MSWG3'),
                                      ('MP_PDE_Solver2DGated', 'RPU'), ('MP_PDE_Solver2DGated', 'MSWG3')])
def test_window50_gradients_match_float64_oracle(mp, kind, exp):
    """d loss / d parameters (loss sqrt(sum (pred - y)^2), two layers) against torch autograd through the float64 oracle; the layer
    backward (msmp_mp_layer_bwd_f32 at tw + 1 + nv = 104) gives bitwise the same gradients twice."""
    torch.manual_seed(2)
    c = case50(mp, exp, bsz=3, seed=4)
    model = getattr(mp, kind)(c.pde, time_window=TW, eq_variables=c.eqv, hidden_layer=2).cuda()
    graph = c.graph.to('cuda')
    grads = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        pred = model(graph)
        loss = torch.sqrt(((pred - graph.y.to(pred.dtype)) ** 2).sum())
        loss.backward()
        grads.append({k: p.grad.detach().clone() for k, p in model.named_parameters()})
    assert all(torch.equal(grads[0][k], grads[1][k]) for k in grads[0])
    sd64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    out = OT.solver_forward(kind, sd64, c.graph_np(), c.pde, TW, c.eqv, 2, as_numpy=False)
    y = torch.tensor(c.graph_np().y).double()
    ref_loss = torch.sqrt(((out - y) ** 2).sum())
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 1e-4 * ref_loss.item()
    scale = max(sd64[name].grad.abs().max().item() for name, _ in model.named_parameters())
    worst = 0.0
    for name, p in model.named_parameters():
        g, r = p.grad.double().cpu(), sd64[name].grad
        if name.endswith('update_net_2.0.bias'):       # GNN_LayerLin feeds its InstanceNorm directly: analytically zero
            assert (g - r).abs().max().item() < 1e-4 * scale, (name, (g - r).abs().max().item(), scale)
            continue
        rel = (g - r).abs().max().item() / max(r.abs().max().item(), 1e-3 * scale)
        worst = max(worst, rel)
        assert rel < 2e-3, (name, rel)
    print(f'{kind}/{exp}: loss {loss.item():.6f} (oracle {ref_loss.item():.6f}); worst relative gradient error {worst:.2e}')


def test_window50_captured_training_follows_the_eager_trajectory(mp):
    """train.CapturedTrainStep for MSMP-PDE2D at time_window 50: losses, parameters and the interleaved eager predictions of a few
    optimisation steps equal the eager trajectory bit for bit."""
    from msmp_pde_amd import train as T
    from msmp_pde_amd.synthetic import make_case
    bsz = 8
    c = make_case('MSWG3', bsz, seed=9, device='cuda', tw=TW, dtype=torch.float32)
    gs = []
    for i in range(4):
        steps = [50 + 7 * i + (j % 5) for j in range(bsz)]
        data, labels = c.creator.create_data(c.u_super, steps)
        gs.append(c.creator.create_graph(data, labels, c.x, c.variables, steps))

    def run(captured):
        torch.manual_seed(11)
        model = mp.MP_PDE_Solver2DLEMLinGated(c.pde, time_window=TW, eq_variables=c.eqv, hidden_layer=2).cuda()
        opt = mp.optim.AdamW(model.parameters(), lr=1e-3, capturable=True)
        losses, preds = [], []
        if captured:
            step = T.CapturedTrainStep(model, opt, gs[0], warmup=3)
        for i, g in enumerate(gs):
            if captured:
                losses.append(step(g))
            else:
                opt.zero_grad(set_to_none=True)
                losses.append(T.dp_loss_backward(model, g).detach().clone())
                opt.step()
            with torch.no_grad():
                preds.append(model(gs[(i + 1) % len(gs)]).clone())
        torch.cuda.synchronize()
        return losses, preds, [p.detach().clone() for p in model.parameters()]

    le, pe, we = run(False)
    lc, pc, wc = run(True)
    print('losses', [round(float(x), 5) for x in lc])
    assert all(torch.isfinite(x) for x in lc) and float(lc[-1]) != float(lc[0])
    for i in range(len(le)):
        assert torch.equal(le[i], lc[i]), (i, float(le[i]), float(lc[i]))
        assert torch.equal(pe[i], pc[i]), i
    assert all(torch.equal(a, b) for a, b in zip(we, wc))
