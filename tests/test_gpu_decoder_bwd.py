"""GPU tests of the decoder under autograd on the HIP kernels (decoder_bwd_kernel.hip, msmp-pde_amd/decoder.py, switch "dec_bwd"):
the four backward entries against float64 autograd of the same formula through torch.nn.functional.conv1d on the CPU, their bitwise
properties, the autograd Function against the PyTorch path of `_decode`, six solver classes against the float64 oracle, and a capture.

Bars (DESIGN.md section 7.1 / profiles/r17a): dh <= 2e-4 max(|ref|max, 1); a parameter gradient <= 1e-4 |ref|max + 2e-5 x the largest
gradient entry of the call; or twice the error of float32 CPU autograd of the same formula on the same inputs, whichever is larger."""
import copy

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import msmp_oracle_torch as OT
from helpers import mp, synthetic_case, record_parity, tuned       # noqa: F401  (mp: fixture)

pytestmark = pytest.mark.gpu
DT = 0.016
GEOMETRY = {20: (15, 4, 10), 25: (16, 3, 14), 50: (12, 2, 10)}
NODE_COUNTS = [1, 15, 16, 17, 31, 32, 33, 333]
N_MAX = 333
N_GRID = 16 * 512 + 2 * 16 + 5          # more than nodes-per-workgroup x the grid cap: a second grid-stride pass that ends in a part-filled block
LDS = {'gated': (164, 256), 'gated2d': (328, 384)}
# kind -> (entry kind, comps, row width, tw, euler)
KINDS = {'1d25': ('1d', 1, 128, 25, True), '2d25': ('2d', 2, 128, 25, True), 'gated': ('gated', 1, 164, 25, True), 'gated2d': ('gated2d', 2, 164, 25, True),
         '1d20': ('1d', 1, 128, 20, True), '1d50': ('1d', 1, 128, 50, True), '1d25diff': ('1d', 1, 128, 25, False), '2d50': ('2d', 2, 128, 50, True)}
SWEEP = ('1d25', '2d25', 'gated', 'gated2d')
REST = ('1d20', '1d50', '1d25diff', '2d50')
BWD = {'1d': 'msmp_decoder_bwd_f32', '2d': 'msmp_decoder2d_bwd_f32', 'gated': 'msmp_decoder_gated_bwd_f32', 'gated2d': 'msmp_decoder2d_gated_bwd_f32'}
FWD = {'1d': 'msmp_decoder_f32', '2d': 'msmp_decoder2d_f32', 'gated': 'msmp_decoder_gated_f32', 'gated2d': 'msmp_decoder2d_gated_f32'}


def swish(x):
    return x * torch.sigmoid(x)


def formula(entry, tw, euler, rows, u, params):
    """out [n, comps tw] of the decoder `entry` from rows [n, comps, W], u [n, comps tw] and the weights (w1, b1, w2, b2 per network) in the
    dtype of its arguments: experiments/models_gnn.py:275-279, 1514-1521, models_gnn2D.py:125-141, 1355-1366 through F.conv1d."""
    n, comps = rows.shape[0], rows.shape[1]
    dtc = torch.cumsum(torch.full((tw,), DT, dtype=rows.dtype), 0)
    if entry in ('1d', '2d'):
        s1 = GEOMETRY[tw][1]
        diff = F.conv1d(swish(F.conv1d(rows, params[0], params[1], stride=s1)), params[2], params[3])
        if not euler:
            return diff.flatten(1, 2)
        base = u[:, None, -1:] if entry == '1d' else u.view(n, 2, tw)
        return (base + dtc.view(1, 1, tw) * diff).flatten(1, 2)
    half = rows.shape[2] // 2
    net = lambda x, p: F.conv1d(swish(F.conv1d(x, p[0], p[1], stride=2)), p[2], p[3])
    scale, diff = net(rows[:, :, :half], params[:4]), net(rows[:, :, half:], params[4:])
    if comps == 1:
        return (1.0 - scale[:, 0]) * u[:, -1:] + dtc.view(1, tw) * (scale[:, 0] * diff[:, 0])
    return ((1.0 - scale) * u.view(n, 2, tw) + dtc.view(1, 1, tw) * scale * diff).flatten(1, 2)


def autograd_of(entry, tw, euler, rows, u, g, params, dtype):
    """(out, d rows, [d params]) of sum(out g) by CPU autograd in `dtype`"""
    r = rows.to(dtype).requires_grad_(True)
    p = [t.detach().to(dtype).requires_grad_(True) for t in params]
    out = formula(entry, tw, euler, r, u.to(dtype), p)
    grads = torch.autograd.grad((out * g.to(dtype)).sum(), [r] + p)
    return out.detach(), grads[0], list(grads[1:])


def bars(ref_dh, ref_params, floor_dh, floor_params):
    """(bar of dh, [bar per parameter]) from the float64 gradients and the errors of the float32 CPU autograd"""
    largest = max(r.abs().max().item() for r in ref_params)
    bar_dh = max(2e-4 * max(ref_dh.abs().max().item(), 1.0), 2.0 * floor_dh)
    return bar_dh, [max(1e-4 * r.abs().max().item() + 2e-5 * largest, 2.0 * f) for r, f in zip(ref_params, floor_params)]


class _Shared:
    """inputs of one decoder geometry, made once: rows, u, grad_out standard normal, nn.Conv1d default init; float64 / float32 CPU autograd
    per node count, cached (read only)"""

    def __init__(self, kind, n_max, seed):
        self.kind = kind
        self.entry, self.comps, self.W, self.tw, self.euler = KINDS[kind]
        rng = np.random.default_rng(seed)
        t = lambda *shape: torch.tensor(rng.standard_normal(shape), dtype=torch.float32)
        self.rows, self.u, self.g = t(n_max, self.comps, self.W), t(n_max, self.comps * self.tw), t(n_max, self.comps * self.tw)
        self.fill = t(n_max, 384)
        torch.manual_seed(seed)
        k1, s1, k2 = (6, 2, 15) if self.entry.startswith('gated') else GEOMETRY[self.tw]
        nets = [(torch.nn.Conv1d(self.comps, 8, k1, stride=s1), torch.nn.Conv1d(8, self.comps, k2)) for _ in range(2 if self.entry.startswith('gated') else 1)]
        self.params = [p.detach() for c1, c2 in nets for p in (c1.weight, c1.bias, c2.weight, c2.bias)]
        self.weights = [p.cuda().contiguous() for p in self.params]
        self._refs = {}

    def reference(self, n):
        """float64 (out, dh, params) of the first n nodes and the max abs errors of float32 CPU autograd (dh, [params])"""
        if n not in self._refs:
            a = (self.entry, self.tw, self.euler, self.rows[:n], self.u[:n], self.g[:n], self.params)
            out, dh, dp = autograd_of(*a, torch.float64)
            _, dh32, dp32 = autograd_of(*a, torch.float32)
            self._refs[n] = (out, dh, dp, (dh32.double() - dh).abs().max().item(), [(a32.double() - b).abs().max().item() for a32, b in zip(dp32, dp)])
        return self._refs[n]

    def strided(self, ld, sel=slice(None)):
        """the rows `sel` at row stride ld on the GPU, the floats past a row's comps * W values random"""
        x = self.fill[sel, :ld].clone()
        x[:, :self.comps * self.W] = self.rows[sel].reshape(-1, self.comps * self.W)
        return x.cuda().contiguous()


_SHARED = {}


@pytest.fixture(scope='module')
def shared():
    def get(kind, n_max=N_MAX):
        if (kind, n_max) not in _SHARED:
            _SHARED[kind, n_max] = _Shared(kind, n_max, 50 + sorted(KINDS).index(kind) + (n_max != N_MAX))
        return _SHARED[kind, n_max]
    return get


def run_bwd(mp, s, x, ld, u, g):
    """the backward entry of s's geometry on GPU tensors: (dh compact, [parameter gradients])"""
    from msmp_pde_amd._lib import check, ptr, current_stream
    L = mp.lib()
    n = x.shape[0]
    gated = int(s.entry.startswith('gated'))
    dh = torch.full((n, s.comps, s.W), float('nan'), device='cuda')
    grads = [torch.full_like(w, float('nan')) for w in s.weights]
    ws = torch.empty(L.msmp_decoder_bwd_workspace_bytes(s.comps, gated, s.W, s.tw), dtype=torch.uint8, device='cuda')
    tail = [ptr(dh)] + [ptr(t) for t in grads] + [ptr(ws), ws.numel(), current_stream()]
    w = [ptr(t) for t in s.weights]
    name = BWD[s.entry]
    if gated:
        rc = getattr(L, name)(ptr(g), ptr(x), ld, ptr(u), n, s.W, s.tw, *w, DT, *tail)
    elif s.comps == 2:
        rc = getattr(L, name)(ptr(g), ptr(x), n, s.tw, *w, DT, *tail)
    else:
        rc = getattr(L, name)(ptr(g), ptr(x), n, s.tw, int(s.euler), *w, DT, *tail)
    check(rc, name)
    return dh, grads


def run_fwd(mp, s, x, ld, u, train):
    from msmp_pde_amd._lib import check, ptr, current_stream
    name = FWD[s.entry].replace('_f32', '_train_fwd_f32') if train else FWD[s.entry]
    n = x.shape[0]
    out = torch.empty(n, s.comps * s.tw, device='cuda')
    w = [ptr(t) for t in s.weights]
    if s.entry.startswith('gated'):
        rc = getattr(mp.lib(), name)(ptr(x), ld, ptr(u), n, s.W, s.tw, *w, DT, ptr(out), current_stream())
    else:
        rc = getattr(mp.lib(), name)(ptr(x), ptr(u) if s.euler else None, n, s.tw, *w, DT, ptr(out), current_stream())
    check(rc, name)
    return out


def check_against_float64(mp, s, n, ld, case):
    x, u, g = s.strided(ld, slice(0, n)), s.u[:n].cuda().contiguous(), s.g[:n].cuda().contiguous()
    dh, grads = run_bwd(mp, s, x, ld, u, g)
    _, ref_dh, ref_p, floor_dh, floor_p = s.reference(n)
    bar_dh, bar_p = bars(ref_dh, ref_p, floor_dh, floor_p)
    err_dh = (dh.double().cpu() - ref_dh).abs().max().item()
    err_p = [(a.double().cpu() - b).abs().max().item() for a, b in zip(grads, ref_p)]
    print(f'decoder backward {case}: dh err {err_dh:.3e} (bar {bar_dh:.3e}, float32 floor {floor_dh:.3e}, max|ref| {ref_dh.abs().max().item():.3g}); parameters '
          + ', '.join(f'{e:.2e}/{b:.2e}' for e, b in zip(err_p, bar_p)))
    record_parity('decoder_backward', case, dh_err=err_dh, dh_bar=bar_dh, dh_floor=floor_dh, param_err=err_p, param_bar=bar_p, param_floor=floor_p)
    assert err_dh <= bar_dh, (case, err_dh, bar_dh)                 # NaN (an element never written) fails this as well
    for i, (e, b) in enumerate(zip(err_p, bar_p)):
        assert e <= b, (case, i, e, b)


SWEEP_CASES = [(k, ld, n) for k in SWEEP for ld in LDS.get(k, (KINDS[k][1] * KINDS[k][2],)) for n in NODE_COUNTS]
REST_CASES = [(k, KINDS[k][1] * KINDS[k][2], n) for k in REST for n in (33, 333)]


@pytest.mark.parametrize('kind,ld,n', SWEEP_CASES + REST_CASES)
def test_entries_against_float64_autograd(mp, shared, kind, ld, n):
    check_against_float64(mp, shared(kind), n, ld, f'{kind}/ld{ld}/n{n}')


@pytest.mark.parametrize('kind', SWEEP)
def test_more_nodes_than_one_pass_of_the_capped_grid(mp, shared, kind):
    s = shared(kind, N_GRID)
    check_against_float64(mp, s, N_GRID, LDS.get(kind, (s.comps * s.W,))[-1], f'{kind}/n{N_GRID}')


@pytest.mark.parametrize('kind', SWEEP)
def test_bitwise_properties(mp, shared, kind):
    s = shared(kind)
    lds = LDS.get(kind, (s.comps * s.W,))
    ld = lds[-1]
    x, u, g = s.strided(ld), s.u.cuda().contiguous(), s.g.cuda().contiguous()
    dh, grads = run_bwd(mp, s, x, ld, u, g)
    dh2, grads2 = run_bwd(mp, s, x, ld, u, g)                                               # two calls
    assert torch.equal(dh, dh2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))
    lo = 100                                                                                # rows 100 .. 116 as a 17-node call of their own
    few, _ = run_bwd(mp, s, x[lo:lo + 17].contiguous(), ld, u[lo:lo + 17].contiguous(), g[lo:lo + 17].contiguous())
    assert torch.equal(few, dh[lo:lo + 17])
    perm = torch.randperm(N_MAX, generator=torch.Generator().manual_seed(5)).cuda()
    dhp, _ = run_bwd(mp, s, x[perm].contiguous(), ld, u[perm].contiguous(), g[perm].contiguous())
    assert torch.equal(dhp, dh[perm])                                                       # permuted nodes
    if len(lds) > 1:                                                                        # the row stride changes no bit
        dh0, grads0 = run_bwd(mp, s, s.strided(lds[0]), lds[0], u, g)
        assert torch.equal(dh0, dh) and all(torch.equal(a, b) for a, b in zip(grads0, grads))
    assert torch.equal(run_fwd(mp, s, x, ld, u, train=True), run_fwd(mp, s, x, ld, u, train=False))


# ---- the Function against the PyTorch path of _decode --------------------------------------------------------------------------
FAMILIES = [('MP_PDE_Solver', 'E2'), ('MP_PDE_Solver2D', 'MSWG3'), ('MP_PDE_SolverLEMLinGatedGLU', 'E2'), ('MP_PDE_Solver2DLEMLinGatedGLU', 'MSWG3')]


def decode_modules(model):
    glu = hasattr(model, 'output_mlp_gate')
    nets = [model.output_mlp_gate, model.output_mlp_diff] if glu else [model.output_mlp]
    params = [p for net in nets for p in (net[0].weight, net[0].bias, net[2].weight, net[2].bias)]
    return glu, params, ([model.double_mlp[0].weight, model.double_mlp[0].bias] if model.TWO_D else [])


def decode_reference(model, h, u, g, dtype):
    """(out, dh, [d decoder params + d double_mlp params]) of model._decode's formula by CPU autograd in `dtype`"""
    glu, params, dm = decode_modules(model)
    tw = model.time_window
    entry = ('gated2d' if model.TWO_D else 'gated') if glu else ('2d' if model.TWO_D else '1d')
    hh = h.detach().cpu().to(dtype).requires_grad_(True)
    p = [t.detach().cpu().to(dtype).requires_grad_(True) for t in params + dm]
    rows = swish(F.linear(hh, p[-2], p[-1])).view(hh.shape[0], 2, -1) if model.TWO_D else hh[:, None, :]
    out = formula(entry, tw, True, rows, u.detach().cpu().to(dtype), p[:len(params)])
    grads = torch.autograd.grad((out * g.detach().cpu().to(dtype)).sum(), [hh] + p)
    return out.detach(), grads[0], list(grads[1:])


@pytest.mark.parametrize('kind,exp', FAMILIES)
def test_function_against_the_pytorch_path(mp, kind, exp):
    torch.manual_seed(7)
    case = synthetic_case(mp, exp, bsz=2, seed=3)
    model = getattr(mp, kind)(case.pde, time_window=25, eq_variables=case.eqv, hidden_layer=1).cuda()
    model.pde.dt = DT
    glu, params, dm = decode_modules(model)
    n, W, tw, comps = 77, model.hidden_features, 25, 2 if model.TWO_D else 1
    gen = torch.Generator().manual_seed(9)
    h, u, g = (torch.randn(n, c, generator=gen).cuda() for c in (W, comps * tw, comps * tw))
    ref_out, ref_dh, ref_p = decode_reference(model, h, u, g, torch.float64)
    out32, dh32, p32 = decode_reference(model, h, u, g, torch.float32)
    floor_out = (out32.double() - ref_out).abs().max().item()
    bar_dh, bar_p = bars(ref_dh, ref_p, (dh32.double() - ref_dh).abs().max().item(), [(a.double() - b).abs().max().item() for a, b in zip(p32, ref_p)])
    bar_out = max(1e-6, 2.0 * floor_out)                # the forward bar of test_gpu_gated_decoder.py
    outs = {}
    for value in (1, 0):
        with tuned(mp.lib(), dec_bwd=value):
            hv = h.clone().requires_grad_(True)
            model.zero_grad(set_to_none=True)
            out = model._decode(hv, u, u, model._dt(h.device), tw)
            out.backward(g)
        outs[value] = out.detach()
        on_function = 'DecoderFunction' in type(out.grad_fn).__name__
        assert on_function == bool(value), (kind, value, type(out.grad_fn).__name__)
        e_out = (out.detach().double().cpu() - ref_out).abs().max().item()
        e_dh = (hv.grad.double().cpu() - ref_dh).abs().max().item()
        e_p = [(q.grad.double().cpu() - r).abs().max().item() for q, r in zip(params + dm, ref_p)]
        print(f'{kind} dec_bwd {value}: out err {e_out:.3e} (bar {bar_out:.3e}), dh err {e_dh:.3e} (bar {bar_dh:.3e}), parameters '
              + ', '.join(f'{e:.2e}/{b:.2e}' for e, b in zip(e_p, bar_p)))
        record_parity('decoder_backward', f'{kind}/_decode/dec_bwd{value}', out_err=e_out, out_bar=bar_out, dh_err=e_dh, dh_bar=bar_dh, param_err=e_p, param_bar=bar_p)
        assert e_out <= bar_out and e_dh <= bar_dh, (kind, value, e_out, bar_out, e_dh, bar_dh)
        for i, (e, b) in enumerate(zip(e_p, bar_p)):
            assert e <= b, (kind, value, i, e, b)
    assert (outs[1] - outs[0]).abs().max().item() <= bar_out


# ---- solvers ---------------------------------------------------------------------------------------------------------------------
SOLVERS = [('MP_PDE_Solver', 'E2', 25), ('MP_PDE_Solver2DGated', 'RPU', 25), ('MSSMP_PDE_Solver', 'E2', 25), ('MP_PDE_SolverLEMLinGatedGLU', 'E2', 25),
           ('MP_PDE_Solver2DLEMLinGatedGLU', 'MSWG3', 25), ('MP_PDE_SolverGated', 'E2', 50)]


def case_at(mp, exp, bsz, seed, tw):
    if tw == 25:
        return synthetic_case(mp, exp, bsz=bsz, seed=seed)
    from types import SimpleNamespace
    from msmp_pde_amd.synthetic import make_case
    c = make_case(exp, bsz, seed=seed, device='cuda', tw=tw, dtype=torch.float64)
    steps = [tw] * bsz
    data, labels = c.creator.create_data(c.u_super, steps)
    c.graph = c.creator.create_graph(data, labels, c.x, c.variables, steps)
    c.graph_np = lambda: SimpleNamespace(**{k: v.detach().cpu().numpy() for k, v in c.graph.__dict__.items() if torch.is_tensor(v)})
    return c


def function_nodes(fn):
    """the DecoderFunction nodes of the autograd graph behind `fn`"""
    seen, stack, found = set(), [fn], []
    while stack:
        f = stack.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        if 'DecoderFunction' in type(f).__name__:
            found.append(f)
        stack.extend(nf for nf, _ in f.next_functions)
    return found


@pytest.mark.parametrize('kind,exp,tw', SOLVERS)
def test_solver_gradients_match_float64_oracle(mp, kind, exp, tw):
    """test_gradients_match_float64_oracle (test_gpu_training.py) with the decoder on the HIP kernels; the autograd graph is the witness of
    the path: a DecoderFunction node per decoder with the switch at 1, none at 0."""
    torch.manual_seed(2)
    case = case_at(mp, exp, 3, 4, tw)
    model = getattr(mp, kind)(case.pde, time_window=tw, eq_variables=case.eqv, hidden_layer=2).cuda()
    graph = case.graph.to('cuda')
    assert graph.x.dtype == torch.float64
    with tuned(mp.lib(), dec_bwd=0):
        assert function_nodes(model(graph).grad_fn) == []
    with tuned(mp.lib(), dec_bwd=1):
        pred = model(graph)
        assert len(function_nodes(pred.grad_fn)) == (2 if kind == 'MSSMP_PDE_Solver' else 1)
        assert pred.dtype == torch.float64
        loss = torch.sqrt(((pred - graph.y.to(pred.dtype)) ** 2).sum())
        loss.backward()
    sd64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    out = OT.solver_forward(kind, sd64, case.graph_np(), case.pde, tw, case.eqv, 2, as_numpy=False)
    ref_loss = torch.sqrt(((out - torch.tensor(case.graph_np().y).double()) ** 2).sum())
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 1e-4 * ref_loss.item()
    scale = max(sd64[name].grad.abs().max().item() for name, _ in model.named_parameters())
    worst = 0.0
    lin_layers = 'Gated' in kind or kind.startswith('MSSMP')
    for name, p in model.named_parameters():
        gr, r = p.grad.double().cpu(), sd64[name].grad
        if lin_layers and name.endswith('update_net_2.0.bias'):        # analytically zero (feeds an InstanceNorm): an absolute bound
            assert (gr - r).abs().max().item() < 1e-4 * scale, (name, (gr - r).abs().max().item(), scale)
            continue
        rel = (gr - r).abs().max().item() / max(r.abs().max().item(), 1e-3 * scale)
        worst = max(worst, rel)
        assert rel < 2e-3, (name, rel)
    print(f'{kind}/{exp}/tw{tw} dec_bwd 1: loss {loss.item():.6f} (oracle {ref_loss.item():.6f}); worst relative gradient error {worst:.2e}')
    record_parity('decoder_backward', f'{kind}/{exp}/tw{tw}/solver', worst_rel=worst, bar=2e-3)


# ---- capture -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', SWEEP)
def test_captured_forward_and_backward_replay_the_eager_bits(mp, shared, kind):
    from msmp_pde_amd.decoder import DecoderFunction
    s = shared(kind)
    n = 77
    w = [t.clone().requires_grad_(True) for t in s.weights]
    inputs = [(s.rows[i:i + n].cuda().contiguous(), s.u[i:i + n].cuda().contiguous(), s.g[i:i + n].cuda().contiguous()) for i in (0, 100)]

    def step(rows, u, g):
        r = rows.requires_grad_(True)
        out = DecoderFunction.apply(s.entry, r, u, s.tw, DT, *w)
        return (out,) + torch.autograd.grad(out, [r] + w, g)

    # detached copies: a copy with a grad_fn would keep the eager autograd graph alive, and with it the weights' AccumulateGrad nodes, which
    # belong to the stream they were made on (here the default stream): the backward under capture would then wait across streams
    eager = [[t.detach().clone() for t in step(rows.clone(), u, g)] for rows, u, g in inputs]
    static = [t.clone() for t in inputs[0]]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(static[0].detach(), static[1], static[2])
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step(static[0].detach(), static[1], static[2])
    for (rows, u, g), want in list(zip(inputs, eager))[::-1]:
        for dst, src in zip(static, (rows, u, g)):
            dst.detach().copy_(src)
        graph.replay()
        torch.cuda.synchronize()
        for got, ref in zip(captured, want):
            assert torch.equal(got, ref)
