"""GPU tests of the Swish MLPs under autograd on the HIP kernels (mlp_train_kernel.hip, msmp-pde_amd/mlp.py, switch "mlp_train"): the
forward and backward entries against float64 CPU autograd of the same formula, their bitwise properties, the absence of an input range,
the autograd Function against the module, five solver classes (one per route) against the float64 oracle with the entries counted, and a
captured training step.

Bars (test_gpu_decoder_bwd.py): forward <= 1e-5; dx <= 2e-4 max(|ref|max, 1); a parameter gradient
<= 1e-4 |ref|max + 2e-5 x the largest gradient entry of the call; or twice the error of float32 CPU autograd of the same formula on the
same inputs, whichever is larger."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import msmp_oracle_torch as OT
from helpers import mp, synthetic_case, record_parity, tuned, counted       # noqa: F401  (mp: fixture)

pytestmark = pytest.mark.gpu
NAN = float('nan')
N_MAX = 333
SWEEP_N = (1, 31, 32, 33, 64, 97, 333)
FEW_N = (33, 97)
# (layers, heads, K, W, row stride of out or None = heads W + 5)
TWO_LAYER = [(2, 1, k, w, None) for k, w in ((128, 128), (164, 164), (28, 128), (31, 128), (55, 128), (105, 128), (1, 32), (33, 33), (256, 256))]
ONE_LAYER = [(1, 2, 128, 128, None), (1, 2, 164, 164, 384), (1, 1, 32, 33, None)]
# more input k-tiles than waves (K > 32 ceil(W / 32)), the other path of both kernels: x is published in several chunks, the last one
# part-filled (7 k-tiles on 2 waves), and a wave accumulates several dx tiles
MORE_K_TILES = [(2, 1, 100, 32, None), (1, 2, 200, 40, None)]
SWEPT = TWO_LAYER[:2] + ONE_LAYER[:1]
CASES = [(f, n) for f in SWEPT for n in SWEEP_N] + [(f, n) for f in TWO_LAYER[2:] + ONE_LAYER[1:] + MORE_K_TILES for n in FEW_N]


def swish(x):
    return x * torch.sigmoid(x)


def formula(x, p):
    a = swish(F.linear(x, p[0], p[1]))
    return swish(F.linear(a, p[2], p[3])) if len(p) == 4 else a


def autograd_of(x, g, params, dtype):
    """(out, dx, [d params], [pre-activations]) of sum(out g) by CPU autograd in `dtype`"""
    xx = x.to(dtype).requires_grad_(True)
    p = [t.detach().to(dtype).requires_grad_(True) for t in params]
    out = formula(xx, p)
    grads = torch.autograd.grad((out * g.to(dtype)).sum(), [xx] + p)
    with torch.no_grad():
        z = [F.linear(xx, p[0], p[1])]
        if len(p) == 4:
            z.append(F.linear(swish(z[0]), p[2], p[3]))
    return out.detach(), grads[0], list(grads[1:]), z


def bars(ref_dx, ref_params, floor_dx, floor_params):
    largest = max(r.abs().max().item() for r in ref_params)
    bar_dx = max(2e-4 * max(ref_dx.abs().max().item(), 1.0), 2.0 * floor_dx)
    return bar_dx, [max(1e-4 * r.abs().max().item() + 2e-5 * largest, 2.0 * f) for r, f in zip(ref_params, floor_params)]


class _Shared:
    """inputs of one form, made once: x and grad_out standard normal (times `scale`), nn.Linear default init; float64 / float32 CPU autograd per
    row count, cached (read only)"""

    def __init__(self, form, seed, scale=1.0):
        self.layers, self.heads, self.K, self.W, ld_out = form
        self.C = self.heads * self.W
        self.ld_out = self.C + 5 if ld_out is None else ld_out
        rng = np.random.default_rng(seed)
        self.x = torch.tensor(rng.standard_normal((N_MAX, self.K)) * scale, dtype=torch.float32)
        self.g = torch.tensor(rng.standard_normal((N_MAX, self.C)), dtype=torch.float32)
        torch.manual_seed(seed)
        lins = [torch.nn.Linear(self.K, self.C)] + ([torch.nn.Linear(self.W, self.W)] if self.layers == 2 else [])
        self.params = [p.detach() for lin in lins for p in (lin.weight, lin.bias)]
        self.weights = [p.cuda().contiguous() for p in self.params]
        self._refs = {}

    def reference(self, n):
        if n not in self._refs:
            out, dx, dp, z = autograd_of(self.x[:n], self.g[:n], self.params, torch.float64)
            _, dx32, dp32, _ = autograd_of(self.x[:n], self.g[:n], self.params, torch.float32)
            self._refs[n] = (out, dx, dp, z, (dx32.double() - dx).abs().max().item(), [(a.double() - b).abs().max().item() for a, b in zip(dp32, dp)])
        return self._refs[n]


_SHARED = {}


@pytest.fixture(scope='module')
def shared():
    def get(form, scale=1.0):
        if (form, scale) not in _SHARED:
            _SHARED[form, scale] = _Shared(form, 210 + (TWO_LAYER + ONE_LAYER + MORE_K_TILES).index(form), scale)
        return _SHARED[form, scale]
    return get


def strided(t, ld):
    """the rows of t [n, c] at row stride ld on the GPU, NaN in every float past a row's c values"""
    buf = torch.full((t.shape[0], ld), NAN)
    buf[:, :t.shape[1]] = t
    return buf.cuda()


def run(mp, s, n, with_dx):
    """pack, forward, backward of the first n rows through the C-ABI: dict of every output, NaN-prefilled"""
    from msmp_pde_amd._lib import check, ptr, current_stream
    L = mp.lib()
    rows = slice(0, n)
    la, he, K, W, C = s.layers, s.heads, s.K, s.W, s.C
    x, g = strided(s.x[rows], K + 3), strided(s.g[rows], C + 2)
    blob = torch.full((L.msmp_packed_mlp_train_floats(la, he, K, W),), NAN, device='cuda')
    w = s.weights + [None] * (4 - len(s.weights))
    check(L.msmp_pack_mlp_train_f32(*[ptr(t) for t in w], la, he, K, W, ptr(blob), current_stream()), 'pack')
    r = {'blob': blob}
    r['saved'] = torch.full((L.msmp_mlp_train_saved_floats(n, la, he, W),), NAN, device='cuda')
    r['out'] = torch.full((n, s.ld_out), NAN, device='cuda')
    check(L.msmp_mlp_train_fwd_f32(ptr(x), K + 3, n, la, he, K, W, ptr(blob), ptr(r['saved']), ptr(r['out']), s.ld_out, current_stream()), 'fwd')
    r['dx'] = torch.full((n, K + 1), NAN, device='cuda')
    r['grads'] = [torch.full_like(t, NAN) for t in s.weights]
    gp = [ptr(t) for t in r['grads']] + [None] * (4 - len(s.weights))
    ws = torch.empty(L.msmp_mlp_train_bwd_workspace_bytes(n, la, he, K, W), dtype=torch.uint8, device='cuda')
    check(L.msmp_mlp_train_bwd_f32(ptr(g), C + 2, ptr(x), K + 3, ptr(r['saved']), n, la, he, K, W, ptr(blob), ptr(r['dx']) if with_dx else None, K + 1,
                                   *gp, ptr(ws), ws.numel(), current_stream()), 'bwd')
    torch.cuda.synchronize()
    return r


def check_against_float64(mp, s, n, with_dx, case, relative_forward=False):
    r = run(mp, s, n, with_dx)
    ref_out, ref_dx, ref_p, ref_z, floor_dx, floor_p = s.reference(n)
    K, W, C, wp = s.K, s.W, s.C, 32 * ((s.W + 31) // 32)
    bar_dx, bar_p = bars(ref_dx, ref_p, floor_dx, floor_p)
    bar_out = 1e-5 * (max(ref_out.abs().max().item(), 1.0) if relative_forward else 1.0)
    out, dx = r['out'].cpu(), r['dx'].cpu()
    err_out = (out[:, :C].double() - ref_out).abs().max().item()
    err_p = [(a.double().cpu() - b).abs().max().item() for a, b in zip(r['grads'], ref_p)]
    err_dx = (dx[:, :K].double() - ref_dx).abs().max().item() if with_dx else 0.0
    print(f'mlp_train {case}: out err {err_out:.3e} (bar {bar_out:.1e}); dx err {err_dx:.3e} (bar {bar_dx:.3e}, float32 floor {floor_dx:.3e}); parameters '
          + ', '.join(f'{e:.2e}/{b:.2e}' for e, b in zip(err_p, bar_p)))
    record_parity('mlp_train', case, out_err=err_out, out_bar=bar_out, dx_err=err_dx, dx_bar=bar_dx, dx_floor=floor_dx, param_err=err_p, param_bar=bar_p,
                  param_floor=floor_p)
    assert err_out <= bar_out, (case, err_out)                          # NaN (an element never written) fails these as well
    assert torch.isnan(out[:, C:]).all(), case                          # nothing past a row's values is written
    saved = r['saved'].cpu().view(-1, n, wp)
    z = torch.stack(ref_z) if s.layers == 2 else ref_z[0].view(n, s.heads, W).permute(1, 0, 2)
    assert (saved[:, :, :W].double() - z).abs().max().item() <= 1e-5 * max(z.abs().max().item(), 1.0), case
    assert (saved[:, :, W:] == 0).all(), case                           # every element written; the padding channels are exact zeros
    if with_dx:
        assert err_dx <= bar_dx, (case, err_dx, bar_dx)
        assert torch.isnan(dx[:, K:]).all(), case
    else:
        assert torch.isnan(dx).all(), case                              # not touched
    for i, (e, b) in enumerate(zip(err_p, bar_p)):
        assert e <= b, (case, i, e, b)


@pytest.mark.parametrize('with_dx', (True, False), ids=('dx', 'nodx'))
@pytest.mark.parametrize('form,n', CASES, ids=lambda v: 'x'.join(str(i) for i in v) if isinstance(v, tuple) else str(v))
def test_entries_against_float64_autograd(mp, shared, form, n, with_dx):
    check_against_float64(mp, shared(form), n, with_dx, f'{form}/n{n}/{"dx" if with_dx else "nodx"}')


@pytest.mark.parametrize('form', SWEPT + ONE_LAYER[1:2] + MORE_K_TILES, ids=lambda v: 'x'.join(str(i) for i in v))
def test_bitwise_properties(mp, shared, form):
    s = shared(form)
    a, b = run(mp, s, 97, True), run(mp, s, 97, True)
    for key in ('blob', 'saved', 'out', 'dx'):                           # two runs: every output, NaN padding included
        assert torch.equal(a[key].view(torch.int32), b[key].view(torch.int32)), key
    assert all(torch.equal(p, q) for p, q in zip(a['grads'], b['grads']))
    few = run(mp, s, 33, True)                                          # the first 33 rows of the 97 as a call of their own
    wp = 32 * ((s.W + 31) // 32)
    assert torch.equal(few['out'][:, :s.C], a['out'][:33, :s.C]) and torch.equal(few['dx'][:, :s.K], a['dx'][:33, :s.K])
    assert torch.equal(few['saved'].view(-1, 33, wp), a['saved'].view(-1, 97, wp)[:, :33])
    few2 = run(mp, s, 33, True)
    assert all(torch.equal(p, q) for p, q in zip(few['grads'], few2['grads']))      # weight gradients: run to run (their row splits depend on N)


def test_no_input_range(mp, shared):
    """inputs of magnitude 1e4: finite results within the same relative bars, and the range status word stays clear"""
    import ctypes
    L = mp.lib()
    flags = ctypes.c_int(0)
    torch.cuda.synchronize()
    assert L.msmp_last_status(ctypes.byref(flags), 1) == 0
    s = shared(TWO_LAYER[0], 1e4)
    r = run(mp, s, 97, True)
    assert all(torch.isfinite(t[:, :c]).all() for t, c in ((r['out'], s.C), (r['dx'], s.K))) and all(torch.isfinite(t).all() for t in r['grads'])
    check_against_float64(mp, s, 97, True, f'{TWO_LAYER[0]}/n97/x1e4', relative_forward=True)
    torch.cuda.synchronize()
    assert L.msmp_last_status(ctypes.byref(flags), 0) == 0 and flags.value == 0


# ---- the Function against the module ---------------------------------------------------------------------------------------------------
def make_seq(mp, form, seed):
    from msmp_pde_amd.layers import Swish
    layers, heads, K, W, _ = form
    torch.manual_seed(seed)
    mods = [torch.nn.Linear(K, heads * W), Swish()] + ([torch.nn.Linear(W, W), Swish()] if layers == 2 else [torch.nn.Unflatten(1, (heads, W))])
    return torch.nn.Sequential(*mods).cuda()


@pytest.mark.parametrize('form', [TWO_LAYER[5], TWO_LAYER[1], ONE_LAYER[1]], ids=lambda v: 'x'.join(str(i) for i in v))
def test_function_against_the_module(mp, shared, monkeypatch, form):
    from msmp_pde_amd.mlp import swish_mlp
    calls = counted(mp, monkeypatch, 'msmp_mlp_train_fwd_f32')
    s = shared(form)
    seq = make_seq(mp, form, 31)
    params = [p for p in seq.parameters()]
    n = 97
    x, g = s.x[:n].cuda(), s.g[:n].cuda()
    ref_out, ref_dx, ref_p, _ = autograd_of(x.cpu(), g.cpu(), [p.detach().cpu() for p in params], torch.float64)
    o32, dx32, p32, _ = autograd_of(x.cpu(), g.cpu(), [p.detach().cpu() for p in params], torch.float32)
    bar_dx, bar_p = bars(ref_dx, ref_p, (dx32.double() - ref_dx).abs().max().item(), [(a.double() - b).abs().max().item() for a, b in zip(p32, ref_p)])
    results = {}
    for which in ('kernels', 'module'):
        xv = x.clone().requires_grad_(True)
        seq.zero_grad(set_to_none=True)
        out = swish_mlp(seq, xv, s.heads, s.ld_out if form[4] else None) if which == 'kernels' else seq(xv)
        assert out is not None and out.shape == ((n, s.heads, s.W) if s.layers == 1 else (n, s.W))
        assert len(calls) == 1                                          # the kernels' turn launched the forward entry, the module's did not
        out.backward(g.view(out.shape))
        e_out = (out.detach().reshape(n, -1).double().cpu() - ref_out).abs().max().item()
        e_dx = (xv.grad.double().cpu() - ref_dx).abs().max().item()
        e_p = [(p.grad.double().cpu() - r).abs().max().item() for p, r in zip(params, ref_p)]
        print(f'swish_mlp {form} {which}: out err {e_out:.3e}, dx err {e_dx:.3e} (bar {bar_dx:.3e}), parameters ' + ', '.join(f'{e:.2e}/{b:.2e}' for e, b in zip(e_p, bar_p)))
        assert e_out <= 1e-5 and e_dx <= bar_dx, (which, e_out, e_dx, bar_dx)
        for i, (e, b) in enumerate(zip(e_p, bar_p)):
            assert e <= b, (which, i, e, b)
        results[which] = out.detach()
    assert (results['kernels'] - results['module']).abs().max().item() <= 2e-5


def test_swish_mlp_returns_none_where_the_kernels_do_not_apply(mp, shared, monkeypatch):
    from msmp_pde_amd.mlp import swish_mlp
    form = TWO_LAYER[5]
    s = shared(form)
    seq = make_seq(mp, form, 32)
    x = s.x[:33].cuda()
    assert swish_mlp(seq, x) is not None                                        # the parameters require grad
    with torch.no_grad():
        assert swish_mlp(seq, x) is None
    with tuned(mp.lib(), mlp_train=0):
        assert swish_mlp(seq, x) is None
    assert swish_mlp(make_seq(mp, form, 32).cpu(), x.cpu()) is None
    assert swish_mlp(make_seq(mp, form, 32).double(), x.double()) is None
    assert swish_mlp(seq, x.double()) is None
    assert swish_mlp(torch.nn.Sequential(seq[0], torch.nn.ReLU(), seq[2], seq[3]), x) is None       # another form
    for p in seq.parameters():
        p.requires_grad_(False)
    assert swish_mlp(seq, x) is None                                            # nothing requires grad
    # a frozen first layer and an input that is data: the call succeeds, the backward is given no dx and the frozen parameters get no gradient
    seq[2].weight.requires_grad_(True)
    seq[2].bias.requires_grad_(True)
    L = mp.lib()
    real, dx_args = L.msmp_mlp_train_bwd_f32, []

    def entry(*a):
        dx_args.append(a[11])
        return real(*a)
    monkeypatch.setattr(L, 'msmp_mlp_train_bwd_f32', entry)
    out = swish_mlp(seq, x)
    out.backward(s.g[:33].cuda())
    assert dx_args == [None]
    assert seq[0].weight.grad is None and seq[0].bias.grad is None and x.grad is None
    ref = autograd_of(x.cpu(), s.g[:33], [p.detach().cpu() for p in seq.parameters()], torch.float64)[2]
    assert (seq[2].weight.grad.double().cpu() - ref[2]).abs().max().item() <= 1e-4 * ref[2].abs().max().item() + 2e-5 * max(r.abs().max().item() for r in ref)


# ---- solvers ---------------------------------------------------------------------------------------------------------------------------
# class, experiment, calls of the forward (= of the backward) entry per iteration: embedding_mlp | lemoutput_mlp | + double_mlp | lstmoutput_mlp | width 164, + double_mlp of 2 heads
SOLVERS = [('MP_PDE_Solver', 'E2', 1), ('MP_PDE_SolverLEMLinGated', 'E2', 1), ('MP_PDE_Solver2DLEMLinGated', 'RPU', 2), ('MP_PDE_SolverLSTMLin', 'E2', 1),
           ('MP_PDE_Solver2DLEMLinGatedGLU', 'MSWG3', 2)]


@pytest.mark.parametrize('kind,exp,calls', SOLVERS)
def test_solver_gradients_match_float64_oracle(mp, monkeypatch, kind, exp, calls):
    """test_solver_gradients_match_float64_oracle of test_gpu_decoder_bwd.py with the MLPs on the HIP kernels; the entries are counted: the
    expected number of calls with the switch on, none with it at 0."""
    torch.manual_seed(2)
    case = synthetic_case(mp, exp, bsz=2, seed=4)
    model = getattr(mp, kind)(case.pde, time_window=25, eq_variables=case.eqv, hidden_layer=2).cuda()
    graph = case.graph.to('cuda')
    fwd, bwd = counted(mp, monkeypatch, 'msmp_mlp_train_fwd_f32'), counted(mp, monkeypatch, 'msmp_mlp_train_bwd_f32')
    with tuned(mp.lib(), mlp_train=0):
        model(graph).sum().backward()
        assert len(fwd) == 0 and len(bwd) == 0
    model.zero_grad(set_to_none=True)
    with tuned(mp.lib(), mlp_train=1):
        pred = model(graph)
        loss = torch.sqrt(((pred - graph.y.to(pred.dtype)) ** 2).sum())
        loss.backward()
    assert (len(fwd), len(bwd)) == (calls, calls), (kind, len(fwd), len(bwd))
    sd64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    out = OT.solver_forward(kind, sd64, case.graph_np(), case.pde, 25, case.eqv, 2, as_numpy=False)
    ref_loss = torch.sqrt(((out - torch.tensor(case.graph_np().y).double()) ** 2).sum())
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 1e-4 * ref_loss.item()
    scale = max(sd64[name].grad.abs().max().item() for name, _ in model.named_parameters())
    worst = 0.0
    lin_layers = 'Gated' in kind or 'Lin' in kind
    for name, p in model.named_parameters():
        gr, r = p.grad.double().cpu(), sd64[name].grad
        if lin_layers and name.endswith('update_net_2.0.bias'):        # analytically zero (feeds an InstanceNorm): an absolute bound
            assert (gr - r).abs().max().item() < 1e-4 * scale, (name, (gr - r).abs().max().item(), scale)
            continue
        rel = (gr - r).abs().max().item() / max(r.abs().max().item(), 1e-3 * scale)
        worst = max(worst, rel)
        assert rel < 2e-3, (name, rel)
    print(f'{kind}/{exp} mlp_train 1: loss {loss.item():.6f} (oracle {ref_loss.item():.6f}); worst relative gradient error {worst:.2e}')
    record_parity('mlp_train', f'{kind}/{exp}/solver', worst_rel=worst, bar=2e-3)


# ---- capture ---------------------------------------------------------------------------------------------------------------------------
def test_captured_training_step_follows_the_eager_trajectory(mp, monkeypatch):
    """train.CapturedTrainStep of MSMP-PDE2D (lemoutput_mlp and double_mlp on the kernels) at batch 2: bit-identical losses and parameters
    over 3 steps of changing batches with the switch on."""
    from msmp_pde_amd import train as T
    from msmp_pde_amd.synthetic import make_case
    bsz = 2
    c = make_case('RPU', bsz, seed=9, device='cuda', dtype=torch.float32)
    gs = []
    for i in range(3):
        steps = [40 + 7 * i + j for j in range(bsz)]
        data, labels = c.creator.create_data(c.u_super, steps)
        gs.append(c.creator.create_graph(data, labels, c.x, c.variables, steps))
    fwd = counted(mp, monkeypatch, 'msmp_mlp_train_fwd_f32')

    def run_steps(captured):
        torch.manual_seed(11)
        model = mp.MODEL_NAMES['MSMP-PDE2D'](c.pde, time_window=25, eq_variables=c.eqv, hidden_layer=2).cuda()
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

    with tuned(mp.lib(), mlp_train=1):
        le, we = run_steps(False)
        assert len(fwd) >= 2 * 3                                        # both MLPs, every eager step
        lc, wc = run_steps(True)
    assert all(torch.isfinite(l) for l in lc) and float(lc[-1]) != float(lc[0])
    for i in range(3):
        assert torch.equal(le[i], lc[i]), (i, float(le[i]), float(lc[i]))
    for a, b in zip(we, wc):
        assert torch.equal(a, b)
