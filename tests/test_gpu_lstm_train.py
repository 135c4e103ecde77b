"""GPU tests of the LSTM kernels (lstm_train_kernel.hip: msmp_lstm_train_fwd_f32 / msmp_lstm_train_bwd_f32, every width 1 .. 256) and of their host
route (lstm._LSTMTrainFunction, solvers.LSTM.forward): parity with torch.nn.LSTM in float64 on the CPU under autograd at the bars of the same
arithmetic in test_gpu_lem_wide_train.py (1e-5 absolute on h_T, 1e-5 max(1, max|c_T|) on c_T, which is not bounded by 1, and 1e-4 of the largest
entry of each gradient tensor), bitwise properties, memory discipline, the absence of an input range, argument errors, the host routes, two
solver classes against the float64 oracle, and hipGraph capture.  Every test sets the switch "lstm_train" itself."""
import copy

import pytest
import torch

from oracle import msmp_oracle_torch as OT
from helpers import synthetic_case, counted, tuned

pytestmark = pytest.mark.gpu
TW = 25
WIDTHS = [33, 128, 129, 164, 256]       # one live channel in the last tile | the classes' width: exact tiles, one 128-block | one live column in the second 128-block | a pad inside a tile | the maximum
SHAPES = [(1, 1, 1), (5, 2, 33), (8, 25, 97), (4, 50, 64)]      # (ninp, T, n)


@pytest.fixture(scope='module')
def mp():
    import msmp_pde_amd
    assert torch.cuda.is_available()
    msmp_pde_amd.lib()
    return msmp_pde_amd


@pytest.fixture(autouse=True)
def switch_on(mp):
    L = mp.lib()
    shipped = L.msmp_tune_query(b'lstm_train')
    L.msmp_tune(b'lstm_train', 1)
    yield
    L.msmp_tune(b'lstm_train', shipped)


def _module(mp, ninp, width, seed):
    """(the module on the GPU, its deep copy as .double().cpu(): the reference)"""
    from msmp_pde_amd.solvers import LSTM
    torch.manual_seed(seed)
    m = LSTM(ninp, width).cuda()
    return m, copy.deepcopy(m).double().cpu()


def _params(m):
    r = m.rnn
    return [r.weight_ih_l0, r.weight_hh_l0, r.bias_ih_l0, r.bias_hh_l0]


def _apply(m, xin, states=None):
    from msmp_pde_amd.lstm import _LSTMTrainFunction
    return _LSTMTrainFunction.apply(m._blob(), xin, *_params(m), *(states or (None, None)))


def _grads(m):
    return [p.grad.clone() for p in _params(m)]


def _reference(ref, xin, states):
    """torch.nn.LSTM in float64 on the CPU: (h_T, c_T) from node-major xin and the same states"""
    x = xin.double().cpu().permute(1, 0, 2).contiguous()
    s64 = None if states is None else tuple(s.double().cpu()[None] for s in states)
    out, (_h, c) = ref.rnn(x) if s64 is None else ref.rnn(x, s64)
    return out[-1], c[0]


def _raw(mp, m, xin, states=None, gout=None, save=True, out=None):
    """The two entries called directly: (h_T, c_T, saved, dG); `out` = (h, c, saved, dg) buffers to write into instead of fresh ones."""
    from msmp_pde_amd.lem import _padded_inputs
    from msmp_pde_amd._lib import check, ptr, current_stream
    L = mp.lib()
    x = _padded_inputs(xin)
    n, t_len, ninp = xin.shape
    W = m.nhid
    h0, c0 = (None, None) if states is None else (s.contiguous() for s in states)
    h, c, saved, dg = out or (None, None, None, None)
    h = torch.empty(n, W, device='cuda') if h is None else h
    c = torch.empty(n, W, device='cuda') if c is None else c
    if save and saved is None:
        saved = torch.empty(L.msmp_lstm_saved_floats(n, t_len, W), device='cuda')
    check(L.msmp_lstm_train_fwd_f32(ptr(x), n, t_len, ninp, W, ptr(m._blob()), ptr(h0), ptr(c0), ptr(saved if save else None), ptr(h), ptr(c),
                                    current_stream()), 'fwd')
    if gout is None:
        return h, c, saved, None
    blob = torch.empty(L.msmp_packed_lstm_bwd_floats(ninp, W), device='cuda')
    check(L.msmp_pack_lstm_bwd_f32(ptr(m.rnn.weight_hh_l0.detach().contiguous()), ninp, W, ptr(blob), current_stream()), 'pack bwd')
    dg = torch.empty(L.msmp_lstm_dg_floats(n, t_len, W), device='cuda') if dg is None else dg
    check(L.msmp_lstm_train_bwd_f32(ptr(gout.contiguous()), ptr(saved), ptr(c0), n, t_len, W, ptr(blob), ptr(dg), current_stream()), 'bwd')
    return h, c, saved, dg


def _check_against_float64(m, ref, xin, states, w_out, h, c, what):
    """h_T within 1e-5, c_T within 1e-5 max(1, max|c_T|), every parameter gradient within 1e-4 of its largest entry; prints the figures"""
    h64, c64 = _reference(ref, xin, states)
    for p in ref.parameters():
        p.grad = None
    (h64 * w_out.double().cpu()).sum().backward()
    eh, ec = (h.double().cpu() - h64).abs().max().item(), (c.double().cpu() - c64).abs().max().item()
    c_scale = max(1.0, c64.abs().max().item())
    errs = [((p.grad.double().cpu() - q.grad).abs().max().item(), q.grad.abs().max().item()) for p, q in zip(_params(m), _params(ref))]
    print(f'{what}: state err {eh:.2e} / {ec:.2e} (max|c| {c_scale:.2f}), gradient errors / largest entry {["%.1e / %.1e" % e for e in errs]}')
    assert eh < 1e-5 and ec < 1e-5 * c_scale, (what, eh, ec, c_scale)
    for (k, _), (err, largest) in zip(m.named_parameters(), errs):
        assert err <= 1e-4 * largest, (what, k, err, largest)       # a gradient that is exactly zero (d weight_hh of one step from zero states) must be exactly zero


@pytest.mark.parametrize('with_states', [False, True], ids=['zeros', 'states'])
@pytest.mark.parametrize('ninp,t_len,n', SHAPES)
@pytest.mark.parametrize('width', WIDTHS)
def test_parity_with_float64_torch_lstm(mp, width, ninp, t_len, n, with_states):
    m, ref = _module(mp, ninp, width, 11 + ninp + width)
    xin = torch.randn(n, t_len, ninp, device='cuda') * 0.7
    w_out = torch.randn(n, width, device='cuda')
    states = (torch.rand(n, width, device='cuda') * 2 - 1, torch.rand(n, width, device='cuda') * 2 - 1) if with_states else None
    h, c = _apply(m, xin, states)
    (h * w_out).sum().backward()
    _check_against_float64(m, ref, xin, states, w_out, h, c, f'W={width} ninp={ninp} T={t_len} N={n} states={with_states}')


def test_bitwise_properties(mp):
    """Two runs are equal (outputs, saved planes, dG, gradients); a node's row depends on nothing but itself (the first 33 rows of a
    97-node call are a 33-node call); saved = NULL gives the same states; 25 steps are 10 + 15 steps with the carried (h, c)."""
    width, ninp, t_len, n = 164, 6, 25, 97
    m, _ = _module(mp, ninp, width, 21)
    xin = torch.randn(n, t_len, ninp, device='cuda') * 0.7
    gout = torch.randn(n, width, device='cuda')
    states = (torch.rand(n, width, device='cuda') * 2 - 1, torch.rand(n, width, device='cuda') * 2 - 1)
    a = _raw(mp, m, xin, states, gout)
    b = _raw(mp, m, xin, states, gout)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    grads = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        h, c = _apply(m, xin, states)
        (h * gout).sum().backward()
        assert torch.equal(h, a[0]) and torch.equal(c, a[1])
        grads.append(_grads(m))
    assert all(torch.equal(p, q) for p, q in zip(*grads))
    # rows
    s33 = tuple(s[:33] for s in states)
    r = _raw(mp, m, xin[:33], s33, gout[:33])
    wp, ldg = 192, 256
    assert torch.equal(r[0], a[0][:33]) and torch.equal(r[1], a[1][:33])
    assert torch.equal(r[2].view(6, 33, t_len, wp), a[2].view(6, n, t_len, wp)[:, :33])
    assert torch.equal(r[3].view(33, t_len, 4 * ldg), a[3].view(n, t_len, 4 * ldg)[:33])
    # saved = NULL
    d = _raw(mp, m, xin, states, save=False)
    assert torch.equal(d[0], a[0]) and torch.equal(d[1], a[1])
    # 25 = 10 + 15
    e = _raw(mp, m, xin[:, :10].contiguous(), states, save=False)
    f = _raw(mp, m, xin[:, 10:].contiguous(), (e[0], e[1]), save=False)
    assert torch.equal(f[0], a[0]) and torch.equal(f[1], a[1])


def test_memory_discipline(mp):
    """h / c outputs, the saved planes and dG of n = 97, W = 164, T = 3 placed inside larger poisoned buffers: nothing outside them is written,
    every element inside is (no poison value survives), columns 164 .. 255 of every gate of dG are exactly zero, every live column of every
    gate is nonzero somewhere, and the pad channels of the c and h planes are exact zeros."""
    width, ninp, t_len, n, wp, ldg, pad = 164, 5, 3, 97, 192, 256, 512
    poison = -7.25e30
    m, _ = _module(mp, ninp, width, 31)
    L = mp.lib()
    xin = torch.randn(n, t_len, ninp, device='cuda')
    gout = torch.randn(n, width, device='cuda')
    sizes = [n * width, n * width, L.msmp_lstm_saved_floats(n, t_len, width), L.msmp_lstm_dg_floats(n, t_len, width)]
    assert sizes[2] == 6 * n * t_len * wp and sizes[3] == 4 * n * t_len * ldg
    big = [torch.full((s + 2 * pad,), poison, device='cuda') for s in sizes]
    inner = [b[pad:pad + s] for b, s in zip(big, sizes)]
    h, c, saved, dg = _raw(mp, m, xin, None, gout, out=(inner[0].view(n, width), inner[1].view(n, width), inner[2], inner[3]))
    torch.cuda.synchronize()
    for b, s in zip(big, sizes):
        assert bool((b[:pad] == poison).all()) and bool((b[pad + s:] == poison).all())
        assert not bool((b[pad:pad + s] == poison).any())
    dg4 = dg.view(n * t_len, 4, ldg)
    assert bool((dg4[:, :, width:] == 0).all())
    assert bool((dg4[:, :, :width] != 0).any(dim=0).all())        # every live column of every gate carries a gradient
    sv = saved.view(6, n * t_len, wp)
    assert bool((sv[[4, 5]][:, :, width:] == 0).all())            # pad channels of c_t and h_{t-1} are exact zeros
    ref = _raw(mp, m, xin, None, gout)
    assert all(torch.equal(p, q) for p, q in zip((h, c, saved, dg), ref))


def test_no_input_range(mp):
    """Step inputs of magnitude up to 1000: the states match float64 to 1e-5 of the largest state entry and the range status stays clear."""
    width, ninp, t_len, n = 164, 4, 6, 70
    m, ref = _module(mp, ninp, width, 41)
    xin = (torch.rand(n, t_len, ninp, device='cuda') * 2 - 1) * 1000.0
    mp.last_status(reset=True)
    h, c = _apply(m, xin)
    h64, c64 = _reference(ref, xin, None)
    torch.cuda.synchronize()
    scale = max(h64.abs().max().item(), c64.abs().max().item())
    eh, ec = (h.double().cpu() - h64).abs().max().item(), (c.double().cpu() - c64).abs().max().item()
    print(f'|x| <= 1000: errors {eh:.2e} / {ec:.2e}, largest state entry {scale:.3f}')
    assert eh < 1e-5 * scale and ec < 1e-5 * scale
    assert mp.last_status() == 0


def test_argument_errors_on_the_device_path(mp):
    from msmp_pde_amd._lib import ptr, current_stream
    L = mp.lib()
    m, _ = _module(mp, 4, 164, 51)
    n, t_len = 40, 3
    x = torch.randn(n, t_len, 4, device='cuda')
    blob = m._blob()
    h, c, s0 = (torch.zeros(n, 164, device='cuda') for _ in range(3))
    saved = torch.zeros(L.msmp_lstm_saved_floats(n, t_len, 164), device='cuda')
    dg = torch.zeros(L.msmp_lstm_dg_floats(n, t_len, 164), device='cuda')
    bblob = torch.zeros(L.msmp_packed_lstm_bwd_floats(4, 164), device='cuda')
    st = current_stream()
    fwd = lambda **k: L.msmp_lstm_train_fwd_f32(*[k.get(key, default) for key, default in (
        ('x', ptr(x)), ('n', n), ('t', t_len), ('ninp', 4), ('width', 164), ('blob', ptr(blob)), ('h0', None), ('c0', None), ('saved', ptr(saved)),
        ('h', ptr(h)), ('c', ptr(c)))], st)
    bwd = lambda **k: L.msmp_lstm_train_bwd_f32(*[k.get(key, default) for key, default in (
        ('g', ptr(h)), ('saved', ptr(saved)), ('c0', None), ('n', n), ('t', t_len), ('width', 164), ('blob', ptr(bblob)), ('dg', ptr(dg)))], st)
    assert fwd() == 0 and fwd(n=0) == 0 and fwd(c=None) == 0 and fwd(saved=None) == 0
    assert fwd(width=0) == -2 and fwd(width=257) == -2 and fwd(ninp=0) == -2 and fwd(ninp=9) == -2
    assert fwd(t=0) == -1 and fwd(x=None) == -1 and fwd(blob=None) == -1 and fwd(h=None) == -1 and fwd(n=-1) == -1
    assert fwd(h0=ptr(s0)) == -1 and fwd(c0=ptr(s0)) == -1 and b'both' in L.msmp_last_error()
    assert fwd(saved=ptr(saved) + 4) == -1 and b'aligned' in L.msmp_last_error()
    assert bwd() == 0 and bwd(n=0) == 0 and bwd(c0=ptr(s0)) == 0
    assert bwd(width=0) == -2 and bwd(width=257) == -2
    assert bwd(t=0) == -1 and bwd(g=None) == -1 and bwd(saved=None) == -1 and bwd(blob=None) == -1 and bwd(dg=None) == -1
    assert bwd(dg=ptr(dg) + 8) == -1 and b'aligned' in L.msmp_last_error()
    assert L.msmp_pack_lstm_train_f32(ptr(x), ptr(x), ptr(x), ptr(x), 4, 164, None, st) == -1
    assert L.msmp_pack_lstm_bwd_f32(None, 4, 164, ptr(dg), st) == -1
    torch.cuda.synchronize()


def test_host_routes(mp, monkeypatch):
    """solvers.LSTM.forward: under grad the forward is reached once with `saved` and the backward once; both input layouts give the same bits;
    no_grad and frozen parameters take the forward with saved = NULL, never the backward, and give the bits of the grad forward; a float64
    module, CPU tensors, inputs that require grad and the switch at 0 reach neither entry, and the switch at 0 is self.rnn(...) bit for bit;
    the state_dict keys are the reference's."""
    width, ninp, t_len, n = 128, 6, 7, 77
    L = mp.lib()
    m, ref = _module(mp, ninp, width, 61)
    assert list(m.state_dict().keys()) == ['rnn.weight_ih_l0', 'rnn.weight_hh_l0', 'rnn.bias_ih_l0', 'rnn.bias_hh_l0']
    xin = torch.randn(n, t_len, ninp, device='cuda') * 0.7
    w_out = torch.randn(n, width, device='cuda')
    real, saved_args = L.msmp_lstm_train_fwd_f32, []

    def fwd(*a):          # (xin, n, t_len, ninp, width, packed, h0, c0, saved, h_out, c_out, stream)
        saved_args.append(a[8])
        return real(*a)
    monkeypatch.setattr(L, 'msmp_lstm_train_fwd_f32', fwd)
    calls_b = counted(mp, monkeypatch, 'msmp_lstm_train_bwd_f32')

    h = m.forward_nodes(xin)
    (h * w_out).sum().backward()
    g = _grads(m)
    assert len(saved_args) == 1 and saved_args[0] is not None and len(calls_b) == 1
    m.zero_grad(set_to_none=True)
    h2 = m(xin.permute(1, 0, 2).contiguous())
    (h2 * w_out).sum().backward()
    assert torch.equal(h, h2) and all(torch.equal(a, b) for a, b in zip(g, _grads(m)))
    assert len(saved_args) == 2 and saved_args[1] is not None and len(calls_b) == 2

    # given states, against float64
    states = (torch.rand(n, width, device='cuda') * 2 - 1, torch.rand(n, width, device='cuda') * 2 - 1)
    m.zero_grad(set_to_none=True)
    hs = m.forward_nodes(xin, states)
    (hs * w_out).sum().backward()
    h64, _c = _reference(ref, xin, states)
    assert (hs.double().cpu() - h64).abs().max().item() < 1e-5 and not torch.equal(hs, h)
    assert len(saved_args) == 3 and len(calls_b) == 3

    # no backward follows: saved = NULL, the same bits
    with torch.no_grad():
        h_ng = m.forward_nodes(xin)
        h_ng2 = m(xin.permute(1, 0, 2))
    for p in m.parameters():
        p.requires_grad_(False)
    h_frozen = m.forward_nodes(xin)
    for p in m.parameters():
        p.requires_grad_(True)
    assert saved_args[3:] == [None] * 3 and len(calls_b) == 3
    assert torch.equal(h_ng, h) and torch.equal(h_ng2, h) and torch.equal(h_frozen, h) and not h_frozen.requires_grad

    # routes that must not reach the entries
    n_f = len(saved_args)
    x_tn = xin.permute(1, 0, 2).contiguous()
    h64 = ref.forward_nodes(xin.double().cpu())                                 # float64 and CPU
    assert h64.dtype == torch.float64 and torch.equal(h64, ref.rnn(x_tn.double().cpu())[0][-1])
    m_cpu = copy.deepcopy(m).cpu()                                              # fp32 on the CPU
    assert torch.equal(m_cpu.forward_nodes(xin.cpu()), m_cpu.rnn(x_tn.cpu())[0][-1])
    xg = xin.clone().requires_grad_(True)                                       # inputs that require grad
    hg = m.forward_nodes(xg)
    (hg * w_out).sum().backward()
    assert xg.grad is not None and (hg - h).abs().max().item() < 1e-5
    with tuned(L, lstm_train=0):
        m.zero_grad(set_to_none=True)
        h0 = m.forward_nodes(xin)
        (h0 * w_out).sum().backward()
        g0 = _grads(m)
        m.zero_grad(set_to_none=True)
        hr = m.rnn(x_tn)[0][-1]
        assert torch.equal(h0, hr)
        with torch.no_grad():
            assert torch.equal(m(x_tn), m.rnn(x_tn)[0][-1])
    assert len(saved_args) == n_f and len(calls_b) == 3
    assert (h0 - h).abs().max().item() < 1e-5
    for a, b in zip(g, g0):          # and both routes agree as closely as each agrees with float64
        assert (a - b).abs().max().item() < 2e-4 * b.abs().max().item()
    with tuned(L, lstm_train=5):     # any value other than 0 selects the kernels
        m.forward_nodes(xin)
    assert len(saved_args) == n_f + 1


@pytest.mark.parametrize('kind,exp', [('MP_PDE_SolverLSTMLinGated', 'E2'), ('MP_PDE_Solver2DLSTMLin', 'RPU')])
def test_solver_gradients_match_float64_oracle(mp, monkeypatch, kind, exp):
    """test_gradients_match_float64_oracle of test_gpu_training.py with the encoder on the new kernels (same loss, same bars and scale rule), and
    the encoder's gradients with the switch at 1 and at 0 within 1e-4 of their largest entry."""
    L = mp.lib()
    torch.manual_seed(2)
    case = synthetic_case(mp, exp, bsz=3, seed=4)
    model = getattr(mp, kind)(case.pde, time_window=TW, eq_variables=case.eqv, hidden_layer=2).cuda()
    graph = case.graph.to('cuda')

    def run():
        model.zero_grad(set_to_none=True)
        pred = model(graph)
        loss = torch.sqrt(((pred - graph.y.to(pred.dtype)) ** 2).sum())
        loss.backward()
        return loss, {k: p.grad.clone() for k, p in model.named_parameters()}
    calls = counted(mp, monkeypatch, 'msmp_lstm_train_bwd_f32')
    loss, grads = run()
    assert len(calls) == 1
    with tuned(L, lstm_train=0):
        _, grads0 = run()
    assert len(calls) == 1

    sd64 = {k: v.detach().cpu().double().requires_grad_(True) for k, v in model.state_dict().items()}
    out = OT.solver_forward(kind, sd64, case.graph_np(), case.pde, TW, case.eqv, 2, as_numpy=False)
    y = torch.tensor(case.graph_np().y).double()
    ref_loss = torch.sqrt(((out - y) ** 2).sum())
    ref_loss.backward()
    assert abs(loss.item() - ref_loss.item()) < 1e-4 * ref_loss.item()
    scale = max(sd64[name].grad.abs().max().item() for name, _ in model.named_parameters())
    worst = 0.0
    for name, _ in model.named_parameters():
        g, r = grads[name].double().cpu(), sd64[name].grad
        if name.endswith('update_net_2.0.bias'):      # analytically zero (GNN_LayerLin feeds its InstanceNorm directly): an absolute bound
            assert (g - r).abs().max().item() < 1e-4 * scale, (name, (g - r).abs().max().item(), scale)
            continue
        rel = (g - r).abs().max().item() / max(r.abs().max().item(), 1e-3 * scale)
        worst = max(worst, rel)
        assert rel < 2e-3, (name, rel)
    emb = [k for k in grads if k.startswith('embedding_lstm.')]
    assert len(emb) == 4
    for k in emb:
        d = (grads[k] - grads0[k]).abs().max().item() / grads0[k].abs().max().item()
        print(f'{kind} {k}: switch 1 vs 0 {d:.2e}')
        assert d < 1e-4, (k, d)
    print(f'{kind}/{exp}: loss {loss.item():.6f} (oracle {ref_loss.item():.6f}); worst relative gradient error {worst:.2e}')


def test_capture(mp):
    """LSTM(6, 128) forward + backward captured with torch.cuda.graph after a warm-up on a side stream and replayed twice: the gradients are
    bitwise those of the eager call (the Function allocates through torch only and never synchronises)."""
    m, _ = _module(mp, 6, 128, 71)
    n, t_len = 97, 25
    xin = torch.randn(n, t_len, 6, device='cuda') * 0.7
    w_out = torch.randn(n, 128, device='cuda')

    def step():
        h = m.forward_nodes(xin)
        (h * w_out).sum().backward()
        return h
    h_eager = step().detach().clone()
    eager = _grads(m)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            m.zero_grad(set_to_none=True)
            step()
    torch.cuda.current_stream().wait_stream(side)
    m.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        h_static = step()
    static = [p.grad for p in _params(m)]
    for _ in range(2):
        for g in static:
            g.fill_(float('nan'))
        h_static.detach().fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(h_static, h_eager)
        assert all(torch.equal(a, b) for a, b in zip(static, eager))


def test_captured_training_step_follows_the_eager_trajectory(mp):
    """train.CapturedTrainStep on 'LSTMGated' / E2 at batch 4 for 3 steps, in the manner of the test of that name in test_gpu_training.py:
    bit-identical losses, interleaved eager predictions and parameters, and two captured runs agree bit for bit."""
    from msmp_pde_amd import train as T
    from msmp_pde_amd.synthetic import make_case
    bsz = 4
    c = make_case('E2', bsz, seed=9, device='cuda', dtype=torch.float32)

    def batches(k):
        out = []
        for i in range(k):
            steps = [40 + 7 * i + (j % 5) for j in range(bsz)]
            data, labels = c.creator.create_data(c.u_super, steps)
            out.append(c.creator.create_graph(data, labels, c.x, c.variables, steps))
        return out
    gs = batches(3)

    def run(captured):
        torch.manual_seed(11)
        model = mp.MODEL_NAMES['LSTMGated'](c.pde, time_window=TW, eq_variables=c.eqv, hidden_layer=3).cuda()
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
            with torch.no_grad():                      # eager work between the replays, reading the freshly updated weights
                preds.append(model(gs[(i + 1) % len(gs)]).clone())
        torch.cuda.synchronize()
        return losses, preds, [p.detach().clone() for p in model.parameters()]

    le, pe, we = run(False)
    lc, pc, wc = run(True)
    lc2, pc2, wc2 = run(True)
    print('LSTMGated losses', [round(float(l), 5) for l in lc])
    assert all(torch.isfinite(l) for l in lc) and float(lc[-1]) != float(lc[0])
    for i in range(len(le)):
        assert torch.equal(le[i], lc[i]), (i, float(le[i]), float(lc[i]))
        assert torch.equal(pe[i], pc[i]), i
    for a, b, b2 in zip(we, wc, wc2):
        assert torch.equal(a, b) and torch.equal(b, b2)
    assert all(torch.equal(a, b) for a, b in zip(lc, lc2))
