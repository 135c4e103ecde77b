"""GPU tests of the LEM TRAINING pair (lem_wide_train_kernel.hip: msmp_lem_train_fwd_wide_f32 / msmp_lem_train_bwd_wide_f32, every width 1 .. 256) and
of its host route (lem._LEMTrainFunction, lem.LEM._recurrence): parity with the float64 restatement of the cell (LEMcuda.forward) at the bars of
test_lem_training_kernels_match_float64_restatement (1e-5 absolute on the states, 1e-4 of the largest entry of each gradient tensor), the bits
of the retired 128-wide pair at width 128, bitwise properties, memory discipline, the absence of an input range, argument errors, the host
routes, two solver classes against the float64 oracle, and hipGraph capture.  Every test sets the switch "lem_wide_train" itself."""
import copy
import ctypes
import os

import numpy as np

import pytest
import torch

from oracle import msmp_oracle_torch as OT
from helpers import synthetic_case, counted, tuned

pytestmark = pytest.mark.gpu
TW = 25
WIDTHS = [33, 128, 129, 164, 192, 256]       # one live channel in the last tile | the flagship width: exact tiles, one 128-block | one live column in the second 128-block | a pad inside a tile | exact tiles, ldg > Wp | the maximum
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
    shipped = L.msmp_tune_query(b'lem_wide_train')
    L.msmp_tune(b'lem_wide_train', 1)
    yield
    L.msmp_tune(b'lem_wide_train', shipped)


def _module(mp, ninp, width, seed, cls=None):
    from msmp_pde_amd.lem import LEM
    torch.manual_seed(seed)
    lem = (cls or LEM)(ninp, width).cuda()
    return lem, copy.deepcopy(lem).double()


def _apply(lem, xin, states=None):
    from msmp_pde_amd.lem import _LEMTrainFunction
    r = lem.rnn
    return _LEMTrainFunction.apply(r, xin, r.weights, r.weights_lin_z, r.bias, r.bias_lin_z, *(states or (None, None)))


def _grads(lem):
    return [p.grad.clone() for p in lem.parameters()]


def _raw(mp, rnn, xin, states=None, gout=None, save=True, out=None):
    """The two entries called directly: (y_T, z_T, saved, dG); `out` = (y, z, saved, dg) buffers to write into instead of fresh ones."""
    from msmp_pde_amd.lem import _padded_inputs
    from msmp_pde_amd._lib import check, ptr, current_stream
    L = mp.lib()
    x = _padded_inputs(xin)
    n, t_len, _ = xin.shape
    W, ninp = rnn.nhid, rnn.ninp
    y0, z0 = (None, None) if states is None else (s.contiguous() for s in states)
    y, z, saved, dg = out or (None, None, None, None)
    y = torch.empty(n, W, device='cuda') if y is None else y
    z = torch.empty(n, W, device='cuda') if z is None else z
    if save and saved is None:
        saved = torch.empty(L.msmp_lem_wide_saved_floats(n, t_len, W), device='cuda')
    check(L.msmp_lem_train_fwd_wide_f32(ptr(x), n, t_len, ninp, W, rnn.dt, ptr(rnn._pack_wide_train()), ptr(y0), ptr(z0), ptr(saved if save else None),
                                        ptr(y), ptr(z), current_stream()), 'fwd')
    if gout is None:
        return y, z, saved, None
    blob = torch.empty(L.msmp_packed_lem_wide_bwd_floats(ninp, W), device='cuda')
    w, wz = rnn.weights.detach().contiguous(), rnn.weights_lin_z.detach().contiguous()
    check(L.msmp_pack_lem_wide_bwd_f32(ptr(w), ptr(wz), ninp, W, ptr(blob), current_stream()), 'pack bwd')
    dg = torch.empty(L.msmp_lem_wide_dg_floats(n, t_len, W), device='cuda') if dg is None else dg
    check(L.msmp_lem_train_bwd_wide_f32(ptr(gout.contiguous()), ptr(saved), ptr(y0), ptr(z0), n, t_len, W, rnn.dt, ptr(blob), ptr(dg), current_stream()), 'bwd')
    return y, z, saved, dg


def _check_against_float64(lem, ref, xin, states, w_out, y, z, what):
    """final states within 1e-5, every parameter gradient within 1e-4 of its largest entry; returns the figures"""
    s64 = None if states is None else tuple(s.double() for s in states)
    y64, z64 = ref.rnn(xin.double().permute(1, 0, 2).contiguous(), s64, return_state=True)
    for p in ref.parameters():
        p.grad = None
    (y64 * w_out.double()).sum().backward()
    ey, ez = (y.double() - y64).abs().max().item(), (z.double() - z64).abs().max().item()
    rels = [(p.grad.double() - q.grad).abs().max().item() / q.grad.abs().max().item() for p, q in zip(lem.parameters(), ref.parameters())]
    print(f'{what}: state err {ey:.2e} / {ez:.2e}, gradient errors {["%.1e" % r for r in rels]}')
    assert ey < 1e-5 and ez < 1e-5, (what, ey, ez)
    for (k, _), rel in zip(lem.named_parameters(), rels):
        assert rel < 1e-4, (what, k, rel)


@pytest.mark.parametrize('with_states', [False, True], ids=['zeros', 'states'])
@pytest.mark.parametrize('ninp,t_len,n', SHAPES)
@pytest.mark.parametrize('width', WIDTHS)
def test_parity_with_the_float64_restatement(mp, width, ninp, t_len, n, with_states):
    lem, ref = _module(mp, ninp, width, 11 + ninp + width)
    xin = torch.randn(n, t_len, ninp, device='cuda') * 0.7
    w_out = torch.randn(n, width, device='cuda')
    states = (torch.rand(n, width, device='cuda') * 2 - 1, torch.rand(n, width, device='cuda') * 2 - 1) if with_states else None
    y, z = _apply(lem, xin, states)
    (y * w_out).sum().backward()
    _check_against_float64(lem, ref, xin, states, w_out, y, z, f'W={width} ninp={ninp} T={t_len} N={n} states={with_states}')


def test_width_128_reproduces_the_retired_128_wide_pair(mp):
    """tests/golden/lem_train_128.npz was recorded on the parent of the commit that retired lem_train_kernel.hip, from ITS 128-wide pair
    (msmp_lem_train_fwd_f32 / msmp_lem_train_bwd_f32 under LEMS(5, 128).forward_nodes with given initial states, T = 2, N = 33): y_T, z_T,
    d bias, d bias_lin_z and rows 0 .. 7 of d weights and d weights_lin_z.  The surviving pair gives the same bits (torch.equal) through
    the same call.  The parameters (270 KB), the states and dL/dy do not fit the fixture: they are regenerated from its seed by the host
    generator, in the order of the recording, and each is pinned by its first row and its float64 sum; xin is stored whole."""
    from msmp_pde_amd.lem import LEMS
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lem_train_128.npz'))
    ninp, t_len, n = (int(v) for v in d['shape'])
    torch.manual_seed(int(d['seed']))
    lems = LEMS(ninp, 128)
    xin = torch.randn(n, t_len, ninp) * 0.7
    y0, z0 = torch.rand(n, 128) * 2 - 1, torch.rand(n, 128) * 2 - 1
    w_out = torch.randn(n, 128)
    for k, v in list(lems.state_dict().items()) + [('y0', y0), ('z0', z0), ('w_out', w_out)]:
        v = v.numpy()
        total, recorded = v.astype(np.float64).sum(), float(d['sum.' + k])       # the sum to 1e-9: it may be reduced in another order
        assert np.array_equal(v.reshape(v.shape[0], -1)[0], d['head.' + k]) and abs(total - recorded) <= 1e-9 * max(1.0, abs(recorded)), f'{k} is not what the fixture was recorded with'
    assert np.array_equal(xin.numpy(), d['xin'])
    lems = lems.cuda()
    lems.states = (y0.cuda(), z0.cuda())
    y = lems.forward_nodes(xin.cuda())
    (y * w_out.cuda()).sum().backward()
    g = {k: p.grad.cpu().numpy() for k, p in lems.named_parameters()}
    got = {'y_T': y.detach().cpu().numpy(), 'z_T': lems.states[1].cpu().numpy(), 'd_bias': g['rnn.bias'], 'd_bias_lin_z': g['rnn.bias_lin_z'],
           'd_weights_rows0_7': g['rnn.weights'][:8], 'd_weights_lin_z_rows0_7': g['rnn.weights_lin_z'][:8]}
    for k, v in got.items():
        assert torch.equal(torch.from_numpy(np.ascontiguousarray(v)), torch.from_numpy(d[k])), k


def test_routes_at_width_128(mp, monkeypatch):
    """lem.LEM._recurrence at the flagship width: LEM and LEMS under grad reach the forward (with `saved`) and the backward once each; LEM and
    LEMS under no_grad, and LEM with frozen parameters, reach the forward with saved = NULL (the same bits) and never the backward; the
    switch at 0 and TRAIN_KERNELS = False reach neither under grad and give the PyTorch restatement bit for bit."""
    from msmp_pde_amd.lem import LEM, LEMS
    L = mp.lib()
    ninp, t_len, n = 5, 2, 33
    lem, _ = _module(mp, ninp, 128, 81)
    lems, _ = _module(mp, ninp, 128, 82, cls=LEMS)
    xin = torch.randn(n, t_len, ninp, device='cuda') * 0.7
    w_out = torch.randn(n, 128, device='cuda')
    real, saved_args = L.msmp_lem_train_fwd_wide_f32, []

    def fwd(*a):          # (xin, n, t_len, ninp, width, dt, packed, y0, z0, saved, y_out, z_out, stream)
        saved_args.append(a[9])
        return real(*a)
    monkeypatch.setattr(L, 'msmp_lem_train_fwd_wide_f32', fwd)
    calls_b = counted(mp, monkeypatch, 'msmp_lem_train_bwd_wide_f32')

    y = lem.forward_nodes(xin)
    (y * w_out).sum().backward()
    assert len(saved_args) == 1 and saved_args[0] is not None and len(calls_b) == 1
    for k in range(2):
        states = lems.states
        yk = lems.forward_nodes(xin)
        (yk * w_out).sum().backward()
        assert (states is None) == (k == 0) and not lems.states[0].requires_grad
    assert len(saved_args) == 3 and all(s is not None for s in saved_args) and len(calls_b) == 3

    with torch.no_grad():
        y_ng = lem.forward_nodes(xin)
        lems.reset_states()
        ys_ng = [lems.forward_nodes(xin) for _ in range(2)]
    for p in lem.parameters():
        p.requires_grad_(False)
    y_frozen = lem.forward_nodes(xin)
    for p in lem.parameters():
        p.requires_grad_(True)
    assert saved_args[3:] == [None] * 4 and len(calls_b) == 3
    assert torch.equal(y_ng, y) and torch.equal(y_frozen, y) and not y_frozen.requires_grad
    lems.reset_states()
    assert torch.equal(lems.forward_nodes(xin), ys_ng[0]) and torch.equal(lems.forward_nodes(xin), ys_ng[1]) and not torch.equal(ys_ng[0], ys_ng[1])
    n_f, n_b = len(saved_args), len(calls_b)

    def restated(module, x):
        return module.rnn(x.permute(1, 0, 2).contiguous())
    with tuned(L, lem_wide_train=0):
        y0 = lem.forward_nodes(xin)
        assert y0.requires_grad and torch.equal(y0, restated(lem, xin))
        (y0 * w_out).sum().backward()
    monkeypatch.setattr(LEM, 'TRAIN_KERNELS', False)
    y1 = lem.forward_nodes(xin)
    assert y1.requires_grad and torch.equal(y1, restated(lem, xin))
    lems.reset_states()
    assert lems.forward_nodes(xin).requires_grad
    monkeypatch.setattr(LEM, 'TRAIN_KERNELS', True)
    assert len(saved_args) == n_f and len(calls_b) == n_b
    assert (y0 - y).abs().max().item() < 1e-5


def test_bitwise_properties(mp):
    """Two runs are equal (outputs, saved planes, dG, gradients); a node's row depends on nothing but itself (the first 33 rows of a
    97-node call are a 33-node call); saved = NULL gives the same states; 25 steps are 10 + 15 steps with the carried states."""
    width, ninp, t_len, n = 164, 6, 25, 97
    lem, _ = _module(mp, ninp, width, 21)
    xin = torch.randn(n, t_len, ninp, device='cuda') * 0.7
    gout = torch.randn(n, width, device='cuda')
    states = (torch.rand(n, width, device='cuda') * 2 - 1, torch.rand(n, width, device='cuda') * 2 - 1)
    a = _raw(mp, lem.rnn, xin, states, gout)
    b = _raw(mp, lem.rnn, xin, states, gout)
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    grads = []
    for _ in range(2):
        lem.zero_grad(set_to_none=True)
        y, _z = _apply(lem, xin, states)
        (y * gout).sum().backward()
        assert torch.equal(y, a[0]) and torch.equal(_z, a[1])
        grads.append(_grads(lem))
    assert all(torch.equal(p, q) for p, q in zip(*grads))
    # rows
    s33 = tuple(s[:33] for s in states)
    c = _raw(mp, lem.rnn, xin[:33], s33, gout[:33])
    wp, ldg = 192, 256
    assert torch.equal(c[0], a[0][:33]) and torch.equal(c[1], a[1][:33])
    assert torch.equal(c[2].view(6, 33, t_len, wp), a[2].view(6, n, t_len, wp)[:, :33])
    assert torch.equal(c[3].view(33, t_len, 4 * ldg), a[3].view(n, t_len, 4 * ldg)[:33])
    # saved = NULL
    d = _raw(mp, lem.rnn, xin, states, save=False)
    assert torch.equal(d[0], a[0]) and torch.equal(d[1], a[1])
    # 25 = 10 + 15
    e = _raw(mp, lem.rnn, xin[:, :10].contiguous(), states, save=False)
    f = _raw(mp, lem.rnn, xin[:, 10:].contiguous(), (e[0], e[1]), save=False)
    assert torch.equal(f[0], a[0]) and torch.equal(f[1], a[1])


def test_memory_discipline(mp):
    """y / z outputs, the saved planes and dG of n = 97, W = 164, T = 3 placed inside larger poisoned buffers: nothing outside them is written,
    every element inside is (no poison value survives), and columns 164 .. 255 of every gate of dG are exactly zero."""
    width, ninp, t_len, n, wp, ldg, pad = 164, 5, 3, 97, 192, 256, 512
    poison = -7.25e30
    lem, _ = _module(mp, ninp, width, 31)
    L = mp.lib()
    xin = torch.randn(n, t_len, ninp, device='cuda')
    gout = torch.randn(n, width, device='cuda')
    sizes = [n * width, n * width, L.msmp_lem_wide_saved_floats(n, t_len, width), L.msmp_lem_wide_dg_floats(n, t_len, width)]
    assert sizes[2] == 6 * n * t_len * wp and sizes[3] == 4 * n * t_len * ldg
    big = [torch.full((s + 2 * pad,), poison, device='cuda') for s in sizes]
    inner = [b[pad:pad + s] for b, s in zip(big, sizes)]
    y, z, saved, dg = _raw(mp, lem.rnn, xin, None, gout, out=(inner[0].view(n, width), inner[1].view(n, width), inner[2], inner[3]))
    torch.cuda.synchronize()
    for b, s in zip(big, sizes):
        assert bool((b[:pad] == poison).all()) and bool((b[pad + s:] == poison).all())
        assert not bool((b[pad:pad + s] == poison).any())
    dg4 = dg.view(n * t_len, 4, ldg)
    assert bool((dg4[:, :, width:] == 0).all())
    assert bool((dg4[:, :, :width] != 0).any(dim=0).all())        # every live column of every gate carries a gradient
    sv = saved.view(6, n * t_len, wp)
    assert bool((sv[[1, 3, 4, 5]][:, :, width:] == 0).all())      # pad channels of c, d, y, z' are exact zeros
    ref = _raw(mp, lem.rnn, xin, None, gout)
    assert all(torch.equal(p, q) for p, q in zip((y, z, saved, dg), ref))


def test_no_input_range(mp):
    """Step inputs of magnitude 1000 (the fp16-split inference kernel stops at 255): the states match float64 to 1e-5 of the largest state entry and
    the range status stays clear."""
    width, ninp, t_len, n = 164, 4, 6, 70
    lem, ref = _module(mp, ninp, width, 41)
    xin = (torch.rand(n, t_len, ninp, device='cuda') * 2 - 1) * 1000.0
    mp.last_status(reset=True)
    y, z = _apply(lem, xin)
    y64, z64 = ref.rnn(xin.double().permute(1, 0, 2).contiguous(), None, return_state=True)
    torch.cuda.synchronize()
    scale = max(y64.abs().max().item(), z64.abs().max().item())
    ey, ez = (y.double() - y64).abs().max().item(), (z.double() - z64).abs().max().item()
    print(f'|x| = 1000: errors {ey:.2e} / {ez:.2e}, largest state entry {scale:.3f}')
    assert ey < 1e-5 * scale and ez < 1e-5 * scale
    assert mp.last_status() == 0


def test_argument_errors_on_the_device_path(mp):
    from msmp_pde_amd._lib import ptr, current_stream
    L = mp.lib()
    lem, _ = _module(mp, 4, 164, 51)
    n, t_len = 40, 3
    x = torch.randn(n, t_len, 4, device='cuda')
    blob = lem.rnn._pack_wide_train()
    y, z, s0 = (torch.zeros(n, 164, device='cuda') for _ in range(3))
    saved = torch.zeros(L.msmp_lem_wide_saved_floats(n, t_len, 164), device='cuda')
    dg = torch.zeros(L.msmp_lem_wide_dg_floats(n, t_len, 164), device='cuda')
    st = current_stream()
    fwd = lambda **k: L.msmp_lem_train_fwd_wide_f32(*[k.get(key, default) for key, default in (
        ('x', ptr(x)), ('n', n), ('t', t_len), ('ninp', 4), ('width', 164), ('dt', 1.0), ('blob', ptr(blob)), ('y0', None), ('z0', None), ('saved', ptr(saved)),
        ('y', ptr(y)), ('z', ptr(z)))], st)
    bwd = lambda **k: L.msmp_lem_train_bwd_wide_f32(*[k.get(key, default) for key, default in (
        ('g', ptr(y)), ('saved', ptr(saved)), ('y0', None), ('z0', None), ('n', n), ('t', t_len), ('width', 164), ('dt', 1.0), ('blob', ptr(blob)), ('dg', ptr(dg)))], st)
    assert fwd() == 0 and fwd(n=0) == 0 and fwd(z=None) == 0 and fwd(saved=None) == 0
    assert fwd(width=0) == -2 and fwd(width=257) == -2 and fwd(ninp=0) == -2 and fwd(ninp=9) == -2
    assert fwd(t=0) == -1 and fwd(x=None) == -1 and fwd(blob=None) == -1 and fwd(y=None) == -1 and fwd(n=-1) == -1
    assert fwd(y0=ptr(s0)) == -1 and fwd(z0=ptr(s0)) == -1 and b'both' in L.msmp_last_error()
    assert fwd(saved=ptr(saved) + 4) == -1 and b'aligned' in L.msmp_last_error()
    assert bwd(n=0) == 0
    assert bwd(width=0) == -2 and bwd(width=257) == -2
    assert bwd(t=0) == -1 and bwd(dt=0.0) == -1 and bwd(g=None) == -1 and bwd(saved=None) == -1 and bwd(blob=None) == -1 and bwd(dg=None) == -1
    assert bwd(y0=ptr(s0)) == -1 and bwd(dg=ptr(dg) + 8) == -1
    assert L.msmp_pack_lem_wide_train_f32(ptr(x), ptr(x), ptr(x), ptr(x), 4, 164, None, st) == -1
    assert L.msmp_pack_lem_wide_bwd_f32(ptr(x), None, 4, 164, ptr(dg), st) == -1
    torch.cuda.synchronize()


def test_host_routes(mp, monkeypatch):
    """At width 164: both input layouts give the same bits; LEMS carries (y, z) over two calls; a float64 module, TRAIN_KERNELS = False, no_grad,
    frozen parameters and the switch at 0 do not reach the new entries, and the switch at 0 reproduces the PyTorch restatement bit for bit."""
    from msmp_pde_amd.lem import LEM, LEMS
    width, ninp, t_len, n = 164, 6, 7, 77
    L = mp.lib()
    lem, ref = _module(mp, ninp, width, 61)
    xin = torch.randn(n, t_len, ninp, device='cuda') * 0.7
    w_out = torch.randn(n, width, device='cuda')
    calls_f, calls_b = counted(mp, monkeypatch, 'msmp_lem_train_fwd_wide_f32'), counted(mp, monkeypatch, 'msmp_lem_train_bwd_wide_f32')
    y = lem.forward_nodes(xin)
    (y * w_out).sum().backward()
    g = _grads(lem)
    assert len(calls_f) == 1 and len(calls_b) == 1
    lem.zero_grad(set_to_none=True)
    y2 = lem(xin.permute(1, 0, 2).contiguous())
    (y2 * w_out).sum().backward()
    assert torch.equal(y, y2) and all(torch.equal(a, b) for a, b in zip(g, _grads(lem)))
    assert len(calls_f) == 2 and len(calls_b) == 2

    # LEMS: two consecutive calls, the second from the carried states, each against the restatement given the same states
    lems, refs = _module(mp, ninp, width, 62, cls=LEMS)
    xs = [torch.randn(n, 2, ninp, device='cuda') for _ in range(2)]
    for k in range(2):
        states = lems.states
        lems.zero_grad(set_to_none=True)
        yk = lems.forward_nodes(xs[k])
        (yk * w_out).sum().backward()
        assert (states is None) == (k == 0) and not lems.states[0].requires_grad and not lems.states[1].requires_grad
        _check_against_float64(lems, refs, xs[k], states, w_out, yk, lems.states[1], f'LEMS call {k}')
    assert len(calls_f) == 4 and len(calls_b) == 4

    # routes that must not reach the entries
    def restated(module, x):
        return module.rnn(x.permute(1, 0, 2).contiguous().to(module.rnn.weights.dtype))
    n_f = len(calls_f)
    y64 = ref.forward_nodes(xin.double())
    assert y64.dtype == torch.float64 and torch.equal(y64, restated(ref, xin.double()))
    monkeypatch.setattr(LEM, 'TRAIN_KERNELS', False)
    assert torch.equal(lem.forward_nodes(xin), restated(lem, xin))
    monkeypatch.setattr(LEM, 'TRAIN_KERNELS', True)
    with torch.no_grad():
        lem.forward_nodes(xin)
    for p in lem.parameters():
        p.requires_grad_(False)
    lem.forward_nodes(xin)
    for p in lem.parameters():
        p.requires_grad_(True)
    with tuned(L, lem_wide_train=0):
        lem.zero_grad(set_to_none=True)
        y0 = lem.forward_nodes(xin)
        (y0 * w_out).sum().backward()
        g0 = _grads(lem)
        lem.zero_grad(set_to_none=True)
        yr = restated(lem, xin)
        (yr * w_out).sum().backward()
        assert torch.equal(y0, yr) and all(torch.equal(a, b) for a, b in zip(g0, _grads(lem)))
    assert len(calls_f) == n_f and len(calls_b) == 4
    for a, b in zip(g, g0):          # and both routes agree as closely as each agrees with float64
        assert (a - b).abs().max().item() < 2e-4 * b.abs().max().item()
    with tuned(L, lem_wide_train=5):  # any value other than 0 selects the kernels
        lem.forward_nodes(xin)
    assert len(calls_f) == n_f + 1


@pytest.mark.parametrize('kind,exp', [('MP_PDE_SolverLEMLinGatedGLU', 'E2'), ('MP_PDE_Solver2DLEMLinGatedGLU', 'MSWG3')])
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
    calls = counted(mp, monkeypatch, 'msmp_lem_train_bwd_wide_f32')
    loss, grads = run()
    assert len(calls) == 1
    with tuned(L, lem_wide_train=0):
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
    emb = [k for k in grads if k.startswith('embedding_lem.')]
    assert len(emb) == 4
    for k in emb:
        d = (grads[k] - grads0[k]).abs().max().item() / grads0[k].abs().max().item()
        print(f'{kind} {k}: switch 1 vs 0 {d:.2e}')
        assert d < 1e-4, (k, d)
    print(f'{kind}/{exp}: loss {loss.item():.6f} (oracle {ref_loss.item():.6f}); worst relative gradient error {worst:.2e}')


def test_capture(mp):
    """LEM(6, 164) forward + backward captured with torch.cuda.graph after a warm-up on a side stream and replayed twice: the gradients are
    bitwise those of the eager call (the Function allocates through torch only and never synchronises)."""
    lem, _ = _module(mp, 6, 164, 71)
    n, t_len = 97, 25
    xin = torch.randn(n, t_len, 6, device='cuda') * 0.7
    w_out = torch.randn(n, 164, device='cuda')

    def step():
        y = lem.forward_nodes(xin)
        (y * w_out).sum().backward()
        return y
    y_eager = step().detach().clone()
    eager = _grads(lem)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            lem.zero_grad(set_to_none=True)
            step()
    torch.cuda.current_stream().wait_stream(side)
    lem.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y_static = step()
    static = [p.grad for p in lem.parameters()]
    for _ in range(2):
        for g in static:
            g.fill_(float('nan'))
        y_static.detach().fill_(float('nan'))
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(y_static, y_eager)
        assert all(torch.equal(a, b) for a, b in zip(static, eager))
