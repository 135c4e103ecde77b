"""GPU tests of the width-generic LEM recurrence (msmp_lem_encoder_wide_f32, lem_wide_kernel.hip): one launch for all T steps at any
hidden width up to 256, against the float64 cell (oracle.msmp_oracle.lem_forward: the restatement of experiments/models_gnn.py:285-342),
its bitwise properties (state carrying, node-count and run-to-run independence, nothing written outside [n, W]), the argument errors of
the C entry, and the host paths that reach it: LEMcuda / LEM / LEMS at width 164 and the two GLU solver classes.
Bar 5e-6 on y and z: the bar of test_lem_encoder_kernel for the 128-wide kernels (same arithmetic: fp16 2-way split, fp32 accumulate)."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import msmp_oracle as O
from helpers import synthetic_case
from helpers import mp, restore_wide_switches       # noqa: F401  (fixtures)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('restore_wide_switches')]

BAR = 5e-6
WIDTHS = [33, 96, 128, 164, 192, 256]
SHAPES = [(1, 1, 1), (5, 2, 33), (6, 25, 97), (8, 25, 300), (4, 50, 64)]       # (ninp, T, n)


def oracle_cell(rnn, xin, states=None):
    """float64 (y_T, z_T) of the cell for node-major xin [N, T, ninp]"""
    sd = {k: v.detach().double().cpu().numpy() for k, v in rnn.state_dict().items()}
    st = None if states is None else tuple(s.double().cpu().numpy() for s in states)
    return O.lem_forward(xin.permute(1, 0, 2).double().cpu().numpy(), sd['weights'], sd['weights_lin_z'], sd['bias'], sd['bias_lin_z'],
                         rnn.dt, states=st, return_state=True)


def err(a, ref):
    return float(np.abs(a.double().cpu().numpy() - ref).max())


@pytest.mark.parametrize('random_states', [False, True])
@pytest.mark.parametrize('ninp,t_len,n', SHAPES)
@pytest.mark.parametrize('width', WIDTHS)
def test_parity_against_the_float64_cell(mp, width, ninp, t_len, n, random_states):
    torch.manual_seed(1000 * width + 10 * ninp + int(random_states))
    rnn = mp.lem.LEMcuda(ninp, width, 1.0).cuda()
    xin = torch.randn(n, t_len, ninp, device='cuda')
    states = (torch.rand(n, width, device='cuda') * 2 - 1, torch.rand(n, width, device='cuda') * 2 - 1) if random_states else None
    ref_y, ref_z = oracle_cell(rnn, xin, states)
    with torch.no_grad():
        y, z = rnn.forward_wide(xin, states)
    e_y, e_z = err(y, ref_y), err(z, ref_z)
    print(f'wide W={width} ninp={ninp} T={t_len} n={n} states={random_states}: y {e_y:.2e} z {e_z:.2e}')
    assert y.shape == (n, width) and z.shape == (n, width)
    assert e_y < BAR and e_z < BAR
    if width == 128:        # the other kernels that serve width 128, on the same inputs: within the same bar of the same oracle
        lem = mp.LEM(ninp, 128).cuda()
        lem.rnn.load_state_dict(rnn.state_dict())
        with torch.no_grad():
            if states is None:
                e_old = err(lem.encode(xin, None), ref_y)                    # weight-stationary fused kernel (zero states)
            else:
                y_old, z_old = mp.lem._train_forward(lem.rnn, mp.lem._padded_inputs(xin), states[0].contiguous(), states[1].contiguous())
                e_old = max(err(y_old, ref_y), err(z_old, ref_z))            # the state-taking fp32-exact recurrence kernel (training forward, saved = NULL)
        print(f'  128-wide kernel: {e_old:.2e}')
        assert e_old < BAR


@pytest.mark.parametrize('width', [164, 256])
def test_split_calls_with_carried_states_are_bitwise_one_call(mp, width):
    torch.manual_seed(width)
    rnn = mp.lem.LEMcuda(6, width, 1.0).cuda()
    xin = torch.randn(97, 25, 6, device='cuda')
    with torch.no_grad():
        y, z = rnn.forward_wide(xin)
        ya, za = rnn.forward_wide(xin[:, :10].contiguous())
        yb, zb = rnn.forward_wide(xin[:, 10:].contiguous(), (ya, za))
    assert torch.equal(y, yb) and torch.equal(z, zb)


@pytest.mark.parametrize('width', [33, 164])
def test_rows_do_not_depend_on_the_batch_and_runs_repeat(mp, width):
    torch.manual_seed(width + 1)
    rnn = mp.lem.LEMcuda(8, width, 1.0).cuda()
    xin = torch.randn(300, 25, 8, device='cuda')
    st = (torch.rand(300, width, device='cuda') * 2 - 1, torch.rand(300, width, device='cuda') * 2 - 1)
    with torch.no_grad():
        y, z = rnn.forward_wide(xin, st)
        y2, z2 = rnn.forward_wide(xin, st)
        ys, zs = rnn.forward_wide(xin[:97].contiguous(), (st[0][:97].contiguous(), st[1][:97].contiguous()))
    assert torch.equal(y, y2) and torch.equal(z, z2)
    assert torch.equal(y[:97], ys) and torch.equal(z[:97], zs)


def test_nothing_is_written_outside_the_outputs(mp):
    """y_out / z_out [n, 164] inside a larger poisoned buffer: the padded channels 164..191 and the node slots 97..127 of the last
    workgroup never reach memory."""
    from msmp_pde_amd._lib import ptr, current_stream
    torch.manual_seed(2)
    L = mp.lib()
    W, n, t_len, ninp = 164, 97, 3, 4
    rnn = mp.lem.LEMcuda(ninp, W, 1.0).cuda()
    xin = mp.lem._padded_inputs(torch.randn(n, t_len, ninp, device='cuda'))
    poison, pad = 777.25, 4096
    buf = torch.full((2, pad + n * W + pad), poison, device='cuda')
    outs = [buf[i, pad:pad + n * W] for i in range(2)]
    with torch.no_grad():
        blob = rnn._pack_wide()
        rc = L.msmp_lem_encoder_wide_f32(ptr(xin), n, t_len, ninp, W, 1.0, ptr(blob), None, None, outs[0].data_ptr(), outs[1].data_ptr(), current_stream())
        assert rc == 0
        y, z = rnn.forward_wide(xin[:, :, :ninp])
    assert (buf[:, :pad] == poison).all() and (buf[:, pad + n * W:] == poison).all()
    assert torch.equal(outs[0].view(n, W), y) and torch.equal(outs[1].view(n, W), z)
    # z_out may be null: y alone, the z buffer untouched
    buf.fill_(poison)
    assert L.msmp_lem_encoder_wide_f32(ptr(xin), n, t_len, ninp, W, 1.0, ptr(blob), None, None, outs[0].data_ptr(), None, current_stream()) == 0
    assert torch.equal(outs[0].view(n, W), y) and (buf[1] == poison).all()


def test_argument_errors_are_return_codes(mp):
    from msmp_pde_amd._lib import ptr, current_stream
    L = mp.lib()
    rnn = mp.lem.LEMcuda(4, 164, 1.0).cuda()
    blob = rnn._pack_wide()
    x = torch.zeros(8, 2, 4, device='cuda')
    y = torch.full((8, 164), 3.0, device='cuda')
    z = torch.full((8, 164), 3.0, device='cuda')
    st = current_stream()
    call = lambda **kw: L.msmp_lem_encoder_wide_f32(*[kw.get(k, d) for k, d in (('xin', ptr(x)), ('n', 8), ('t', 2), ('ninp', 4), ('width', 164), ('dt', 1.0),
                                                                                ('blob', ptr(blob)), ('y0', None), ('z0', None), ('y', ptr(y)), ('z', ptr(z)), ('st', st))])
    bad = [dict(width=0), dict(width=257), dict(ninp=0), dict(ninp=9), dict(t=0), dict(xin=None), dict(blob=None), dict(y=None)]
    for kw in bad:
        rc = call(**kw)
        assert rc < 0, kw
        assert L.msmp_last_error(), kw
    assert call(n=0) == 0                           # no-op success
    for ninp, width in [(4, 0), (4, 257), (0, 164), (9, 164)]:
        assert L.msmp_packed_lem_wide_floats(ninp, width) == 0 and L.msmp_last_error()
        w = torch.zeros(16, device='cuda')
        assert L.msmp_pack_lem_wide_f32(ptr(w), ptr(w), ptr(w), ptr(w), ninp, width, ptr(w), st) < 0
    assert L.msmp_pack_lem_wide_f32(None, ptr(blob), ptr(blob), ptr(blob), 4, 164, ptr(blob), st) < 0
    torch.cuda.synchronize()
    assert (y == 3.0).all() and (z == 3.0).all()     # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert (y.abs() < 1.0).all() and (z.abs() < 1.0).all()      # the valid call did launch: states of the cell, not the 3.0 fill


def test_out_of_range_step_input_raises_the_status(mp):
    rnn = mp.lem.LEMcuda(4, 164, 1.0).cuda()
    xin = torch.randn(40, 3, 4, device='cuda')
    with torch.no_grad():
        rnn.forward_wide(xin)
        torch.cuda.synchronize()
        assert mp.last_status() == 0
        xin[17, 1, 2] = 1.0e3
        rnn.forward_wide(xin)
    torch.cuda.synchronize()
    assert mp.last_status(reset=True) & mp.MSMP_STATUS_INPUT_RANGE


def test_host_forward_without_grad_is_the_kernel(mp, monkeypatch):
    torch.manual_seed(5)
    lem = mp.LEM(4, 164).cuda()
    x = torch.randn(150, 25, 4, device='cuda')
    ref_y, _ = oracle_cell(lem.rnn, x)

    def no_addmm(*a, **k):
        raise AssertionError('torch.addmm reached')
    monkeypatch.setattr(torch, 'addmm', no_addmm)
    with torch.no_grad():
        y = lem.forward_nodes(x)
        assert err(y, ref_y) < BAR
        y_ref_layout = lem(x.permute(1, 0, 2))
        assert torch.equal(y, y_ref_layout)
        mp.lib().msmp_tune(b'lem_wide', 0)
        try:
            with pytest.raises(AssertionError, match='addmm reached'):
                lem.forward_nodes(x)
        finally:
            mp.lib().msmp_tune(b'lem_wide', 1)


def test_lems_at_width_164(mp):
    torch.manual_seed(6)
    lems = mp.LEMS(4, 164).cuda()
    ref = mp.lem.LEMcuda(4, 164, 1.0).double().cuda()
    ref.load_state_dict({k: v.double() for k, v in lems.rnn.state_dict().items()})
    xs = [torch.randn(70, 5, 4, device='cuda') for _ in range(5)]
    st = None
    with torch.no_grad():
        for i in range(4):
            if i == 3:
                lems.reset_states()
                st = None
            y = lems.forward_nodes(xs[i])
            ry, rz = ref(xs[i].permute(1, 0, 2).double().contiguous(), st, return_state=True)
            st = (ry, rz)
            assert err(y, ry.cpu().numpy()) < BAR, i
            assert err(lems.states[1], rz.cpu().numpy()) < BAR, i
    # with grad: the PyTorch-ROCm restatement, differentiable, from the carried states
    y = lems.forward_nodes(xs[4])
    assert y.grad_fn is not None
    ry = ref(xs[4].permute(1, 0, 2).double().contiguous(), st)
    assert err(y.detach(), ry.detach().cpu().numpy()) < BAR
    y.sum().backward()
    assert lems.rnn.weights.grad is not None and torch.isfinite(lems.rnn.weights.grad).all()
    with pytest.raises(RuntimeError):
        lems.forward_nodes(xs[0].cpu())


@pytest.mark.parametrize('kind,exp', [('MP_PDE_SolverLEMLinGatedGLU', 'E2'), ('MP_PDE_Solver2DLEMLinGatedGLU', 'MSWG3')])
def test_glu_solver_forward_on_either_lem_path(mp, kind, exp):
    from msmp_pde_amd import _lib
    torch.manual_seed(7)
    case = synthetic_case(mp, exp, bsz=2, seed=3)
    model = getattr(mp, kind)(case.pde, time_window=25, eq_variables=case.eqv, hidden_layer=2).cuda().eval()
    graph = case.graph.to('cuda')
    L = mp.lib()
    with torch.no_grad():
        out1 = model(graph)
        L.msmp_tune(b'lem_wide', 0)
        try:
            out0 = model(graph)
            with _lib.exact_fp32():
                out_exact = model(graph)
        finally:
            L.msmp_tune(b'lem_wide', 1)
        with _lib.exact_fp32():
            out_exact1 = model(graph)       # the switch is irrelevant on the exact path
    d = (out1 - out0).abs().max().item()
    print(f'{kind}/{exp}: lem_wide 1 vs 0 max abs {d:.2e} (output max {out0.abs().max().item():.2e})')
    assert torch.isfinite(out1).all() and d < 1e-5
    assert torch.equal(out_exact, out0) and torch.equal(out_exact1, out0)
