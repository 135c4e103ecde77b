"""GPU tests of the gated CNN decoder of the GLU classes (msmp_decoder_gated_f32 / msmp_decoder2d_gated_f32, decoder_kernel.hip): the two
entries against the float64 formulas of the reference (oracle.msmp_oracle.conv1d / swish) at node counts around both possible
nodes-per-workgroup values and at two row strides each, their bitwise properties (repeatable, node rows independent of one another and of
the batch around them), double_mlp at width 164 as one msmp_linear_f32 call, and the host path of the two solver classes: which launches a
forward makes under each switch, the dtype it returns, and a captured forward.

Bar of the float64 comparisons: max(1e-6, 2 x floor), floor = the max abs error of the SAME formula evaluated in float32 by torch on the
CPU for the same inputs (outputs reach |x| ~ 5, where half an ulp is 2.4e-7: the plain 1e-6 of the one-network decoders is not reachable
by any float32 evaluation here); the factor 2 is the project's margin over a float32 floor."""
import numpy as np
import pytest
import torch

from oracle import msmp_oracle as O
from helpers import mp, synthetic_case, fp32_floors, err_stats, launch_counts, tuned       # noqa: F401  (mp: fixture)

pytestmark = pytest.mark.gpu
W, HALF, TW, DT = 164, 82, 25, 0.016
N_MAX = 333
NODE_COUNTS = [1, 15, 16, 17, 31, 32, 33, 333]
LDS = {1: (164, 256), 2: (328, 384)}


def bar_of(floor):
    return max(1e-6, 2.0 * floor)


def make_nets(comps, seed):
    """(gate, diff): Conv1d(comps -> 8, 6, stride 2) and Conv1d(8 -> comps, 15) at nn.Conv1d's default init, float32 on the CPU"""
    torch.manual_seed(seed)
    return [(torch.nn.Conv1d(comps, 8, 6, stride=2), torch.nn.Conv1d(8, comps, 15)) for _ in range(2)]


def flat_weights(nets, device):
    return [p.detach().to(device=device, dtype=torch.float32).contiguous() for c1, c2 in nets for p in (c1.weight, c1.bias, c2.weight, c2.bias)]


def reference64(comps, rows, u, nets):
    """float64 numpy: rows [n, comps, 164], u [n, comps * tw] -> out [n, comps * tw] by the reference's formulas (models_gnn.py:1514-1521,
    models_gnn2D.py:1355-1366)"""
    p = [[t.detach().double().numpy() for t in (c1.weight, c1.bias, c2.weight, c2.bias)] for c1, c2 in nets]
    dec = lambda x, q: O.conv1d(O.swish(O.conv1d(x, q[0], q[1], 2)), q[2], q[3], 1)
    scale, diff = dec(rows[:, :, :HALF], p[0]), dec(rows[:, :, HALF:], p[1])
    dtc = np.cumsum(np.full(TW, DT, dtype=np.float64))
    if comps == 1:
        return (1.0 - scale[:, 0]) * u[:, -1:] + dtc[None, :] * (scale[:, 0] * diff[:, 0])
    return ((1.0 - scale) * u.reshape(-1, 2, TW) + dtc[None, None, :] * scale * diff).reshape(-1, 2 * TW)


def formula32(comps, rows, u, nets):
    """the same formulas in float32 torch on the CPU"""
    with torch.no_grad():
        swish = lambda x: x * torch.sigmoid(x)
        dec = lambda x, net: net[1](swish(net[0](x)))
        scale, diff = dec(rows[:, :, :HALF].contiguous(), nets[0]), dec(rows[:, :, HALF:].contiguous(), nets[1])
        dtc = torch.cumsum(torch.ones(TW, dtype=torch.float32) * DT, 0)
        if comps == 1:
            return (1.0 - scale[:, 0]) * u[:, -1:] + dtc.view(1, TW) * (scale[:, 0] * diff[:, 0])
        return ((1.0 - scale) * u.view(-1, 2, TW) + dtc.view(1, 1, TW) * scale * diff).flatten(1, 2)


class _Shared:
    """inputs of N_MAX nodes, their float64 reference and the per-element error of the float32 formula: computed once per entry, read only"""

    def __init__(self, comps):
        rng = np.random.default_rng(40 + comps)
        self.comps = comps
        self.rows = torch.tensor(rng.standard_normal((N_MAX, comps, W)), dtype=torch.float32)
        self.u = torch.tensor(rng.standard_normal((N_MAX, comps * TW)), dtype=torch.float32)
        self.nets = make_nets(comps, 7 + comps)
        self.ref = reference64(comps, self.rows.double().numpy(), self.u.double().numpy(), self.nets)
        self.floor_err = np.abs(formula32(comps, self.rows, self.u, self.nets).double().numpy() - self.ref)
        self.fill = torch.tensor(rng.standard_normal((N_MAX, 512)), dtype=torch.float32)      # what lies between the rows at a larger stride
        self.weights = flat_weights(self.nets, 'cuda')

    def strided(self, ld, sel=slice(None)):
        """the rows `sel` at row stride ld on the GPU, the floats past a row's comps * 164 values random"""
        x = self.fill[sel, :ld].clone()
        x[:, :self.comps * W] = self.rows[sel].reshape(-1, self.comps * W)
        return x.cuda().contiguous()


_SHARED = {}


@pytest.fixture(scope='module')
def shared():
    def get(comps):
        if comps not in _SHARED:
            _SHARED[comps] = _Shared(comps)
        return _SHARED[comps]
    return get


def run_entry(mp, comps, x, ld, u, weights, width=W, tw=TW):
    from msmp_pde_amd._lib import check, ptr, current_stream
    name = 'msmp_decoder2d_gated_f32' if comps == 2 else 'msmp_decoder_gated_f32'
    out = torch.empty_like(u)
    check(getattr(mp.lib(), name)(ptr(x), ld, ptr(u), u.shape[0], width, tw, *[ptr(t) for t in weights], DT, ptr(out), current_stream()), name)
    return out


@pytest.mark.parametrize('n', NODE_COUNTS)
@pytest.mark.parametrize('comps,ld', [(c, ld) for c in (1, 2) for ld in LDS[c]])
def test_entries_against_the_float64_formula(mp, shared, comps, ld, n):
    s = shared(comps)
    out = run_entry(mp, comps, s.strided(ld, slice(0, n)), ld, s.u[:n].cuda().contiguous(), s.weights)
    err = np.abs(out.double().cpu().numpy() - s.ref[:n]).max()
    floor = s.floor_err[:n].max()
    print(f'gated decoder {comps}-D, ld {ld}, {n} nodes: max|hip - float64| = {err:.3e}, float32 floor {floor:.3e}, bar {bar_of(floor):.3e}, '
          f'max|out| {np.abs(s.ref[:n]).max():.3g}')
    assert err <= bar_of(floor), (comps, ld, n, err, floor)


@pytest.mark.parametrize('comps', [1, 2])
def test_rows_are_repeatable_and_independent_of_one_another(mp, shared, comps):
    s = shared(comps)
    ld = LDS[comps][1]
    x, u = s.strided(ld), s.u.cuda().contiguous()
    out = run_entry(mp, comps, x, ld, u, s.weights)
    assert torch.equal(run_entry(mp, comps, x, ld, u, s.weights), out)                       # two runs
    perm = torch.randperm(N_MAX, generator=torch.Generator().manual_seed(5)).cuda()
    assert torch.equal(run_entry(mp, comps, x[perm].contiguous(), ld, u[perm].contiguous(), s.weights), out[perm])      # permuted node rows
    lo = 100                                                                                 # rows 100 .. 116 as a 17-node call of their own
    few = run_entry(mp, comps, x[lo:lo + 17].contiguous(), ld, u[lo:lo + 17].contiguous(), s.weights)
    assert torch.equal(few, out[lo:lo + 17])
    assert torch.equal(run_entry(mp, comps, s.strided(LDS[comps][0]), LDS[comps][0], u, s.weights), out)      # the row stride changes no bit


def test_double_mlp_as_one_row_gemm(mp):
    """double_mlp at width 164 (Linear(164, 328) + Swish) in the form the 2-D class uses: one msmp_linear_f32 call into the 384-float rows
    the decoder reads in place; against float64, bar of test_general_linear_kernel."""
    from msmp_pde_amd import decoder
    torch.manual_seed(11)
    lin = torch.nn.Linear(W, 2 * W).cuda()
    h = torch.randn(33, W, device='cuda')
    hd, ld = decoder.double_mlp(lin, h)
    assert ld == 384 and hd.shape == (33, 384)
    ref = O.swish(O.linear(h.double().cpu().numpy(), lin.weight.detach().double().cpu().numpy(), lin.bias.detach().double().cpu().numpy()))
    got = hd.double().cpu().numpy()
    err = np.abs(got[:, :2 * W] - ref).max()
    print(f'double_mlp as msmp_linear_f32: max|hip - float64| = {err:.3e}')
    assert err < 2e-6 * max(1.0, np.abs(ref).max())
    assert np.all(got[:, 2 * W:] == 0.0)


CLASSES = [('MP_PDE_SolverLEMLinGatedGLU', 'E2'), ('MP_PDE_Solver2DLEMLinGatedGLU', 'MSWG3')]


def small_model(mp, kind, exp):
    torch.manual_seed(7)
    case = synthetic_case(mp, exp, bsz=2, seed=3)
    model = getattr(mp, kind)(case.pde, time_window=TW, eq_variables=case.eqv, hidden_layer=2).cuda().eval()
    return case, model, case.graph.to('cuda')


@pytest.mark.parametrize('kind,exp', CLASSES)
def test_solver_forward_on_either_decoder_against_the_oracle(mp, kind, exp):
    """Both settings of "wide_dec" against the class's float64 oracle and against each other; floor: the float32 evaluations of the same
    oracle (helpers.fp32_floors)."""
    case, model, graph = small_model(mp, kind, exp)
    L = mp.lib()
    with torch.no_grad():
        with tuned(L, wide_dec=1):          # `tuned` puts a switch back in its `finally`
            out1 = model(graph)
        with tuned(L, wide_dec=0):
            out0 = model(graph)
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    g = case.graph_np()
    ref = O.solver_forward(kind, sd, g, case.pde, TW, case.eqv, 2)
    floor = max(err_stats(v, ref)[0] for v in fp32_floors(kind, sd, g, case.pde, TW, case.eqv, 2).values())
    e1, e0 = err_stats(out1.double().cpu().numpy(), ref)[0], err_stats(out0.double().cpu().numpy(), ref)[0]
    d = (out1 - out0).abs().max().item()
    print(f'{kind}/{exp}: max|hip - float64| = {e1:.3e} (wide_dec 1), {e0:.3e} (wide_dec 0), 1 against 0 {d:.3e}; float32 floor {floor:.3e}, '
          f'bar {bar_of(floor):.3e}, max|out| {np.abs(ref).max():.3g}')
    assert out1.dtype == graph.x.dtype and out1.shape == out0.shape == ref.shape
    assert e1 <= bar_of(floor) and e0 <= bar_of(floor) and d <= bar_of(floor), (e1, e0, d, floor)


@pytest.mark.parametrize('kind,exp', CLASSES)
def test_which_forward_takes_the_launch(mp, kind, exp):
    """The library's own launch counter of the decoder family: exactly one launch per no-grad forward with "wide_dec" on, none with it off,
    under autograd, or with "lem_wide" 0 (the unfused path as a whole)."""
    case, model, graph = small_model(mp, kind, exp)
    L = mp.lib()

    def decoder_launches(grad=False):
        with launch_counts(L) as counts:
            with torch.enable_grad() if grad else torch.no_grad():
                out = model(graph)
        assert torch.isfinite(out).all()
        return counts['DECODER']

    with tuned(L, wide_dec=1):              # `tuned` puts a switch back in its `finally`
        with torch.no_grad():
            model(graph)                    # the first forward of a model also probes the range status
        assert decoder_launches() == 1
        assert decoder_launches(grad=True) == 0
        with tuned(L, lem_wide=0):
            assert decoder_launches() == 0
        with tuned(L, wide_dec=0):
            assert decoder_launches() == 0
        with tuned(L, wide_dec=5):          # any value other than 0 is "on"
            assert decoder_launches() == 1


@pytest.mark.parametrize('kind,exp', CLASSES)
def test_dtype_of_the_result_and_a_captured_forward(mp, kind, exp):
    case, model, graph = small_model(mp, kind, exp)
    import copy
    with tuned(mp.lib(), wide_dec=1), torch.no_grad():
        assert graph.x.dtype == torch.float64
        eager = model(graph)
        assert eager.dtype == torch.float64
        g32 = copy.copy(graph)
        g32.x = graph.x.float()
        assert model(g32).dtype == torch.float32
        step = model.capture(graph)
        assert torch.equal(step(graph), eager)            # the replay gives the eager bits
        assert torch.equal(step(graph), eager)
        torch.cuda.synchronize()
