"""GPU tests of the centred update_net_2 of the fused width-generic node tail (msmp_wide_node_tail_f32, wide_node_tail_kernel.hip; DESIGN.md
4.20, 5).  InstanceNorm removes any per-graph, per-channel constant, so the kernel runs update_net_2 on 2^6 (Swish(z_n) - Swish(z_ref)) (z_ref:
the graph's first node) from zero accumulators and never reads b4: the roundings of the fp32 accumulator are then relative to the variation
of y over the graph, which is what the norm divides by, and the fp16 hi / lo split of the operand stays out of the fp16 denormals
(profiles/r28a_glu_wide_tail_centred.md: centred but unscaled, E2 still measured 1.80e-4 / 9.81e-6).  Checked here:
  * b4 does not enter the arithmetic: a head packed with its b4 and with b4 = 0 gives the same bits;
  * the GLU classes at full depth under msmp_tune("wide_tail", 1) against the float64 oracle, at the bar of test_full_depth_vs_oracle
    (helpers.assert_parity: max(1e-5, 2 x float32 floor) on max and rms).  Before the centring MP_PDE_SolverLEMLinGatedGLU / E2 measured
    max 2.13e-4 / rms 1.32e-5 against 8.4e-5 / 1.0e-5 (profiles/r10a_glu_wide_node_tail.md);
  * the rule of test_layer_error_growth for that class with the switch on.
The parity properties of the kernel itself (float64 formula, run-to-run bits, independence of the batch, padding) stay in
test_gpu_wide_node_tail.py."""
import numpy as np
import pytest
import torch

from oracle import msmp_oracle as O
from helpers import synthetic_case, ld_of, assert_parity, record_parity, fp32_floors, layer_error_profile, counted
from helpers import mp, restore_wide_switches       # noqa: F401  (fixtures)

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures('restore_wide_switches')]

TW = 25
EPS = 1e-5
SIZES = [100, 65, 64, 1, 2, 128]        # two pairs, one node into the second pair, exactly one pair, one node, two nodes, the cap
GLU_CASES = [('MP_PDE_SolverLEMLinGatedGLU', 'E2'), ('MP_PDE_SolverLEMLinGatedGLU', 'WE3'),
             ('MP_PDE_Solver2DLEMLinGatedGLU', 'MSWG3'), ('MP_PDE_Solver2DLEMLinGatedGLU', 'RPU')]


class Case(object):
    """The Case of test_gpu_wide_node_tail.py (update_net_1 / update_net_2 of two GNN_LayerLin heads at width W with the reference's
    initialisation; h and both aggregates standard normal with row stride ld, variables uniform in [0, 1)), every head packed TWICE:
    blobs[k] with its b4, blobs_b0[k] with b4 = 0."""

    def __init__(self, mp, W, nv, sizes, ld, seed=0):
        from msmp_pde_amd._lib import ptr, current_stream
        torch.manual_seed(1000 * W + 10 * nv + seed)
        self.W, self.nv, self.ld, self.sizes, self.n = W, nv, ld, list(sizes), int(sum(sizes))
        self.gptr = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int32, device='cuda')
        L = mp.lib()
        nf = L.msmp_packed_wide_tail_floats(W, nv)
        assert nf > 0

        def pack(w):
            blob = torch.empty(nf, dtype=torch.float32, device='cuda')
            assert L.msmp_pack_wide_tail_f32(ptr(w[0]), ptr(w[1]), ptr(w[2]), ptr(w[3]), W, nv, ptr(blob), current_stream()) == 0
            return blob
        self.b4, self.blobs, self.blobs_b0 = [], [], []
        for _ in range(2):
            layer = mp.GNN_LayerLin(W, W, W, 25, nv).cuda()
            sd = {k: v.detach() for k, v in layer.state_dict().items()}
            w = [sd[k].contiguous() for k in ('update_net_1.0.weight', 'update_net_1.0.bias', 'update_net_2.0.weight', 'update_net_2.0.bias')]
            assert w[0].shape == (W, 2 * W + nv) and w[2].shape == (W, W) and w[3].shape == (W,)
            self.b4.append(w[3])
            self.blobs.append(pack(w))
            self.blobs_b0.append(pack(w[:3] + [torch.zeros_like(w[3])]))
        torch.cuda.synchronize()
        n = self.n
        self.h = torch.randn(n, ld, device='cuda')
        self.agg = [torch.randn(n, ld, device='cuda') for _ in range(2)]
        self.var = torch.rand(n, nv, device='cuda')


def run(mp, case, blobs, gated):
    from msmp_pde_amd._lib import ptr, current_stream
    out = torch.full((case.n, case.ld), float('nan'), device='cuda')
    rc = mp.lib().msmp_wide_node_tail_f32(ptr(case.h), ptr(case.agg[0]), ptr(case.agg[1]) if gated else None, ptr(case.var), ptr(case.gptr), case.n,
                                          len(case.sizes), max(case.sizes), case.nv, case.W, case.ld, ptr(blobs[0]), ptr(blobs[1]) if gated else None,
                                          EPS, out.data_ptr(), current_stream())
    torch.cuda.synchronize()
    assert rc == 0
    return out


@pytest.mark.parametrize('gated', [True, False], ids=['gated', 'plain'])
@pytest.mark.parametrize('W', [33, 164, 256])       # KT 2, 6, 8
def test_b4_does_not_enter_the_arithmetic(mp, W, gated):
    case = Case(mp, W, 2, SIZES, ld_of(W))
    for k in range(2):
        # the precondition: b4 does not move the power-of-two scale of (W4, b4), so the two blobs carry the same scaled W4 and differ in
        # the b4 words alone (true of these seeds: max |b4| < max |W4| under the reference's initialisation)
        assert torch.equal(case.blobs[k][:8], case.blobs_b0[k][:8])
        assert case.b4[k].abs().max().item() > 1e-3 and not torch.equal(case.blobs[k], case.blobs_b0[k])
    with_b4, without = run(mp, case, case.blobs, gated), run(mp, case, case.blobs_b0, gated)
    assert torch.isfinite(with_b4).all()
    assert torch.equal(with_b4, without)
    assert mp.last_status() == 0


@pytest.mark.parametrize('kind,exp', GLU_CASES)
def test_full_depth_under_the_switch(mp, kind, exp, monkeypatch):
    """test_full_depth_vs_oracle (6 gated pairs, 8 graphs, default initialisation, the same seeds) with the fused node tail selected."""
    torch.manual_seed(3)
    case = synthetic_case(mp, exp, bsz=8, seed=11)
    model = getattr(mp, kind)(case.pde, time_window=TW, eq_variables=case.eqv, hidden_layer=6)
    model.cuda().eval()
    data = case.graph.to('cuda')
    mp.lib().msmp_tune(b'wide_tail', 1)
    calls = counted(mp, monkeypatch, 'msmp_wide_node_tail_f32')
    with torch.no_grad():
        out = model(data)
        assert len(calls) == 6                      # one launch per gated pair
        out2 = model(data)
    assert len(calls) == 12
    assert torch.equal(out, out2)                   # fixed summation order -> bitwise repeatable
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    g = case.graph_np()
    ref = O.solver_forward(kind, sd, g, case.pde, TW, case.eqv, 6)
    floor = fp32_floors(kind, sd, g, case.pde, TW, case.eqv, 6)
    assert_parity('full_depth_wide_tail_centred', f'{kind}/{exp}', out.double().cpu().numpy(), ref, floor)     # bar: helpers.assert_parity


def test_layer_error_growth_under_the_switch(mp):
    """The rule of test_layer_error_growth for MP_PDE_SolverLEMLinGatedGLU / E2 with the fused node tail selected: after every gated pair
    the rms error of the hidden state against the float64 oracle is at most 1.5 x that of the oracle's float32 evaluation at the same
    layer, and grows from one layer to the next at most 1.5 x as fast.  The error a layer adds on exact input ("fresh") is recorded, not
    asserted: width 164 has no reference value for it yet."""
    kind, exp = 'MP_PDE_SolverLEMLinGatedGLU', 'E2'
    mp.lib().msmp_tune(b'wide_tail', 1)
    r = layer_error_profile(mp, kind, exp)
    hip = [r['encoder']['hip'][1]] + [l['hip'][1] for l in r['layers']]
    f32 = [r['encoder']['f32'][1]] + [l['f32'][1] for l in r['layers']]
    fresh = [l['hip_fresh'][1] for l in r['layers']]
    record_parity('layer_error_growth_wide_tail_centred', f'{kind}/{exp}', hip_rms=hip, f32_rms=f32, fresh_rms=fresh,
                  out_hip=r['out']['hip'], out_f32=r['out']['f32'])
    print(f'{kind}/{exp} (wide_tail 1): rms per layer hip ' + ' '.join(f'{x:.2e}' for x in hip) + ' | f32 ' + ' '.join(f'{x:.2e}' for x in f32)
          + ' | hip/f32 ' + ' '.join(f'{a / b:.2f}' for a, b in zip(hip[1:], f32[1:])) + ' | fresh ' + ' '.join(f'{x:.1e}' for x in fresh))
    for i in range(1, len(hip)):
        assert hip[i] <= 1.5 * f32[i], (i, hip[i], f32[i])
        if i > 1:
            assert hip[i] / hip[i - 1] <= 1.5 * f32[i] / f32[i - 1], (i, hip[i] / hip[i - 1], f32[i] / f32[i - 1])
