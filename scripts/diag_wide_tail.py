"""CPU diagnostic (no GPU): what sets the error of the fused width-generic node tail (wide_node_tail_kernel.hip) at hidden width 164?
The method of DESIGN.md section 5 (scripts/diag_quant.py, whose MFMA emulation this imports) for MP_PDE_SolverLEMLinGatedGLU: the
float64 oracle's gated pair is evaluated on the exact input of layer pairs 0, 1 and 3 with the message half in float64 and the NODE
half restated as the kernel computes it -- operands as fp16 hi + lo pairs (fp16 denormals kept, as v_mfma_f32_32x32x16_f16 keeps them),
K in steps of 16 with h and agg each padded to Wp, one fp32 rounding of the accumulator per MFMA -- one ingredient at a time:
  acc    '3': three accumulator roundings per k-step (the kernel), '0': float64 accumulation of the same split operands
  centre update_net_2 on Swish(z_n) - Swish(z_ref) from zero accumulators, or on Swish(z_n) from the scaled bias
  zscale the power of two the update_net_2 operand is multiplied by before its hi / lo split
Reported: rms / max error of the pair's output against the exact float64 pair ("fresh" error), next to numpy float32.
    python scripts/diag_wide_tail.py [E2|WE3|MSWG3|RPU]"""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, 'tests')); sys.path.insert(0, os.path.join(ROOT, 'scripts'))
import numpy as np, torch
import msmp_pde_amd as mp
from helpers import synthetic_case
from oracle import msmp_oracle as O
from diag_quant import mfma_gemm

TW = 25
f32 = lambda a: np.asarray(a, dtype=np.float32).astype(np.float64)


def node_half(p, h, agg, var, batch, acc, centre, zscale):
    """update_net_1 / update_net_2 of one head as the kernel evaluates them: the pre-norm y [n, W]"""
    W = h.shape[1]
    pad = np.zeros((h.shape[0], (-W) % 32))
    x = np.concatenate((h, pad, agg, pad, var), 1)                                    # k-steps: h | agg | variables
    w3 = np.concatenate((p.w3[:, :W], pad[:W], p.w3[:, W:2 * W], pad[:W], p.w3[:, 2 * W:]), 1)
    z = f32(O.swish(f32(mfma_gemm(x, w3, p.b3, 256.0, acc))))
    if not centre:
        return mfma_gemm(z, p.w4, p.b4, zscale, acc)
    first = np.concatenate(([0], np.flatnonzero(batch[1:] != batch[:-1]) + 1))
    return mfma_gemm(f32(z - z[first[batch]]), p.w4, 0.0 * p.b4, zscale, acc)


def main(exp):
    kind = 'MP_PDE_Solver2DLEMLinGatedGLU' if exp in ('MSWG3', 'RPU') else 'MP_PDE_SolverLEMLinGatedGLU'
    torch.manual_seed(3)
    case = synthetic_case(mp, exp, bsz=8, seed=11, device='cpu')
    model = getattr(mp, kind)(case.pde, time_window=TW, eq_variables=case.eqv, hidden_layer=6)
    sd = {k: v.detach().numpy().astype(np.float64) for k, v in model.state_dict().items()}
    g = case.graph_np()
    r64 = O.solver_forward(kind, sd, g, case.pde, TW, case.eqv, 6, parts=True)
    u = np.asarray(g.x, dtype=np.float64)
    pos_x, pos_t, var = O.build_variables(kind, g, case.pde, case.eqv)
    ei, batch = np.asarray(g.edge_index), np.asarray(g.batch)
    variants = [('split operands, float64 accumulation, uncentred', '0', False, 1.0),
                ('kernel before the centring (z x 1)', '3', False, 1.0),
                ('centred, z x 1', '3', True, 1.0),
                ('centred, z x 1, float64 accumulation', '0', True, 1.0),
                ('centred, z x 2^6', '3', True, 64.0),
                ('centred, z x 2^10', '3', True, 1024.0),
                ('centred, z x 2^10, float64 accumulation', '0', True, 1024.0),
                ('uncentred, z x 2^6', '3', False, 64.0)]
    for li in (0, 1, 3):
        hin, ref = (r64.hs[li - 1] if li else r64.h_enc), r64.hs[li]
        heads = [O.layer_params(sd, f'gnn_layers.{li}.'), O.layer_params(sd, f'gnn_layers_gate.{li}.')]
        aggs = []
        for p in heads:         # the message half in float64 (experiments/models_gnn.py:132-138, :107)
            j, i = ei[0], ei[1]
            m1 = O.swish(np.concatenate((hin[i], hin[j], u[i] - u[j], pos_x[i] - pos_x[j], var[i]), 1) @ p.w1.T + p.b1)
            aggs.append(O.scatter_mean(O.swish(m1 @ p.w2.T + p.b2), i, hin.shape[0]))

        def pair(y_of):
            tau = O.sigmoid(O.instance_norm(y_of(heads[1], aggs[1]), batch))
            return (1.0 - tau) * hin + tau * O.swish(O.instance_norm(y_of(heads[0], aggs[0]), batch))
        exact = pair(lambda p, a: O.swish(np.concatenate((hin, a, var), 1) @ p.w3.T + p.b3) @ p.w4.T + p.b4)
        assert np.abs(exact - ref).max() < 1e-9
        y = O.swish(np.concatenate((hin, aggs[0], var), 1) @ heads[0].w3.T + heads[0].b3)
        yy = y @ heads[0].w4.T + heads[0].b4
        print(f'{kind}/{exp} layer pair {li}: |Swish(z)| rms {np.sqrt(np.mean(y ** 2)):.3g}, its per-graph std (median channel) {np.median(y[:100].std(0)):.3g}; '
              f'|y| rms {np.sqrt(np.mean(yy ** 2)):.3g}, per-graph std (median channel) {np.median(yy[:100].std(0)):.3g}')
        o32 = pair(lambda p, a: (O.swish((np.concatenate((hin, a, var), 1).astype(np.float32) @ p.w3.T.astype(np.float32) + p.b3.astype(np.float32)))
                                 @ p.w4.T.astype(np.float32) + p.b4.astype(np.float32)).astype(np.float64))
        print(f'    {"node half in numpy float32":55s} rms {np.sqrt(np.mean((o32 - ref) ** 2)):.2e}  max {np.abs(o32 - ref).max():.2e}')
        for name, acc, centre, zscale in variants:
            out = pair(lambda p, a: node_half(p, hin, a, var, batch, acc, centre, zscale))
            print(f'    {name:55s} rms {np.sqrt(np.mean((out - ref) ** 2)):.2e}  max {np.abs(out - ref).max():.2e}')


if __name__ == '__main__':
    main(sys.argv[1] if len(sys.argv) > 1 else 'E2')
