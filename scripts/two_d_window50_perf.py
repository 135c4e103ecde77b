"""Time record of the 2-D classes at time_window 50 (four 32-column tail chunks of message_net_1), all in ONE process:
  1. forward time per rollout step of MSMP-PDE2D (MP_PDE_Solver2DLEMLinGated) on MSWG3 at time_window 50 next to 25;
  2. per-launch time of the folded tile message kernel with four tail chunks (tw = 100) next to two (tw = 50), same graphs;
  3. A/B of the four-chunk layer: folded projections (one launch) against mode 0 (msmp_node_project_f32 + the tile kernel on staged
     P / Q rows), per launch and per rollout step (msmp_tune("tile", 1) against the default).
Rounds of A and B alternate; medians of CUDA-event times.  Usage: python scripts/two_d_window50_perf.py [--graphs 2048] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import msmp_pde_amd as mp                                   # noqa: E402
from msmp_pde_amd._lib import check, ptr, current_stream     # noqa: E402
from msmp_pde_amd.synthetic import make_case                 # noqa: E402
from msmp_pde_amd.graph import structure_of                  # noqa: E402
from msmp_pde_amd.layers import node_features                # noqa: E402

H = 128


def timed(fn, reps):
    """milliseconds per call: `reps` calls between two events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def ab(fns, rounds, reps):
    """alternating rounds; median ms per call of each named function"""
    for f in fns.values():
        f()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(rounds):
        for k, f in fns.items():
            t[k].append(timed(f, reps))
    return {k: statistics.median(v) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', type=int, default=2048)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None, help='also write the JSON record to this file (it is always printed)')
    a = ap.parse_args()
    L = mp.lib()
    res = {'graphs': a.graphs, 'device': torch.cuda.get_device_name(0)}

    # ---- 1 + 3b: forward per rollout step, time_window 50 vs 25, and the mode-0 routing of the 50 model
    models, datas = {}, {}
    for tw in (25, 50):
        c = make_case('MSWG3', a.graphs, seed=1, device='cuda', tw=tw, dtype=torch.float32)
        steps = [60] * a.graphs
        data, labels = c.creator.create_data(c.u_super, steps)
        datas[tw] = c.creator.create_graph(data, labels, c.x, c.variables, steps)
        torch.manual_seed(0)
        models[tw] = mp.MP_PDE_Solver2DLEMLinGated(c.pde, time_window=tw, eq_variables=c.eqv, hidden_layer=6).cuda().eval()
    tile_default = L.msmp_tune_query(b'tile')

    def fwd(tw):
        def f():
            with torch.no_grad():
                models[tw](datas[tw])
        return f

    def fwd_mode0():
        L.msmp_tune(b'tile', 1)
        try:
            fwd(50)()
        finally:
            L.msmp_tune(b'tile', tile_default)
    with torch.no_grad():
        o_def = models[50](datas[50])
        L.msmp_tune(b'tile', 1)
        o_m0 = models[50](datas[50])
        L.msmp_tune(b'tile', tile_default)
    res['step_max_abs_diff_folded_vs_mode0'] = float((o_def - o_m0).abs().max())
    res['step_ms'] = ab({'tw25': fwd(25), 'tw50': fwd(50), 'tw50_mode0': fwd_mode0}, a.rounds, 3)
    print('forward per step (ms):', res['step_ms'], flush=True)

    # ---- 2 + 3a: one layer's message kernel on the 2048-graph structure
    gs = structure_of(datas[50])
    t = gs.tiles()
    n, e = gs.n_nodes, gs.n_edges
    rng = np.random.default_rng(0)
    h = torch.tensor(rng.standard_normal((n, H)), dtype=torch.float32).cuda()
    pos = torch.rand(n, device='cuda')
    var = torch.rand(n, 3, device='cuda')
    kern = {}
    for tw in (50, 100):
        nv = 3
        k1, k3 = 2 * H + tw + 1 + nv, 2 * H + nv
        w = lambda *s: (torch.rand(*s, device='cuda') * 2 - 1) / np.sqrt(s[-1])
        ts = [w(H, k1), w(H, k1)[:, 0].contiguous(), w(H, H), w(H, H)[:, 0].contiguous(), w(H, k3), w(H, k3)[:, 0].contiguous(), w(H, H),
              w(H, H)[:, 0].contiguous()]
        blob = torch.empty(L.msmp_packed_layer_floats(tw, nv), device='cuda')
        check(L.msmp_pack_layer_f32(*[ptr(x) for x in ts], tw, nv, ptr(blob), current_stream()), 'pack')
        u = (torch.randn(n, tw, device='cuda') * 0.05).contiguous()
        feat = node_features(u, pos, var)
        agg, P, Q = (torch.empty(n, H, device='cuda') for _ in range(3))
        kern[tw] = (u, feat, blob, agg, P, Q)

    def folded(tw):
        u, feat, blob, agg, _, _ = kern[tw]
        return lambda: check(L.msmp_edge_aggregate_tiled_f32(ptr(h), ptr(u), ptr(pos), ptr(var), ptr(feat), None, None, ptr(gs.rowptr),
                                                             ctypes.byref(t[0]), n, e, tw, 3, ptr(blob), ptr(agg), current_stream()), 'folded')

    def mode0(tw):
        u, _, blob, agg, P, Q = kern[tw]

        def f():
            check(L.msmp_node_project_f32(ptr(h), ptr(u), ptr(pos), ptr(var), n, tw, 3, ptr(blob), ptr(P), ptr(Q), current_stream()), 'proj')
            check(L.msmp_edge_aggregate_tiled_f32(None, None, None, None, None, ptr(P), ptr(Q), ptr(gs.rowptr), ctypes.byref(t[0]), n, e, tw, 3,
                                                  ptr(blob), ptr(agg), current_stream()), 'staged')
        return f
    res['layer_nodes'], res['layer_edges'] = n, e
    res['message_us'] = {k: 1e3 * v for k, v in ab({'folded_2chunks_tw50': folded(50), 'folded_4chunks_tw100': folded(100),
                                                     'mode0_4chunks_tw100': mode0(100)}, a.rounds, 20).items()}
    print('message per launch (us):', res['message_us'], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == '__main__':
    main()
