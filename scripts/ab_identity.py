"""Do two (or more) builds of the library give the same bits?  Run on the GPU box:
    python scripts/ab_identity.py libmsmp_pde.so libmsmp_pde_v3.so [--graphs 64] [--encoders | --training]
Each library (a path relative to the package, or absolute) runs in its own process (MSMP_LIB_PATH), under its own time limit, on the same seeded
workloads (E2 / WE3 / RPU / MSWG3, MSMP-PDE classes: two rollout steps) and prints a SHA-256 of the predictions; this parent compares them
and, where they differ, prints the largest difference (so a numerics-preserving but not bit-identical change is told apart from a wrong one).
It stops at the first child that does not exit 0.
--encoders: the recurrent encoders under autograd instead (ENCODER_CASES: the LEM and LSTM training pairs through their raw entries and their
Functions; final states, the whole `saved` and dG buffers and the four parameter gradients are hashed).
--training: the training-side entries instead (training_child): msmp_mp_layer_bwd_f32 over LAYER_CASES (dh and the 8 / 16 gradients),
msmp_wide_layer_bwd_f32 at widths 164 and 256, the msmp_linear_f32 / msmp_linear_swish_f32 outputs, both reductions, and parameters and moments
after eager, capturable and guarded AdamW steps over 50 tensors.  The package of this tree drives every library, so a difference isolates the
device side."""
import hashlib, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [('E2', 'MSMP-PDE'), ('WE3', 'MSMP-PDE'), ('RPU', 'MSMP-PDE2D'), ('MSWG3', 'MSMP-PDE2D'), ('E2', 'MP-PDE')]


# the smallest shapes that reach every path: KT 2, 4, 6, 8, a pad inside a tile, a second 128-column block of dG; at width 128 every compile-time
# NS body and every odd input pad; the t == 0 branch, one node in a second tile, dead lanes; with and without initial states
ENCODER_CASES = [(cell, w, ninp, t, n, states) for cell in ('lem', 'lstm') for w in (33, 128, 164, 256) for ninp in (range(1, 9) if w == 128 else (5,))
                 for t, n in ((1, 1), (3, 33)) for states in (False, True)]


def encoder_child(out):
    sys.path.insert(0, ROOT)
    import torch
    import msmp_pde_amd as mp
    from msmp_pde_amd import lem, lstm
    L, res = mp.lib(), {}
    L.msmp_tune(b'lstm_train', 1)
    for cell, w, ninp, t, n, states in ENCODER_CASES:
        g = torch.Generator().manual_seed(1000 * w + 10 * ninp + t)
        rand = lambda *shape: (torch.rand(*shape, generator=g) * 2 - 1).cuda()
        xin, gy = rand(n, t, ninp), rand(n, w)
        s0, s1 = (rand(n, w), rand(n, w)) if states else (None, None)
        x = lem._padded_inputs(xin)
        wp, ldg = 32 * ((w + 31) // 32), 128 * ((w + 127) // 128)
        saved, dg = torch.zeros(6 * n * t * wp, device='cuda'), torch.zeros(n * t, 4 * ldg, device='cuda')
        if cell == 'lem':
            rnn = lem.LEMcuda(ninp, w, 0.5).cuda()
            ps = [rnn.weights, rnn.weights_lin_z, rnn.bias, rnn.bias_lin_z]
        else:
            rnn = torch.nn.LSTM(ninp, w).cuda()
            ps = [rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0]
        with torch.no_grad():
            for p in ps:
                p.copy_(rand(*p.shape) / w ** 0.5)
        blob_t = torch.empty(getattr(L, f'msmp_packed_{"lem_wide" if cell == "lem" else "lstm"}_bwd_floats')(ninp, w), device='cuda')
        ptr, st = mp._lib.ptr, mp._lib.current_stream()
        if cell == 'lem':
            h, c = lem._train_forward(rnn, x, s0, s1, saved)
            mp._lib.check(L.msmp_pack_lem_wide_bwd_f32(ptr(ps[0]), ptr(ps[1]), ninp, w, ptr(blob_t), st), 'pack')
            mp._lib.check(L.msmp_lem_train_bwd_wide_f32(ptr(gy), ptr(saved), ptr(s0), ptr(s1), n, t, w, rnn.dt, ptr(blob_t), ptr(dg), st), 'bwd')
            out_f = lem._LEMTrainFunction.apply(rnn, xin, *ps, s0, s1)[0]
        else:
            blob = lstm.packed(mp._lib.PackedCache(), rnn)
            h, c = lstm.train_forward(blob, ninp, w, x, s0, s1, saved)
            mp._lib.check(L.msmp_pack_lstm_bwd_f32(ptr(ps[1]), ninp, w, ptr(blob_t), st), 'pack')
            mp._lib.check(L.msmp_lstm_train_bwd_f32(ptr(gy), ptr(saved), ptr(s1), n, t, w, ptr(blob_t), ptr(dg), st), 'bwd')
            out_f = lstm._LSTMTrainFunction.apply(blob, xin, *ps, s0, s1)[0]
        (out_f * gy).sum().backward()
        torch.cuda.synchronize()
        digest = hashlib.sha256()
        for tensor in [h, c, saved, dg, out_f] + [p.grad for p in ps]:
            digest.update(tensor.detach().float().cpu().contiguous().numpy().tobytes())
        res[f'{cell} W={w} ninp={ninp} T={t} N={n} states={int(states)}'] = digest.hexdigest()
    json.dump(res, open(out, 'w'))


# (graphs of 100 nodes with 6 neighbours, tw, nv, form, by-source arrays given, tune bwd_gemm): 2 graphs = 1 200 edges on rows_gemm_small_kernel;
# 56 graphs = 33 600 edges, just past RG_SMALL_ROWS = 32 768, on the 128-row kernel; one 2-D-sized window (tw = 50, nv = 3) on the factorised route
LAYER_CASES = [(2, 25, 1, form, by_source, bwd_gemm) for form in ('gated', 'lin', 'residual') for by_source in (True, False) for bwd_gemm in (0, 1)]
LAYER_CASES += [(56, 25, 1, 'gated', True, 1), (2, 50, 3, 'gated', True, 1)]


def training_child(out):
    """Hashes of what the training-side entries leave: the layer backwards, the linear entries, the reductions and the optimiser steps."""
    sys.path.insert(0, ROOT)
    import ctypes, torch
    import msmp_pde_amd as mp
    from msmp_pde_amd import autograd as A, optim, reductions
    from msmp_pde_amd.graph import GraphStructure
    from msmp_pde_amd._lib import check, ptr, current_stream
    L, res = mp.lib(), {}

    def digest(tensors):
        torch.cuda.synchronize()
        d = hashlib.sha256()
        for t in tensors:
            d.update(t.detach().cpu().contiguous().numpy().tobytes())
        return d.hexdigest()

    def batch_of(graphs):
        i = torch.arange(100)
        src = torch.cat([(i + d) % 100 for d in (-3, -2, -1, 1, 2, 3)])
        ei = torch.cat([torch.stack([src, i.repeat(6)]) + 100 * g for g in range(graphs)], 1).cuda()
        return GraphStructure(ei, torch.arange(graphs).repeat_interleave(100).cuda(), 100 * graphs)

    def layer_inputs(gs, width, tw, nv, gated):
        g = torch.Generator().manual_seed(1000 * width + 10 * tw + gs.n_graphs)
        r = lambda *s: torch.randn(*s, generator=g).cuda()
        n, k1, k3 = gs.n_nodes, 2 * width + tw + 1 + nv, 2 * width + nv
        one = lambda: [r(width, k1) / k1 ** 0.5, r(width) * 0.1, r(width, width) / width ** 0.5, r(width) * 0.1,
                       r(width, k3) / k3 ** 0.5, r(width) * 0.1, r(width, width) / width ** 0.5, r(width) * 0.1]
        return (r(n, width), r(n, width), r(n, tw), r(n), r(n, nv)), one() + (one() if gated else [])

    arr = lambda ts: (ctypes.c_void_p * 8)(*[t.data_ptr() for t in ts])
    structures = {}
    for graphs, tw, nv, form, by_source, bwd_gemm in LAYER_CASES:
        gs = structures.setdefault(graphs, batch_of(graphs))
        gated = form == 'gated'
        (gout, h, u, pos, var), ps = layer_inputs(gs, 128, tw, nv, gated)
        grads, dh = [torch.empty_like(q) for q in ps], torch.empty_like(h)
        ws = torch.empty(L.msmp_mp_layer_bwd_workspace_bytes(gs.n_nodes, gs.n_edges, tw, nv, int(gated)), dtype=torch.uint8, device='cuda')
        perm32, src_rowptr = gs.by_source32() if by_source else (None, None)
        prev = L.msmp_tune_query(b'bwd_gemm')
        check(L.msmp_tune(b'bwd_gemm', bwd_gemm), 'tune')
        check(L.msmp_mp_layer_bwd_f32(ptr(gout), ptr(h), ptr(u), ptr(pos), ptr(var), ptr(gs.rowptr), ptr(gs.col), ptr(gs.tgt), ptr(src_rowptr),
                                      ptr(perm32), ptr(gs.graph_ptr), gs.n_nodes, gs.n_edges, gs.n_graphs, tw, nv, arr(ps[:8]),
                                      arr(ps[8:]) if gated else None, 0 if form == 'residual' else 1, 1e-5, ptr(dh), arr(grads[:8]),
                                      arr(grads[8:]) if gated else None, ptr(ws), ws.numel(), current_stream()), 'msmp_mp_layer_bwd_f32')
        check(L.msmp_tune(b'bwd_gemm', prev), 'tune')
        # without the by-source arrays dh is scattered with float atomics: its bits are not fixed from run to run, so only the gradients count
        res[f'layer_bwd {form} graphs={graphs} tw={tw} nv={nv} by_source={int(by_source)} bwd_gemm={bwd_gemm}'] = digest(([dh] if by_source else []) + grads)
    for width in (164, 256):
        gs = structures[2]
        (gout, h, u, pos, var), ps = layer_inputs(gs, width, 25, 1, True)
        dh, grads = A.layer_backward_wide_native(gout, h, u, pos, var, gs, ps, True, 1e-5)
        res[f'wide_layer_bwd gated W={width}'] = digest([dh] + grads)

    g = torch.Generator().manual_seed(7)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    for k, n_out, mode in [(k, 164, mode) for k in (5, 333) for mode in (0, 1, 2)]:
        ldx, ld_out = (k + 3) // 4 * 4, 128 * ((n_out + 127) // 128)
        x, w, b, y = r(200, ldx), r(n_out, k) / k ** 0.5, r(n_out), r(200, ld_out)
        ws = torch.empty(L.msmp_linear_workspace_bytes(k, n_out), dtype=torch.uint8, device='cuda')
        check(L.msmp_linear_f32(ptr(x), ldx, 200, k, ptr(w), k, ptr(b), n_out, mode, ptr(y), ld_out, ptr(ws), ws.numel(), current_stream()), 'msmp_linear_f32')
        res[f'linear k={k} n_out={n_out} mode={mode}'] = digest([y])
    x, w, b, y = r(200, 128), r(256, 128) / 128 ** 0.5, r(256), torch.empty(200, 256, device='cuda')
    ws = torch.empty(L.msmp_linear_swish_workspace_bytes(128, 256), dtype=torch.uint8, device='cuda')
    check(L.msmp_linear_swish_f32(ptr(x), 200, 128, ptr(w), ptr(b), 256, ptr(y), ptr(ws), ws.numel(), current_stream()), 'msmp_linear_swish_f32')
    res['linear_swish k=128 n_out=256'] = digest([y])
    res['colsum 1000x164 group=4'] = digest([reductions.colsum(r(1000, 164), 4)])
    res['sqerr_sum 12345'] = digest([reductions.sqerr_sum(r(12345), r(12345))])

    # 50 tensors: more than ADAMW_MAX_TENSORS = 48, i.e. two launches; sizes on both sides of the 4096-element chunk
    for name, kw in (('eager', {}), ('capturable', dict(capturable=True)), ('guarded', dict(capturable=True, skip_nonfinite=True)),
                     ('guarded NaN gradient', dict(capturable=True, skip_nonfinite=True))):
        ps = [torch.nn.Parameter(r(1 + 977 * (i % 7) + 5000 * (i == 49))) for i in range(50)]
        opt = optim.AdamW(ps, lr=1e-3, **kw)
        for step in range(2):
            for p in ps:
                p.grad = r(*p.shape)
            if 'NaN' in name and step == 1:
                ps[17].grad[3] = float('nan')
            opt.step()
        extra = [opt.param_groups[0]['_msmp_dev'][key] for key in (('step', 'verdict', 'skipped') if 'guarded' in name else ('step',) if kw else ())]
        res[f'adamw {name}'] = digest(ps + [opt.state[p][key] for p in ps for key in ('exp_avg', 'exp_avg_sq')] + extra)
    json.dump(res, open(out, 'w'))


def child(graphs, out):
    sys.path.insert(0, ROOT)
    import argparse, torch, bench
    import msmp_pde_amd as mp
    dev = torch.device('cuda:0')
    res = {}
    for exp, model in CASES:
        a = bench.parse(['--experiment', exp, '--model', model, '--graphs', str(graphs)])
        w = bench.Workload(a, mp, dev, graphs, seed=1)
        with torch.no_grad():
            w.first(); w.step(); w.step()
        torch.cuda.synchronize()
        p = w.pred.float().cpu().contiguous()
        res[f'{exp}/{model}'] = hashlib.sha256(p.numpy().tobytes()).hexdigest()
        torch.save(p, f'{out}.{exp}.{model}.pt')
    json.dump(res, open(out, 'w'))


if __name__ == '__main__':
    if sys.argv[1] == '--child':
        mode, out = sys.argv[2:4]
        encoder_child(out) if mode == 'encoders' else training_child(out) if mode == 'training' else child(int(mode), out)
        sys.exit(0)
    libs = [a for a in sys.argv[1:] if a.endswith('.so')]
    graphs = int(sys.argv[sys.argv.index('--graphs') + 1]) if '--graphs' in sys.argv else 64
    encoders = 'training' if '--training' in sys.argv else 'encoders' if '--encoders' in sys.argv else ''
    outs = []
    for i, l in enumerate(libs):
        out = f'/tmp/ab_identity_{i}.json'
        env = dict(os.environ, MSMP_LIB_PATH=os.path.join(ROOT, 'msmp-pde_amd', l))
        r = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.abspath(__file__), '--child', encoders or str(graphs), out],
                           env=env, capture_output=True, text=True)
        if r.returncode:
            print(l, 'FAILED', r.stderr[-1500:]); sys.exit(1)
        outs.append(json.load(open(out)))
    import torch
    ok = True
    for k in outs[0]:
        for i in range(1, len(libs)):
            same = outs[i][k] == outs[0][k]
            msg = f'bit-identical (sha256 {outs[0][k][:16]})'
            if not same and encoders:
                msg, ok = 'DIFFERENT', False
            elif not same:
                exp, model = k.split('/')
                a = torch.load(f'/tmp/ab_identity_0.json.{exp}.{model}.pt'); b = torch.load(f'/tmp/ab_identity_{i}.json.{exp}.{model}.pt')
                msg = f'DIFFERENT: max |a - b| = {(a - b).abs().max().item():.3e} (max |a| = {a.abs().max().item():.3e}), nan {int(torch.isnan(b).sum())}'
                ok = False
            print(f'{k:44s} {libs[0]} vs {libs[i]}: {msg}', flush=True)
    sys.exit(0 if ok else 2)
