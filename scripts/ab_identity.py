"""Do two (or more) builds of the library give the same bits?  Run on the GPU box:
    python scripts/ab_identity.py libmsmp_pde.so libmsmp_pde_v3.so [--graphs 64] [--encoders]
Each library (a path relative to the package, or absolute) runs in its own process (MSMP_LIB_PATH), under its own time limit, on the same seeded
workloads (E2 / WE3 / RPU / MSWG3, MSMP-PDE classes: two rollout steps) and prints a SHA-256 of the predictions; this parent compares them
and, where they differ, prints the largest difference (so a numerics-preserving but not bit-identical change is told apart from a wrong one).
It stops at the first child that does not exit 0.
--encoders: the recurrent encoders under autograd instead (ENCODER_CASES: the LEM and LSTM training pairs through their raw entries and their
Functions; final states, the whole `saved` and dG buffers and the four parameter gradients are hashed).  The package of this tree drives every
library, so a difference isolates the device side."""
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
        encoder_child(sys.argv[3]) if sys.argv[2] == 'encoders' else child(int(sys.argv[2]), sys.argv[3])
        sys.exit(0)
    libs = [a for a in sys.argv[1:] if a.endswith('.so')]
    graphs = int(sys.argv[sys.argv.index('--graphs') + 1]) if '--graphs' in sys.argv else 64
    encoders = '--encoders' in sys.argv
    outs = []
    for i, l in enumerate(libs):
        out = f'/tmp/ab_identity_{i}.json'
        env = dict(os.environ, MSMP_LIB_PATH=os.path.join(ROOT, 'msmp-pde_amd', l))
        r = subprocess.run(['timeout', '-k', '10', '300', sys.executable, os.path.abspath(__file__), '--child', 'encoders' if encoders else str(graphs), out],
                           env=env, capture_output=True, text=True)
        if r.returncode:
            print(l, 'FAILED', r.stderr[-1500:]); sys.exit(1)
        outs.append(json.load(open(out)))
    import torch
    ok = True
    for k in outs[0]:
        for i in range(1, len(libs)):
            same = outs[i][k] == outs[0][k]
            msg = 'bit-identical'
            if not same and encoders:
                msg, ok = 'DIFFERENT', False
            elif not same:
                exp, model = k.split('/')
                a = torch.load(f'/tmp/ab_identity_0.json.{exp}.{model}.pt'); b = torch.load(f'/tmp/ab_identity_{i}.json.{exp}.{model}.pt')
                msg = f'DIFFERENT: max |a - b| = {(a - b).abs().max().item():.3e} (max |a| = {a.abs().max().item():.3e}), nan {int(torch.isnan(b).sum())}'
                ok = False
            print(f'{k:44s} {libs[0]} vs {libs[i]}: {msg}', flush=True)
    sys.exit(0 if ok else 2)
