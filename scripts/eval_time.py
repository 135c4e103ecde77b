"""Time of one evaluation pass over a split: the reference's three loops restated over GraphCreator against evaluate.test, alternating
inside ONE job, on an E2-shaped split (nt 250, nx 100, tw 25, batch 16, 128 samples; MSMP-PDE) and on MSWG3 (the same sizes, two
components; MSMP-PDE2D).

    A   test_timestep_losses + test_unrolled_losses + compute_L2_norms (experiments/train_helper.py:150-296, :362-471) as the reference
        writes them, over msmp_pde_amd.GraphCreator on a split that is already on the device (u_all[i0:i1]: no loader, no host copy
        of trajectories): create_data, create_graph / create_next_graph, model(graph), a float32 MSELoss(reduction='sum') per forward,
        the host reads the reference makes (the printed mean per step, the two .item() of compute_L2_norms), and the second rollout
        compute_L2_norms needs.  The numerical-baseline half of test_unrolled_losses (:279-289) is left out of A (B caches it).
    B   evaluate.test(model, creator, dataset, ...): timestep losses, ONE rollout, both metrics, one read-back.

    python scripts/eval_time.py                  the table: ms per pass for A and B, forwards per pass, and the eval kernel by events
    python scripts/eval_time.py kernel EXP       only the kernel, 200 launches: for a kernel trace (rocprofv3 --kernel-trace --stats) of its own
Every number is a median over rounds after warm-up; the spread over the rounds is printed beside it."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import msmp_pde_amd as mp
from msmp_pde_amd import evaluate as E
from msmp_pde_amd.synthetic import make_case, EXPERIMENTS

SAMPLES, BATCH, NT, NX, TW, NR_GT = 128, 16, 250, 100, 25, 1
CONFIGS = [('E2', 'MSMP-PDE'), ('MSWG3', 'MSMP-PDE2D')]
HBM = 6.3e12          # bytes / s the project takes as achievable


def setup(exp, name, seed=1):
    c = make_case(exp, SAMPLES, seed=seed, device='cuda', nt=NT, nx=NX, tw=TW, dtype=torch.float32)
    store = c.u_super if c.u_super.dim() == 4 else c.u_super[:, :, None, :]
    variables = {k: v.float() for k, v in c.variables.items()}
    ds = mp.DeviceDataset(c.pde, store, c.x[0], variables, 'cuda')
    torch.manual_seed(1)
    model = mp.MODEL_NAMES[name](c.pde, time_window=TW, eq_variables=EXPERIMENTS[exp], hidden_layer=6).cuda().eval()
    x32 = c.x[0].float().cuda()
    loader = [(c.u_super[i:i + BATCH], x32[None].repeat(len(c.u_super[i:i + BATCH]), 1), {k: v[i:i + BATCH] for k, v in variables.items()})
              for i in range(0, SAMPLES, BATCH)]
    return c, ds, model, loader


def reference_pass(model, creator, loader, counts):
    """Route A.  Returns (mean unrolled loss, L2 abs, L2 rel) as the reference's functions do."""
    criterion = torch.nn.MSELoss(reduction='sum')
    tw, nt, nx = creator.tw, creator.t_res, NX
    d = 2 if f'{creator.pde}' == 'AD' else 1
    model.eval()
    with torch.no_grad():
        for step in range(tw, nt - tw + 1):                                   # test_timestep_losses
            if step != tw and step % tw != 0:
                continue
            losses = []
            for u, x, variables in loader:
                same_steps = [step] * len(u)
                data, labels = creator.create_data(u, same_steps)
                graph = creator.create_graph(data, labels, x, variables, same_steps)
                losses.append(criterion(model(graph), graph.y) / BATCH)
                counts[0] += 1
            float(torch.mean(torch.stack(losses)))                            # print(f'Step {step}, mean loss {...}')
        losses = []
        for u, x, variables in loader:                                        # test_unrolled_losses
            tmp = []
            for w, step in enumerate(range(tw * NR_GT, nt - tw + 1, tw)):
                same_steps = [step] * len(u)
                data, labels = creator.create_data(u, same_steps)
                graph = creator.create_graph(data, labels, x, variables, same_steps) if w == 0 else creator.create_next_graph(graph, pred, labels, same_steps)
                pred = model(graph)
                counts[0] += 1
                tmp.append(criterion(pred, graph.y) / nx / BATCH)
            losses.append(torch.sum(torch.stack(tmp)))
        unrolled = float(torch.mean(torch.stack(losses)))                     # print(f'Unrolled forward losses {...}')
        all_l, all_n = [], []
        for u, x, variables in loader:                                        # compute_L2_norms
            b = len(u)
            l_t, n_t = [], []
            for w, step in enumerate(range(tw * NR_GT, nt - tw + 1, tw)):
                same_steps = [step] * b
                data, labels = creator.create_data(u, same_steps)
                graph = creator.create_graph(data, labels, x, variables, same_steps) if w == 0 else creator.create_next_graph(graph, pred, labels, same_steps)
                pred = model(graph)
                counts[0] += 1
                l_t.append(torch.square(pred - graph.y).unflatten(0, (b, nx)).permute(0, 2, 1).unflatten(1, (tw, d)))
                n_t.append(torch.square(graph.y).unflatten(0, (b, nx)).permute(0, 2, 1).unflatten(1, (tw, d)))
            all_l.append(torch.cat(l_t, 1)), all_n.append(torch.cat(n_t, 1))
        losses, norms = torch.cat(all_l, 0), torch.cat(all_n, 0)
        losses, norms = torch.sqrt(torch.sum(losses, 2).mean((1, 2))).mean(), torch.sqrt(torch.sum(norms, 2).mean((1, 2))).mean()
        return unrolled, losses.item(), (losses / norms).item()


def alternate(runs, rounds):
    times = {k: [] for k in runs}
    for run in runs.values():
        run()
    for _ in range(rounds):
        for k, run in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) * 1e3)
    return times


def kernel_setup(ds):
    cols = ds.comps * TW
    idx = torch.arange(BATCH, dtype=torch.int32, device='cuda')
    stp = torch.full((BATCH,), 3 * TW, dtype=torch.int32, device='cuda')
    pred = torch.randn(BATCH * NX, cols, device='cuda')
    err = torch.empty(BATCH, cols, dtype=torch.float64, device='cuda')
    nrm = torch.empty_like(err)
    pos = torch.zeros(BATCH * NX, 2, device='cuda')
    moved = 2 * BATCH * NX * cols * 4 + 2 * BATCH * cols * 8 + BATCH * NX * 4          # window + pred read; two tables and the time column written
    return (lambda: E.window_errors(ds, idx, stp, pred, TW, err=err, nrm=nrm, pos=pos)), moved


def kernel_by_events(ds, n=200):
    """us per launch of n back-to-back launches between two events: an upper bound of the kernel's own time (it includes the gaps
    between launches); the kernel trace of `kernel EXP` gives the time without them."""
    run, moved = kernel_setup(ds)
    for _ in range(20):
        run()
    per = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            run()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) / n * 1e3)
    return statistics.median(per), moved


def table():
    print(f'device: {torch.cuda.get_device_name(0)}; split of {SAMPLES} samples on the device, nt {NT}, nx {NX}, tw {TW}, batch {BATCH}, '
          f'nr_gt_steps {NR_GT}; ms per evaluation pass, median of 5 rounds', flush=True)
    for exp, name in CONFIGS:
        c, ds, model, loader = setup(exp, name)
        counts, calls = [0], [0]
        hook = model.register_forward_hook(lambda m, i, o: calls.__setitem__(0, calls[0] + 1))
        out = {}

        def run_a():
            out['A'] = reference_pass(model, c.creator, loader, counts)

        def run_b():
            out['B'] = E.test(model, c.creator, ds, BATCH, NR_GT, NX)
        run_a()
        fwd_a, calls[0] = counts[0], 0
        run_b()
        fwd_b = calls[0]
        hook.remove()
        t = alternate({'A': run_a, 'B': run_b}, rounds=5)
        a, b = statistics.median(t['A']), statistics.median(t['B'])
        ua, la, ra = out['A']
        rb = out['B']
        print(f'evaluation pass  {name:10s} {exp:6s}: A {a:8.2f} ms [{min(t["A"]):.2f}..{max(t["A"]):.2f}] ({fwd_a} forwards)  '
              f'B {b:8.2f} ms [{min(t["B"]):.2f}..{max(t["B"]):.2f}] ({fwd_b} forwards)  A/B {a / b:5.2f}x', flush=True)
        print(f'    results  A (float32 loss): unrolled {ua:.9g}  L2 {la:.9g}  rel {ra:.9g}    B: unrolled {rb.unrolled:.9g}  L2 {rb.l2_abs:.9g}  '
              f'rel {rb.l2_rel:.9g}', flush=True)
        us, moved = kernel_by_events(ds)
        floor = moved / HBM * 1e6
        print(f'    eval kernel {exp:6s} batch {BATCH}: {us:6.2f} us per launch between events (200 back-to-back launches); '
              f'{moved / 1e3:.1f} kB moved -> HBM floor {floor:.3f} us at 6.3 TB/s; ratio {us / floor:.0f}x', flush=True)
        del c, ds, model, loader


def kernel(exp):
    c, ds, model, loader = setup(exp, dict(CONFIGS)[exp])
    run, moved = kernel_setup(ds)
    for _ in range(200):
        run()
    torch.cuda.synchronize()
    print(f'kernel run {exp} batch {BATCH}: 200 launches done, {moved} bytes moved per launch', flush=True)


if __name__ == '__main__':
    if sys.argv[1:2] == ['kernel']:
        kernel(sys.argv[2])
    else:
        table()
