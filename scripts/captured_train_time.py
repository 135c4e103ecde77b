"""Optimisation step (forward + loss + backward + AdamW on a prepared batch; experiments/train_helper.py:125-141) eager vs as one
hipGraph launch (train.CapturedTrainStep), E2, the reference's batch size 16 and larger ones.
    python scripts/captured_train_time.py [batch sizes ...]
    python scripts/captured_train_time.py guard [batch sizes ...]     the cost of optim.AdamW(skip_nonfinite=True) and of range_policy
        'auto' / 'sync' (train.py): every variant is built first, then they are timed in turn, several rounds inside the one job
        (boxes differ by a few percent), and the median round is printed; 'off' is the step without the guard."""
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import msmp_pde_amd as mp
from msmp_pde_amd import train as T
from msmp_pde_amd.synthetic import make_case, EXPERIMENTS
sizes = [int(a) for a in sys.argv[1:] if a.isdigit()] or [16, 64]
names = [a for a in sys.argv[1:] if a in mp.MODEL_NAMES] or ['MSMP-PDE', 'Gated', 'MP-PDE']
modes = [a for a in sys.argv[1:] if a in ('eager', 'captured')] or ['eager', 'captured']


def guard_cost(name, bsz, rounds=5, n=20):
    import statistics
    torch.manual_seed(0)
    case = make_case('E2', bsz, seed=1, device='cuda', dtype=torch.float32)
    steps = [60] * bsz
    data, labels = case.creator.create_data(case.u_super, steps)
    graph = case.creator.create_graph(data, labels, case.x, case.variables, steps)
    runs = {}
    for mode in modes:
        for policy in ('off', 'auto', 'sync'):
            torch.manual_seed(1)
            model = mp.MODEL_NAMES[name](case.pde, time_window=25, eq_variables=EXPERIMENTS['E2'], hidden_layer=6).cuda().train()
            opt = mp.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-8, capturable=True, skip_nonfinite=policy != 'off')
            rp = None if policy == 'off' else policy
            if mode == 'captured':
                step = T.CapturedTrainStep(model, opt, graph, range_policy=rp)
                run = (lambda step: lambda: step(graph))(step)
            elif rp is None:
                def run(model=model, opt=opt):
                    opt.zero_grad(set_to_none=True)
                    loss = T.dp_loss_backward(model, graph)
                    opt.step()
                    return loss
            else:
                run = (lambda model, opt, rp: lambda: T._guarded_eager_step(model, graph, opt, rp))(model, opt, rp)
            for _ in range(3): run()
            runs[mode, policy] = run
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, run in runs.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for _ in range(n): run()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / n * 1e3)
    for mode in modes:
        off = statistics.median(times[mode, 'off'])
        print(f'{name:9s} batch {bsz:4d} {mode:8s}: ' + ', '.join(f'{pol} {statistics.median(times[mode, pol]):7.3f} ms ({100 * (statistics.median(times[mode, pol]) / off - 1):+5.1f} %)'
                                                              for pol in ('off', 'auto', 'sync'))
              + f'   [rounds min..max of off: {min(times[mode, "off"]):.3f}..{max(times[mode, "off"]):.3f}]', flush=True)


if 'guard' in sys.argv[1:]:
    for name in ([a for a in sys.argv[1:] if a in mp.MODEL_NAMES] or ['MSMP-PDE']):
        for bsz in (sizes if any(a.isdigit() for a in sys.argv[1:]) else [16, 512]):
            guard_cost(name, bsz)
    sys.exit(0)
for name in names:
    for bsz in sizes:
        torch.manual_seed(0)
        case = make_case('E2', bsz, seed=1, device='cuda', dtype=torch.float32)
        steps = [60] * bsz
        data, labels = case.creator.create_data(case.u_super, steps)
        graph = case.creator.create_graph(data, labels, case.x, case.variables, steps)
        res = {}
        for mode in modes:
            torch.manual_seed(1)
            model = mp.MODEL_NAMES[name](case.pde, time_window=25, eq_variables=EXPERIMENTS['E2'], hidden_layer=6).cuda().train()
            opt = mp.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-8, capturable=True)
            if mode == 'captured':
                step = T.CapturedTrainStep(model, opt, graph)
                run = lambda: step(graph)
            else:
                def run():
                    opt.zero_grad(set_to_none=True)
                    loss = T.dp_loss_backward(model, graph)
                    opt.step()
                    return loss
                for _ in range(3): run()
            torch.cuda.synchronize(); t0 = time.perf_counter()
            n = 20
            for _ in range(n): loss = run()
            torch.cuda.synchronize()
            res[mode] = ((time.perf_counter() - t0) / n * 1e3, float(loss))
        print(f'{name:9s} batch {bsz:4d}: ' + ', '.join(f'{m} {res[m][0]:7.2f} ms' for m in modes) + ' per optimisation step (loss after the timed steps '
              + ' / '.join(f'{res[m][1]:.5f}' for m in modes) + ')', flush=True)
