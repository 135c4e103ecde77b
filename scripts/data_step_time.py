"""Time to a ready training batch, and whole captured iterations including batch preparation: the parent's fastest path against the
device-resident dataset (msmp_pde_amd.data), E2 and MSWG3 at batch 16 and 512, alternating inside ONE job.

    A   creator.create_data + create_graph on the batch's trajectories taken from a device-resident split (u_all[idx]: the parent has
        no other way to pick samples that are already on the device), x and the parameter dict as a DataLoader hands them over
        (host float64): GraphCreator as it is.
    A0  the same without the sample selection: create_data + create_graph on ONE fixed pre-gathered batch (the most favourable
        reading of the parent: nothing picks the samples).
    B   dataset.batch(creator, indices, steps) from host lists (one pinned [2, B] copy + one launch).

    python scripts/data_step_time.py                 the table: time to a ready batch (A, A0, B) and captured MSMP-PDE iterations
    python scripts/data_step_time.py count           launches and host-to-device copies per batch (torch.profiler), a run of its own
    python scripts/data_step_time.py kernel EXP B    only B, 200 batches: for a kernel trace (rocprofv3 --kernel-trace --stats) of its own
Every number is a median over rounds after warm-up; the spread of A over the rounds is printed beside it."""
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import msmp_pde_amd as mp
from msmp_pde_amd import train as T
from msmp_pde_amd.synthetic import make_case, EXPERIMENTS

SAMPLES = 1024
CONFIGS = [('E2', 16), ('E2', 512), ('MSWG3', 16), ('MSWG3', 512)]
HBM = 6.3e12          # bytes / s the project takes as achievable


def setup(exp, bsz, seed=1):
    c = make_case(exp, SAMPLES, seed=seed, device='cuda', dtype=torch.float32)
    store = c.u_super if c.u_super.dim() == 4 else c.u_super[:, :, None, :]
    ds = mp.DeviceDataset(c.pde, store, c.x[0], c.variables, 'cuda')
    rng = random.Random(7)
    draws = [([rng.randrange(SAMPLES) for _ in range(bsz)], mp.random_steps(c.creator, bsz, 0, rng)) for _ in range(64)]
    host_vars = [{k: v[torch.tensor(idx)] for k, v in c.variables.items()} for idx, _ in draws]      # what collation hands over: [B] host float64
    x = c.x[:1].repeat(bsz, 1)
    fixed = c.u_super[torch.tensor(draws[0][0], device='cuda')].clone()
    state = {'i': 0}

    def nxt():
        state['i'] = (state['i'] + 1) % len(draws)
        return state['i']

    def run_a():
        i = nxt()
        idx, steps = draws[i]
        u = c.u_super[torch.tensor(idx, device='cuda')]
        data, labels = c.creator.create_data(u, steps)
        return c.creator.create_graph(data, labels, x, host_vars[i], steps)

    def run_a0():
        i = nxt()
        _, steps = draws[i]
        data, labels = c.creator.create_data(fixed, steps)
        return c.creator.create_graph(data, labels, x, host_vars[i], steps)

    def run_b():
        idx, steps = draws[nxt()]
        return ds.batch(c.creator, idx, steps)
    return c, ds, draws, host_vars, x, {'A': run_a, 'A0': run_a0, 'B': run_b}


def alternate(runs, rounds, n):
    times = {k: [] for k in runs}
    for k, run in runs.items():
        for _ in range(5):
            run()
    for _ in range(rounds):
        for k, run in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(n):
                run()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t0) / n * 1e3)
    return times


def med(v):
    return statistics.median(v)


def floor_us(exp, bsz, tw=25, nx=100):
    comps = 2 if exp == 'MSWG3' else 1
    n_vars = {'E2': 3, 'MSWG3': 2}[exp]
    moved = 2 * (2 * tw * comps * nx * bsz * 4) + bsz * nx * 4 * (2 + n_vars)          # window read + x, y written; pos and columns written
    return moved, moved / HBM * 1e6


def table():
    print(f'device: {torch.cuda.get_device_name(0)}; split of {SAMPLES} samples on the device; ms per batch, median of 7 rounds', flush=True)
    for exp, bsz in CONFIGS:
        c, ds, draws, host_vars, x, runs = setup(exp, bsz)
        t = alternate(runs, rounds=7, n=100 if bsz == 16 else 40)
        a, a0, b = med(t['A']), med(t['A0']), med(t['B'])
        print(f'ready batch  {exp:6s} batch {bsz:4d}: A {a:7.4f} ms [{min(t["A"]):.4f}..{max(t["A"]):.4f}]  A0 {a0:7.4f} ms [{min(t["A0"]):.4f}..{max(t["A0"]):.4f}]  '
              f'B {b:7.4f} ms [{min(t["B"]):.4f}..{max(t["B"]):.4f}]  A/B {a / b:5.1f}x  A0/B {a0 / b:5.1f}x', flush=True)
        del c, ds, runs
    for exp, bsz in CONFIGS:
        c, ds, draws, host_vars, x, _ = setup(exp, bsz)
        name = 'MSMP-PDE' if exp == 'E2' else 'MSMP-PDE2D'
        steppers = {}
        for path in ('A', 'B'):
            torch.manual_seed(1)
            model = mp.MODEL_NAMES[name](c.pde, time_window=25, eq_variables=EXPERIMENTS[exp], hidden_layer=6).cuda().train()
            opt = mp.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-8, capturable=True)
            idx, steps = draws[0]
            if path == 'A':
                data, labels = c.creator.create_data(c.u_super[torch.tensor(idx, device='cuda')], steps)
                step = T.CapturedTrainStep(model, opt, c.creator.create_graph(data, labels, x, host_vars[0], steps))
            else:
                step = T.CapturedTrainStep(model, opt, ds.batch(c.creator, idx, steps))
            steppers[path] = (model, opt, step)
        state = {'i': 0}

        def it_a():
            state['i'] = (state['i'] + 1) % len(draws)
            idx, steps = draws[state['i']]
            model, opt, step = steppers['A']
            return T.training_step(model, c.creator, c.u_super[torch.tensor(idx, device='cuda')], x, host_vars[state['i']], steps, 0, opt, captured=step)

        def it_b():
            state['i'] = (state['i'] + 1) % len(draws)
            idx, steps = draws[state['i']]
            model, opt, step = steppers['B']
            return T.dataset_training_step(model, c.creator, ds, idx, steps, 0, opt, captured=step)
        t = alternate({'A': it_a, 'B': it_b}, rounds=5, n=30 if bsz == 16 else 10)
        a, b = med(t['A']), med(t['B'])
        print(f'captured iteration incl. batch  {name:10s} {exp:6s} batch {bsz:4d}: A {a:7.3f} ms [{min(t["A"]):.3f}..{max(t["A"]):.3f}]  '
              f'B {b:7.3f} ms [{min(t["B"]):.3f}..{max(t["B"]):.3f}]  A/B {a / b:5.2f}x', flush=True)
        del steppers, c, ds
    for exp, bsz in CONFIGS:
        moved, us = floor_us(exp, bsz)
        print(f'HBM floor of the assembly  {exp:6s} batch {bsz:4d}: {moved / 1e6:7.3f} MB read + written -> {us:6.2f} us at 6.3 TB/s', flush=True)


def count():
    from torch.profiler import profile, ProfilerActivity
    for exp, bsz in CONFIGS:
        c, ds, draws, host_vars, x, runs = setup(exp, bsz)
        for k in ('A', 'A0', 'B'):
            for _ in range(5):
                runs[k]()
            torch.cuda.synchronize()
            n = 10
            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                for _ in range(n):
                    runs[k]()
                torch.cuda.synchronize()
            kernels = h2d = 0
            other = {}
            for ev in prof.events():
                if ev.device_type == torch.autograd.DeviceType.CUDA:
                    nm = ev.name.lower()
                    if 'memcpy' in nm:          # the profiler lists the copy from pinned host memory as "Memcpy DtoD"
                        if 'htod' in nm or 'hosttodevice' in nm or 'host to device' in nm:
                            h2d += 1
                        else:
                            other[ev.name] = other.get(ev.name, 0) + 1
                    else:
                        kernels += 1
            print(f'per batch  {exp:6s} batch {bsz:4d} {k:2s}: {kernels / n:5.1f} kernel launches, {h2d / n:4.1f} host-to-device copies'
                  + ''.join(f', {v / n:4.1f} x "{nm}"' for nm, v in other.items()), flush=True)
        del c, ds, runs


def kernel(exp, bsz):
    c, ds, draws, host_vars, x, runs = setup(exp, bsz)
    for _ in range(200):
        runs['B']()
    torch.cuda.synchronize()
    print(f'kernel run {exp} batch {bsz}: 200 batches done', flush=True)


if __name__ == '__main__':
    if sys.argv[1:2] == ['count']:
        count()
    elif sys.argv[1:2] == ['kernel']:
        kernel(sys.argv[2], int(sys.argv[3]))
    else:
        table()
