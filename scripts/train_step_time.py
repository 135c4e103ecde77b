"""Wall time of one training iteration (train.training_step: pushforward unroll under no_grad + forward/backward + AdamW)
on the HIP forward / native backward path, E2, reference batch size 16 and larger.  Optimizer: msmp_pde_amd.optim.AdamW
(msmp_adamw_f32; `--torch-adamw` times torch.optim.AdamW(fused=True) instead).

    --model NAME          one model of msmp_pde_amd.MODEL_NAMES (repeatable; default MSMP-PDE, Gated, MP-PDE)
    --batches 16,512      batch sizes (default 16,128,512)
    --warmup W --iters N  untimed and timed iterations per (model, batch) (default 4 and 5)
    --tune KEY=VALUE      an msmp_tune switch for the whole process (repeatable), e.g. --tune lem_wide_train=1
    --exp NAME            the experiment of msmp_pde_amd.synthetic.EXPERIMENTS (default E2; MSWG3 for the *2D classes)
    --ab KEY              A/B of one msmp_tune switch INSIDE the process (the boxes of a pool differ by more than most switches do): per
                          (model, batch) the switch alternates 0, 1, 0, 1, ... for --rounds rounds of --iters timed iterations each; prints
                          the median per setting, their difference, and the spread between two runs of the same setting (the largest
                          distance of a run from its setting's median).  One of dec_bwd, g2_gate, lem_wide_train, lstm_train, mlp_train, wide_bwd.
    --rounds R            alternations of --ab (default 5)
    --captured            with --ab: the iteration as train.CapturedTrainStep replays (one capture per setting) instead of eager"""
import argparse
import sys, os, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import msmp_pde_amd as mp
from msmp_pde_amd.synthetic import make_case, EXPERIMENTS
from msmp_pde_amd.train import training_step
from msmp_pde_amd.lem import LEM
ap = argparse.ArgumentParser()
ap.add_argument('--model', action='append')
ap.add_argument('--batches', default='16,128,512')
ap.add_argument('--warmup', type=int, default=4)
ap.add_argument('--iters', type=int, default=5)
ap.add_argument('--tune', action='append', default=[])
ap.add_argument('--torch-adamw', action='store_true')
ap.add_argument('--exp', default='E2')
ap.add_argument('--ab', choices=('dec_bwd', 'g2_gate', 'lem_wide_train', 'lstm_train', 'mlp_train', 'wide_bwd'))
ap.add_argument('--rounds', type=int, default=5)
ap.add_argument('--captured', action='store_true')
args = ap.parse_args()
for kv in args.tune:
    key, value = kv.split('=')
    assert mp.lib().msmp_tune(key.encode(), int(value)) == 0, mp.lib().msmp_last_error()
variants = [(name, True) for name in (args.model or ['MSMP-PDE', 'Gated', 'MP-PDE'])]
TORCH_ADAMW = args.torch_adamw


def ab(name, bsz):
    """the --ab measurement of one (model, batch)"""
    from statistics import median
    from msmp_pde_amd.train import CapturedTrainStep
    key, L, steps = args.ab.encode(), mp.lib(), [60] * bsz
    case = make_case(args.exp, bsz, seed=1, device='cuda', dtype=torch.float32)
    before = L.msmp_tune_query(key)
    run = {}
    for value in (0, 1):                    # eager: one model per setting as well, so both settings train from the same state
        L.msmp_tune(key, value)
        torch.manual_seed(0)
        model = mp.MODEL_NAMES[name](case.pde, time_window=25, eq_variables=case.eqv, hidden_layer=6).cuda().train()
        opt = mp.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-8, capturable=args.captured)
        cap = None
        if args.captured:
            data, labels = case.creator.create_data(case.u_super, steps)
            cap = CapturedTrainStep(model, opt, case.creator.create_graph(data, labels, case.x, case.variables, steps))
        run[value] = lambda model=model, opt=opt, cap=cap: training_step(model, case.creator, case.u_super, case.x, case.variables, steps, 1, opt, captured=cap)
    times = {0: [], 1: []}
    try:
        for _ in range(args.rounds):
            for value in (0, 1):
                L.msmp_tune(key, value)
                for _ in range(args.warmup): run[value]()
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(args.iters): run[value]()
                torch.cuda.synchronize()
                times[value].append((time.perf_counter() - t0) / args.iters * 1e3)
    finally:
        L.msmp_tune(key, before)
    m = {v: median(t) for v, t in times.items()}
    spread = max(abs(t - m[v]) for v, ts in times.items() for t in ts)
    print(f'{name:11s} batch {bsz:4d} {"captured" if args.captured else "eager   "} {args.ab} 0: {m[0]:8.3f} ms  1: {m[1]:8.3f} ms  (1 - 0: {m[1] - m[0]:+.3f} ms, '
          f'{(m[1] / m[0] - 1) * 100:+.2f} %; same-setting spread {spread:.3f} ms = {spread / m[0] * 100:.2f} %; runs 0: '
          + ' '.join(f'{t:.3f}' for t in times[0]) + ' | 1: ' + ' '.join(f'{t:.3f}' for t in times[1]) + ')', flush=True)


if args.ab:
    for name, _ in variants:
        for bsz in [int(b) for b in args.batches.split(',')]:
            ab(name, bsz)
    sys.exit(0)
for name, lem_kernels in variants:
    LEM.TRAIN_KERNELS = lem_kernels
    for bsz in [int(b) for b in args.batches.split(',')]:
        torch.manual_seed(0)
        case = make_case(args.exp, bsz, seed=1, device='cuda', dtype=torch.float32)
        model = mp.MODEL_NAMES[name](case.pde, time_window=25, eq_variables=case.eqv, hidden_layer=6).cuda().train()
        opt = (torch.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-8, fused=True) if TORCH_ADAMW
               else mp.optim.AdamW(model.parameters(), lr=1e-4, weight_decay=1e-8))
        steps = [60] * bsz
        for _ in range(args.warmup): training_step(model, case.creator, case.u_super, case.x, case.variables, steps, 1, opt)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        n = args.iters
        for _ in range(n): loss = training_step(model, case.creator, case.u_super, case.x, case.variables, steps, 1, opt)
        torch.cuda.synchronize()
        tuned = ''.join(f' [{kv}]' for kv in args.tune)
        print(f'{name:9s}{"" if lem_kernels else " (LEM in PyTorch)"}{tuned} batch {bsz:4d}: {(time.perf_counter() - t0) / n * 1e3:8.2f} ms per training iteration (1 unrolled step), loss {float(loss):.4f}', flush=True)
