"""Wall time of one training iteration (train.training_step: pushforward unroll under no_grad + forward/backward + AdamW)
on the HIP forward / native backward path, E2, reference batch size 16 and larger.  Optimizer: msmp_pde_amd.optim.AdamW
(msmp_adamw_f32; `--torch-adamw` times torch.optim.AdamW(fused=True) instead).

    --model NAME          one model of msmp_pde_amd.MODEL_NAMES (repeatable; default MSMP-PDE, Gated, MP-PDE)
    --batches 16,512      batch sizes (default 16,128,512)
    --warmup W --iters N  untimed and timed iterations per (model, batch) (default 4 and 5)
    --tune KEY=VALUE      an msmp_tune switch for the whole process (repeatable), e.g. --tune lem_wide_train=1
    --exp NAME            the experiment of msmp_pde_amd.synthetic.EXPERIMENTS (default E2; MSWG3 for the *2D classes)"""
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
args = ap.parse_args()
for kv in args.tune:
    key, value = kv.split('=')
    assert mp.lib().msmp_tune(key.encode(), int(value)) == 0, mp.lib().msmp_last_error()
variants = [(name, True) for name in (args.model or ['MSMP-PDE', 'Gated', 'MP-PDE'])]
TORCH_ADAMW = args.torch_adamw
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
