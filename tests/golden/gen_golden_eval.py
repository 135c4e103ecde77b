#!/usr/bin/env python3
"""Generate tests/golden/eval_{CE,AD}.npz from the REFERENCE's own evaluation loops: test_timestep_losses, test_unrolled_losses and
compute_L2_norms (experiments/train_helper.py:150-296, :362-471) over the reference's GraphCreator (common/utils.py:267-471).

Runs only where the reference tree is present (like gen_golden_dataset.py, whose stand-ins for the third-party modules it reuses):

    python tests/golden/gen_golden_eval.py

The "loader" is a list of batches shaped like the DataLoader's collation of HDF5Dataset.__getitem__: (u_base, u_super, x, variables)
with S = 5 samples in batches of 2 (so the last batch holds one), nt = 5 tw, tw = 4, nx = 10, float64 as the reference runs here.  The
model is a stub whose repr is 'GNN' and whose forward is a fixed closed form of data.x and data.pos,

    pred = tanh(x) A + sin(pos[:, 0:1]) b_t + cos(pos[:, 1:2]) b_x + d,

with the coefficients stored in the fixture: no solver weights are involved.  The trajectories are float32-representable (a
DeviceDataset keeps its store in float32), so a float64 evaluation of the same arrays differs from the reference's by summation order
only.  Each fixture holds arrays only: the inputs (`u_super`; `u_base` in the file layout, [S, 2, nt, nx] for AD; `x`; `var_<name>`;
`tmin`, `tmax`, `L`, `tw`, `batch_size`), the stub's coefficients (`coef_A`, `coef_bt`, `coef_bx`, `coef_d`), and what the reference
returned: `steps` / `timestep_means` (the means test_timestep_losses prints, taken as tensors where it formats them), and per
nr_gt_steps in (1, 2) `unrolled_<n>` (the returned per-batch losses), `l2_<n>` (abs, rel) and `base_<n>` (the per-batch base losses,
recomputed with the reference's own criterion lines :279-289 and checked against the mean it prints).  A few KB each."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF = '/root/reference'
if not os.path.isdir(REF):
    sys.exit('reference tree not present: golden vectors can only be regenerated in the build container')
sys.path.insert(0, os.path.join(HERE, 'standins'))
sys.path.insert(0, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import common.utils as U  # noqa: E402
import experiments.train_helper as TH  # noqa: E402

assert torch.get_default_dtype() == torch.float64  # side effect of temporal/solvers.py:10

S, BATCH, TW, NX = 5, 2, 4, 10
NT = 5 * TW
TMIN, TMAX, LENGTH = 0.0, 0.25 * (NT - 1), 16.0
VARIABLES = {'CE': ('alpha', 'beta', 'gamma'), 'AD': ('a', 'b')}


class Named(object):
    """What GraphCreator reads of a PDE: its name, time interval and grid."""

    def __init__(self, name):
        self.name, self.untructured_grid = name, False
        self.tmin, self.tmax, self.L, self.grid_size = TMIN, TMAX, LENGTH, (NT, NX)

    def __repr__(self):
        return self.name


class Stub(torch.nn.Module):
    def __init__(self, A, bt, bx, d):
        super().__init__()
        self.A, self.bt, self.bx, self.d = (torch.as_tensor(v) for v in (A, bt, bx, d))

    def __repr__(self):
        return 'GNN'

    def forward(self, data):
        x, pos = data.x.double(), data.pos.double()
        return torch.tanh(x) @ self.A + torch.sin(pos[:, 0:1]) * self.bt + torch.cos(pos[:, 1:2]) * self.bx + self.d


class Recorded(object):
    """torch.mean with its results kept: the reference formats its means into strings (print(f'... {torch.mean(losses)}')), whose
    default precision is four digits, so the tensors are taken where they are made."""

    def __enter__(self):
        self.values, self._mean = [], torch.mean

        def mean(*args, **kwargs):
            out = self._mean(*args, **kwargs)
            self.values.append(out)
            return out
        torch.mean = mean
        return self.values

    def __exit__(self, *exc):
        torch.mean = self._mean


def make(name, seed):
    rng = np.random.default_rng(seed)
    comps = 2 if name == 'AD' else 1
    cols = comps * TW
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    shape = (S, NT, 2, NX) if name == 'AD' else (S, NT, NX)
    u_super = f32(rng.standard_normal(shape))
    u_base_s = f32(u_super + 0.05 * rng.standard_normal(shape))              # per-sample layout, as __getitem__ returns it
    x = 0.5 * np.arange(NX, dtype=np.float64)
    variables = {v: f32(rng.uniform(0.1, 2.0, S)) for v in VARIABLES[name]}
    coef = {'coef_A': 0.8 * np.eye(cols) + 0.1 * rng.standard_normal((cols, cols)), 'coef_bt': 0.1 * rng.standard_normal((1, cols)),
            'coef_bx': 0.1 * rng.standard_normal((1, cols)), 'coef_d': 0.05 * rng.standard_normal((1, cols))}
    model = Stub(coef['coef_A'], coef['coef_bt'], coef['coef_bx'], coef['coef_d'])
    loader = [(torch.tensor(u_base_s[i:i + BATCH]), torch.tensor(u_super[i:i + BATCH]), torch.tensor(x)[None].repeat(len(u_super[i:i + BATCH]), 1),
               {k: torch.tensor(v[i:i + BATCH]) for k, v in variables.items()}) for i in range(0, S, BATCH)]
    creator = U.GraphCreator(Named(name), neighbors=2, time_window=TW, t_resolution=NT, x_resolution=NX)
    criterion = torch.nn.MSELoss(reduction='sum')
    out = {'u_super': u_super, 'u_base': np.swapaxes(u_base_s, 1, 2) if name == 'AD' else u_base_s, 'x': x,
           'tmin': np.float64(TMIN), 'tmax': np.float64(TMAX), 'L': np.float64(LENGTH), 'tw': np.int64(TW), 'batch_size': np.int64(BATCH)}
    out.update(coef)
    out.update({'var_' + k: v for k, v in variables.items()})

    steps = [t for t in range(TW, NT - TW + 1)]                               # experiments/train.py:273
    with Recorded() as means:
        TH.test_timestep_losses(model=model, steps=steps, batch_size=BATCH, loader=loader, graph_creator=creator, criterion=criterion)
    kept = [s for s in steps if not (s != TW and s % TW != 0)]
    assert len(means) == len(kept)
    out['steps'], out['timestep_means'] = np.array(kept, dtype=np.int64), np.array([float(m) for m in means])

    for nr in (1, 2):
        with Recorded() as means:
            losses = TH.test_unrolled_losses(model=model, steps=steps, batch_size=BATCH, nr_gt_steps=nr, nx_base_resolution=NX, loader=loader,
                                             graph_creator=creator, criterion=criterion)
        assert len(means) == 2 and float(means[0]) == float(torch.mean(losses))
        base = []
        for (u_base, u_sup, _, _) in loader:                                 # experiments/train_helper.py:279-289
            tmp = []
            for step in range(creator.tw * nr, creator.t_res - creator.tw + 1, creator.tw):
                same_steps = [step] * BATCH
                _, labels_super = creator.create_data(u_sup, same_steps)
                _, labels_base = creator.create_data(u_base, same_steps)
                tmp.append(criterion(labels_super, labels_base) / NX / BATCH)
            base.append(torch.sum(torch.stack(tmp)))
        base = torch.stack(base)
        assert float(torch.mean(base)) == float(means[1])
        l2 = TH.compute_L2_norms(model=model, batch_size=BATCH, nr_gt_steps=nr, loader=loader, graph_creator=creator)
        out[f'unrolled_{nr}'], out[f'base_{nr}'], out[f'l2_{nr}'] = losses.numpy(), base.numpy(), np.array(l2)
        assert out[f'unrolled_{nr}'].dtype == np.float64 and out[f'unrolled_{nr}'].shape == (3,)
    path = os.path.join(HERE, f'eval_{name}.npz')
    np.savez(path, **out)
    print(path, {k: np.asarray(v).shape for k, v in out.items()}, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    for k, name in enumerate(('CE', 'AD')):
        make(name, 2000 + k)
