"""CPU tests of msmp_pde_amd.evaluate against the REFERENCE's own evaluation loops: tests/golden/eval_{CE,AD}.npz hold what
test_timestep_losses, test_unrolled_losses and compute_L2_norms (experiments/train_helper.py) returned for seeded arrays and a stub model
whose forward is a closed form of data.x and data.pos (tests/golden/gen_golden_eval.py).  The same rollout is rebuilt here on the CPU
path of `evaluate` -- a DeviceDataset with device='cpu', the PyTorch restatement of the kernel's formulas -- and every number agrees to
1e-12 relative: the reference ran in float64 and the trajectories are float32-representable, so only the order of summation differs.
S = 5 in batches of 2: the last batch holds one sample."""
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
RTOL = 1e-12
VARS = {'CE': ('alpha', 'beta', 'gamma'), 'AD': ('a', 'b')}


class Stub(torch.nn.Module):
    """pred = tanh(x) A + sin(pos[:, 0:1]) b_t + cos(pos[:, 1:2]) b_x + d in float64: the generator's stub, from its stored coefficients."""

    def __init__(self, g):
        super().__init__()
        self.A, self.bt, self.bx, self.d = (torch.from_numpy(g['coef_' + k]) for k in ('A', 'bt', 'bx', 'd'))
        self.calls = 0

    def __repr__(self):
        return 'GNN'

    def forward(self, data):
        self.calls += 1
        x, pos = data.x.double(), data.pos.double()
        return torch.tanh(x) @ self.A + torch.sin(pos[:, 0:1]) * self.bt + torch.cos(pos[:, 1:2]) * self.bx + self.d


@pytest.fixture(scope='module', params=['CE', 'AD'])
def case(request):
    import msmp_pde_amd as mp
    name = request.param
    g = np.load(os.path.join(GOLDEN, f'eval_{name}.npz'))
    u = torch.from_numpy(g['u_super'])
    assert torch.equal(u.float().double(), u)                     # float32-representable: the float32 store loses nothing
    nt, nx, tw = u.shape[1], u.shape[-1], int(g['tw'])
    pde = (mp.CE if name == 'CE' else mp.AD)(tmin=float(g['tmin']), tmax=float(g['tmax']), grid_size=[nt, nx], L=float(g['L']))
    store = u if name == 'AD' else u[:, :, None, :]
    variables = {k: g['var_' + k] for k in VARS[name]}
    ds = mp.DeviceDataset(pde, store, g['x'], variables, 'cpu', u_base=g['u_base'])
    creator = mp.GraphCreator(pde, neighbors=2, time_window=tw, t_resolution=nt, x_resolution=nx)
    return mp.evaluate, g, ds, creator, Stub(g), int(g['batch_size'])


def close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    rel = np.abs(got - want) / np.abs(want)
    print('largest relative difference', rel.max())
    assert (rel <= RTOL).all(), (got, want, rel)


@pytest.mark.parametrize('nr_gt_steps', [1, 2])
def test_unrolled_losses_and_l2_norms_are_the_references(case, nr_gt_steps):
    E, g, ds, creator, model, bs = case
    model.calls = 0
    err, nrm = E.rollout(model, creator, ds, bs, nr_gt_steps)
    windows = len(range(creator.tw * nr_gt_steps, ds.nt - creator.tw + 1, creator.tw))
    assert err.dtype == nrm.dtype == torch.float64 and tuple(err.shape) == tuple(nrm.shape) == (5, windows, ds.comps * creator.tw)
    assert model.calls == 3 * windows                              # ONE rollout: batches of 2, 2 and 1 samples
    losses = E.unrolled_losses(err, bs, ds.nx)
    assert losses.dtype == torch.float64 and tuple(losses.shape) == (3,)
    close(losses, g[f'unrolled_{nr_gt_steps}'])
    l2_abs, l2_rel = E.l2_norms(err, nrm, ds.nx, comps=ds.comps)
    close([float(l2_abs), float(l2_rel)], g[f'l2_{nr_gt_steps}'])
    assert model.calls == 3 * windows                              # ... feeds both metrics


@pytest.mark.parametrize('nr_gt_steps', [1, 2])
def test_base_losses_are_the_references_and_are_computed_once(case, nr_gt_steps):
    E, g, ds, creator, model, bs = case
    base = E.base_losses(ds, creator, bs, nr_gt_steps, ds.nx)
    assert base.dtype == torch.float64
    close(base, g[f'base_{nr_gt_steps}'])
    assert E.base_losses(ds, creator, bs, nr_gt_steps, ds.nx) is base


def test_base_losses_need_u_base(case):
    import msmp_pde_amd as mp
    E, g, ds, creator, model, bs = case
    bare = mp.DeviceDataset(ds.pde, ds.store, ds.x, ds.variables, 'cpu')
    with pytest.raises(ValueError, match='u_base'):
        E.base_losses(bare, creator, bs, 1, ds.nx)


def test_timestep_losses_are_the_means_the_reference_prints(case):
    E, g, ds, creator, model, bs = case
    model.calls = 0
    got = E.timestep_losses(model, creator, ds, bs)                # default steps: tw .. nt - tw, filtered by the reference's rule
    assert list(got) == g['steps'].tolist()
    assert model.calls == 3 * len(got)                             # one forward per (step, batch)
    close([float(got[s]) for s in got], g['timestep_means'])
    some = E.timestep_losses(model, creator, ds, bs, steps=[creator.tw, creator.tw + 1, 3 * creator.tw])
    assert list(some) == [creator.tw, 3 * creator.tw]
    close([float(some[s]) for s in some], g['timestep_means'][[0, 2]])


def test_test_returns_everything_as_host_numbers(case):
    E, g, ds, creator, model, bs = case
    model.train()
    r = E.test(model, creator, ds, bs, 1, ds.nx)
    assert not model.training                                      # model.eval(), experiments/train.py:270
    close(r.unrolled, g['unrolled_1'].mean())
    close([r.l2_abs, r.l2_rel], g['l2_1'])
    close(r.base, g['base_1'].mean())
    close([r.timestep[s] for s in g['steps'].tolist()], g['timestep_means'])
    assert all(isinstance(v, float) for v in (r.unrolled, r.l2_abs, r.l2_rel, r.base) + tuple(r.timestep.values()))


def test_window_errors_restatement_marks_bad_indices_and_writes_the_next_time(case):
    """The PyTorch restatement on its own: NaN entries for a graph whose index or step is out of range, the others untouched; pos[:, 0]
    becomes t[p + tw] only where p + tw still starts a window; padded tables keep their padding."""
    E, g, ds, creator, model, bs = case
    tw, nx, cols = creator.tw, ds.nx, ds.comps * creator.tw
    gen = torch.Generator().manual_seed(3)
    pred = torch.randn(4 * nx, cols, generator=gen, dtype=torch.float64)
    idx, steps = [4, 0, 2, 1], [tw, ds.nt - tw, 2 * tw + 1, ds.nt - 2 * tw]
    pos = torch.full((4 * nx, 2), -7.0, dtype=torch.float64)
    table = torch.full((2, 4, cols + 3), -5.0, dtype=torch.float64)
    err, nrm = E.window_errors(ds, idx, steps, pred, tw, err=table[0, :, :cols], nrm=table[1, :, :cols], pos=pos)
    assert (table[:, :, cols:] == -5.0).all() and err.data_ptr() == table.data_ptr()
    for b, (s, p) in enumerate(zip(idx, steps)):
        y = ds.store[s, p:p + tw].double().permute(2, 1, 0).reshape(nx, cols)
        close(err[b], (pred[b * nx:(b + 1) * nx] - y).square().sum(0))
        close(nrm[b], y.square().sum(0))
        want_t = float(ds.t[p + tw]) if p + tw <= ds.nt - tw else -7.0
        assert (pos[b * nx:(b + 1) * nx, 0] == want_t).all() and (pos[b * nx:(b + 1) * nx, 1] == -7.0).all()
    for bad_idx, bad_steps in (([4, -1, 2, 1], steps), ([4, 5, 2, 1], steps), (idx, [tw, tw - 1, 2 * tw + 1, ds.nt - 2 * tw]),
                               (idx, [tw, ds.nt - tw + 1, 2 * tw + 1, ds.nt - 2 * tw])):
        e2, n2 = E.window_errors(ds, torch.tensor(bad_idx), torch.tensor(bad_steps), pred, tw)
        assert torch.isnan(e2[1]).all() and torch.isnan(n2[1]).all()
        keep = [0, 2, 3]
        assert torch.equal(e2[keep], err[keep]) and torch.equal(n2[keep], nrm[keep])
