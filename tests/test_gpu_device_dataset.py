"""GPU tests of the device-resident dataset (msmp_pde_amd.data, msmp_batch_assemble_f32): a batch assembled by ONE launch is, bit for
bit, the batch GraphCreator.create_data + create_graph / create_next_graph make of the same float32 arrays; invalid device-side
indices give NaN rows and touch nothing else; the launch can be captured; the solvers and the training step see no difference."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
S = 5
VARS = {'CE': ('alpha', 'beta', 'gamma'), 'KF': ('r', 'D'), 'KS': (), 'WE': ('bc_left', 'bc_right', 'c'), 'AD': ('a', 'b')}


@pytest.fixture(scope='module')
def mp():
    import msmp_pde_amd
    assert torch.cuda.is_available()
    return msmp_pde_amd


def make_pde(mp, name, nt, nx):
    from msmp_pde_amd.pde import _PDE
    if name == 'CE':
        return mp.CE(tmin=0.0, tmax=4.0, grid_size=[nt, nx], L=16.0)
    if name == 'WE':
        return mp.WE(tmin=0.0, tmax=100.0, grid_size=[nt, nx])
    if name == 'AD':
        return mp.AD(tmin=0.0, tmax=1.0, grid_size=[nt, nx], L=16.0)
    pde = _PDE(tmin=0.0, tmax=10.0, grid_size=[nt, nx], L=16.0)          # KF, KS: GraphCreator reads the name and the grid only
    pde.name = name
    return pde


def seeded(mp, name, tw, nx, seed=0, neighbors=2):
    """(dataset, creator, float32 host-layout arrays of the creator path) for a seeded float32 store of S samples, nt = 3 tw + 3."""
    nt = 3 * tw + 3
    comps = 2 if name == 'AD' else 1
    gen = torch.Generator().manual_seed(seed + 1000 * tw + nx)
    store = torch.randn(S, nt, comps, nx, generator=gen).to(DEV)
    x = (torch.sort(torch.rand(nx, generator=gen, dtype=torch.float64))[0] * 16).float().double() if name == 'WE' \
        else torch.linspace(0, 16, nx, dtype=torch.float64).float().double()
    variables = {k: (0.1 + torch.rand(S, generator=gen)).float() for k in VARS[name]}
    pde = make_pde(mp, name, nt, nx)
    ds = mp.DeviceDataset(pde, store, x, variables, DEV)
    creator = mp.GraphCreator(pde, neighbors=neighbors, time_window=tw, t_resolution=nt, x_resolution=nx, device=DEV)
    u = store if comps == 2 else store[:, :, 0]
    return ds, creator, u, x.float()


def creator_graph(creator, u, x32, variables, idx, steps, edge_index=None):
    """create_graph(*create_data(u, steps), x, variables, steps) on the samples idx: the parent's path, on float32 arrays."""
    it = torch.as_tensor(idx, device=u.device, dtype=torch.long)
    ub = u[it]
    data, labels = creator.create_data(ub, list(steps))
    vb = {k: v.to(u.device)[it] for k, v in variables.items()}
    return creator.create_graph(data, labels, x32[None].repeat(len(idx), 1), vb, list(steps), edge_index=edge_index)


def raw_assemble(mp, ds, idx, steps, tw, mode=0):
    """One msmp_batch_assemble_f32 launch on fresh (guard-banded) outputs; needs no edge_index, so it also runs at nx = 1."""
    from msmp_pde_amd import _lib
    b, n = len(idx), len(idx) * ds.nx
    ix = torch.tensor([list(idx), list(steps)], dtype=torch.int32, device=DEV)
    x = torch.empty(n, ds.comps * tw, dtype=torch.float32, device=DEV)
    y = torch.empty(n, ds.comps * tw, dtype=torch.float32, device=DEV)
    pos = torch.empty(n, 2, dtype=torch.float32, device=DEV)
    cols = torch.empty(max(ds.n_vars, 1), n, dtype=torch.float32, device=DEV)
    _lib.check(_lib.lib().msmp_batch_assemble_f32(ds.store.data_ptr(), ds.n_samples, ds.nt, ds.comps, ds.nx, ix[0].data_ptr(), ix[1].data_ptr(), b, tw,
                                                  ds.t32.data_ptr(), ds.x32.data_ptr(), ds.var_table.data_ptr() if ds.n_vars else None, ds.n_vars, mode,
                                                  x.data_ptr(), y.data_ptr(), pos.data_ptr(), cols.data_ptr() if ds.n_vars else None,
                                                  _lib.current_stream()), 'msmp_batch_assemble_f32')
    return x, y, pos, cols


def assert_same_fields(got, want, names):
    for k in ('x', 'y', 'pos') + tuple(names):
        a, b = getattr(got, k), getattr(want, k)
        assert a.dtype == torch.float32 and a.shape == b.shape, (k, a.dtype, a.shape, b.shape)
        assert torch.equal(a, b), k


def index_sets(tw, nt):
    """B in {1, 3, 16}: repeated sample indices, steps at both ends of tw .. nt - tw and in between."""
    lo, hi = tw, nt - tw
    return [([3], [hi]), ([4, 0, 4], [lo, hi, lo + 1]),
            ([(7 * j + 2) % S for j in range(16)], [lo + (5 * j) % (hi - lo + 1) for j in range(14)] + [lo, hi])]


@pytest.mark.parametrize('name', ['KS', 'KF', 'CE', 'AD'])          # n_vars 0, 2, 3 (CE: the negated beta) at one component; 2 at two
@pytest.mark.parametrize('tw', [1, 20, 25, 50, 64])
def test_the_kernel_is_the_creator_bit_for_bit(mp, name, tw):
    """x, y, pos and every column of one launch against create_data + create_graph, at node counts on both sides of the 64-node
    chunk (1, 33, 64, 65, 100, 130: a lone node, a partial chunk, the edge, a one-node tail, two and three chunks)."""
    for nx in (1, 33, 64, 65, 100, 130):
        ds, creator, u, x32 = seeded(mp, name, tw, nx)
        no_edges = torch.zeros(2, 0, dtype=torch.long, device=DEV)
        for idx, steps in index_sets(tw, ds.nt):
            want = creator_graph(creator, u, x32, ds.variables, idx, steps, edge_index=no_edges)
            x, y, pos, cols = raw_assemble(mp, ds, idx, steps, tw)
            what = (name, tw, nx, len(idx))
            assert torch.equal(x, want.x) and torch.equal(y, want.y), what
            assert want.pos.dtype == torch.float32 and torch.equal(pos, want.pos), what
            for v, key in enumerate(VARS[name]):
                col = getattr(want, key)
                assert col.dtype == torch.float32 and torch.equal(cols[v].view(-1, 1), col), what + (key,)
    torch.cuda.synchronize()


@pytest.mark.parametrize('name,nx,neighbors', [('CE', 100, 3), ('WE', 33, 2), ('AD', 130, 2), ('KS', 65, 1)])
def test_batch_is_the_creator_graph(mp, name, nx, neighbors):
    """DeviceDataset.batch from host lists and from device tensors: every field of the creator's graph, edge_index and batch included."""
    tw = 25 if name == 'CE' else 20
    ds, creator, u, x32 = seeded(mp, name, tw, nx, seed=1, neighbors=neighbors)
    for idx, steps in index_sets(tw, ds.nt):
        want = creator_graph(creator, u, x32, ds.variables, idx, steps)
        got = ds.batch(creator, idx, steps)
        assert_same_fields(got, want, VARS[name])
        assert torch.equal(got.batch, want.batch) and torch.equal(got.edge_index, want.edge_index)
        assert got.keys() == want.keys()
        dev = ds.batch(creator, torch.tensor(idx, device=DEV), torch.tensor(steps, device=DEV, dtype=torch.int32))
        assert_same_fields(dev, want, VARS[name])
        assert dev.batch is got.batch and dev.edge_index is got.edge_index          # the same objects for every batch of one size


@pytest.mark.parametrize('name,nx', [('CE', 100), ('AD', 65)])
def test_advance_is_create_next_graph(mp, name, nx):
    tw = 25
    ds, creator, u, x32 = seeded(mp, name, tw, nx, seed=2)
    idx, steps = [1, 4, 1], [tw, tw + 3, ds.nt - 2 * tw]
    nxt = [s + tw for s in steps]
    want = creator_graph(creator, u, x32, ds.variables, idx, steps)
    got = ds.batch(creator, idx, steps)
    pred = torch.randn(want.x.shape, generator=torch.Generator().manual_seed(5)).to(DEV)
    _, labels = creator.create_data(u[torch.tensor(idx, device=DEV)], nxt)
    pos_x = got.pos[:, 1].clone()
    cols = {k: getattr(got, k).clone() for k in VARS[name]}
    want = creator.create_next_graph(want, pred, labels, nxt)
    back = ds.advance(got, pred, idx, nxt)
    assert back is got and got.x is pred                             # x becomes the prediction, as in the creator
    assert_same_fields(got, want, VARS[name])
    assert torch.equal(got.pos[:, 1], pos_x) and all(torch.equal(getattr(got, k), v) for k, v in cols.items())
    # a graph whose x is wider than the window keeps the last comps * tw columns of cat(x, pred)
    wide = ds.batch(creator, idx, steps)
    first = wide.x.clone()
    wide.x = torch.cat((first, first), 1)
    ds.advance(wide, pred[:, :3], idx, nxt)
    assert torch.equal(wide.x, torch.cat((first, first, pred[:, :3]), 1)[:, wide.y.shape[1]:])


@pytest.mark.parametrize('bad_index,bad_step', [(-1, None), (S, None), (None, -1), (None, +1)])
@pytest.mark.parametrize('name', ['CE', 'AD'])
def test_an_invalid_device_index_gives_nan_rows_and_nothing_else(mp, name, bad_index, bad_step):
    """A device-side index outside 0 .. S - 1, or a step of tw - 1 / nt - tw + 1, in the middle graph of a batch of three: that graph's
    x / y rows are NaN, its pos / column rows come from the clamped values, the two other graphs are the creator's, and the run ends
    clean (the bounds check at work: nothing outside the store is read)."""
    tw, nx = 20, 100
    ds, creator, u, x32 = seeded(mp, name, tw, nx, seed=3)
    good_idx, good_steps = [2, 0, 4], [tw, tw + 5, ds.nt - tw]
    idx, steps = list(good_idx), list(good_steps)
    if bad_index is not None:
        idx[1] = bad_index
    if bad_step is not None:
        steps[1] = tw - 1 if bad_step < 0 else ds.nt - tw + 1
    clamped_idx = [min(max(i, 0), S - 1) for i in idx]
    clamped_steps = [min(max(s, tw), ds.nt - tw) for s in steps]
    want = creator_graph(creator, u, x32, ds.variables, clamped_idx, clamped_steps)
    got = ds.batch(creator, torch.tensor(idx, device=DEV, dtype=torch.int32), torch.tensor(steps, device=DEV, dtype=torch.int32))
    torch.cuda.synchronize()
    mid = slice(nx, 2 * nx)
    for k in ('x', 'y'):
        a, b = getattr(got, k), getattr(want, k)
        assert torch.isnan(a[mid]).all(), k
        assert torch.equal(a[:nx], b[:nx]) and torch.equal(a[2 * nx:], b[2 * nx:]), k
    assert torch.equal(got.pos, want.pos)
    for k in VARS[name]:
        assert torch.equal(getattr(got, k), getattr(want, k)), k
    nxt = ds.advance(got, got.x, torch.tensor(idx, device=DEV, dtype=torch.int32), torch.tensor(steps, device=DEV, dtype=torch.int32))
    assert torch.isnan(nxt.y[mid]).all() and torch.equal(nxt.y[:nx], want.y[:nx]) and torch.equal(nxt.pos, want.pos)


def test_out_writes_in_place_and_two_calls_agree(mp):
    ds, creator, u, x32 = seeded(mp, 'CE', 25, 100, seed=4)
    (_, _), (ia, sa), (ib, sb) = index_sets(25, ds.nt)
    first = ds.batch(creator, ib, sb)
    again = ds.batch(creator, ib, sb)
    assert_same_fields(first, again, VARS['CE'])                      # two calls are bitwise equal
    other = ds.batch(creator, list(reversed(ib)), sb)
    ptrs = {k: getattr(other, k).data_ptr() for k in ('x', 'y', 'pos') + VARS['CE']}
    back = ds.batch(creator, ib, sb, out=other)
    assert back is other and ptrs == {k: getattr(other, k).data_ptr() for k in ptrs}
    assert_same_fields(other, first, VARS['CE'])
    # columns that do not lie behind one another (separate clones, as CapturedTrainStep keeps them) are filled all the same
    loose = copy.copy(first)
    for k in ('x', 'y', 'pos') + VARS['CE']:
        setattr(loose, k, torch.zeros_like(getattr(first, k)))
    ds.batch(creator, ib, sb, out=loose)
    assert_same_fields(loose, first, VARS['CE'])
    with pytest.raises(ValueError, match='out='):
        ds.batch(creator, ia, sa, out=first)                          # another batch size


def test_a_captured_launch_replays_on_new_indices(mp):
    ds, creator, u, x32 = seeded(mp, 'AD', 25, 100, seed=5)
    _, (ia, sa), _ = index_sets(25, ds.nt)
    idx = torch.tensor(ia, dtype=torch.int32, device=DEV)
    stp = torch.tensor(sa, dtype=torch.int32, device=DEV)
    out = ds.batch(creator, idx, stp)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ds.batch(creator, idx, stp, out=out)
    new_idx, new_steps = [0, 2, 3], [ds.nt - 25, 26, 40]
    idx.copy_(torch.tensor(new_idx, dtype=torch.int32))
    stp.copy_(torch.tensor(new_steps, dtype=torch.int32))
    for k in ('x', 'y', 'pos', 'a', 'b'):
        getattr(out, k).fill_(-7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert_same_fields(out, ds.batch(creator, new_idx, new_steps), VARS['AD'])


# ---- model level ------------------------------------------------------------------------------------------------------------------
def case_dataset(mp, exp, n_samples, seed):
    from msmp_pde_amd.synthetic import make_case
    c = make_case(exp, n_samples, seed=seed, device=DEV, dtype=torch.float32)
    store = c.u_super if c.u_super.dim() == 4 else c.u_super[:, :, None, :]
    c.variables32 = {k: v.float() for k, v in c.variables.items()}
    c.x32 = c.x[0].float().to(DEV)
    return c, mp.DeviceDataset(c.pde, store, c.x[0], c.variables32, DEV)


@pytest.mark.parametrize('kind,exp,bsz', [('MP_PDE_Solver', 'E2', 4), ('MP_PDE_SolverLEMLinGated', 'E2', 4), ('MP_PDE_Solver2DLEMLinGated', 'MSWG3', 2)])
def test_the_solvers_see_no_difference_and_rebuild_no_structure(mp, kind, exp, bsz, monkeypatch):
    from msmp_pde_amd import graph as G
    c, ds = case_dataset(mp, exp, 6, seed=3)
    torch.manual_seed(1)
    model = getattr(mp, kind)(c.pde, time_window=c.tw, eq_variables=c.eqv, hidden_layer=2).to(DEV).eval()
    built = []
    init = G.GraphStructure.__init__

    def counting(self, *a, **kw):
        built.append(1)
        init(self, *a, **kw)
    batches = [([0, 5, 2, 3][:bsz], [30, 200, 25, 111][:bsz]), ([4, 4, 1, 0][:bsz], [225, 77, 140, 26][:bsz]), ([5, 1, 3, 2][:bsz], [99, 25, 60, 61][:bsz])]
    for k, (idx, steps) in enumerate(batches):
        want = creator_graph(c.creator, c.u_super, c.x32, c.variables32, idx, steps)
        got = ds.batch(c.creator, idx, steps)
        if k == 0:
            monkeypatch.setattr(G.GraphStructure, '__init__', counting)      # from the second batch on, the dataset's graphs build none
        with torch.no_grad():
            a = model(got)
            n_dataset = len(built)
            b = model(want)
        assert n_dataset == 0, f'batch {k}: {n_dataset} GraphStructure constructions on the dataset path'
        built.clear()
        assert torch.isfinite(a).all() and torch.equal(a, b), (kind, k)


@pytest.mark.parametrize('captured', [False, True])
@pytest.mark.parametrize('unrolled', [0, 1])
@pytest.mark.parametrize('name', ['MP-PDE', 'MSMP-PDE'])
def test_dataset_training_step_is_training_step(mp, name, unrolled, captured):
    """Three iterations of train.dataset_training_step against train.training_step on the same indices and steps, from identically
    seeded models: losses and all parameters are bitwise equal, eager and with a CapturedTrainStep."""
    from msmp_pde_amd import train as T
    bsz = 4
    c, ds = case_dataset(mp, 'E2', 6, seed=7)
    its = [([0, 5, 2, 3], [30, 200 - 25 * unrolled, 25, 111]), ([4, 4, 1, 0], [225 - 25 * unrolled, 77, 140, 26]), ([5, 1, 3, 2], [99, 25, 60, 61])]

    def run(dataset_path):
        torch.manual_seed(11)
        model = mp.MODEL_NAMES[name](c.pde, time_window=c.tw, eq_variables=c.eqv, hidden_layer=2).to(DEV)
        opt = mp.optim.AdamW(model.parameters(), lr=1e-3, capturable=True)
        step = None
        if captured:
            idx, steps = its[0]
            first = ds.batch(c.creator, idx, steps) if dataset_path else creator_graph(c.creator, c.u_super, c.x32, c.variables32, idx, steps)
            step = T.CapturedTrainStep(model, opt, first, warmup=3)
        losses = []
        for idx, steps in its:
            if dataset_path:
                losses.append(T.dataset_training_step(model, c.creator, ds, idx, steps, unrolled, opt, captured=step).detach().clone())
            else:
                it = torch.tensor(idx, device=DEV)
                vb = {k: v[torch.tensor(idx)] for k, v in c.variables32.items()}
                losses.append(T.training_step(model, c.creator, c.u_super[it], c.x32[None].repeat(bsz, 1), vb, steps, unrolled, opt,
                                              captured=step).detach().clone())
        torch.cuda.synchronize()
        return losses, [p.detach().clone() for p in model.parameters()]

    la, pa = run(False)
    lb, pb = run(True)
    print(name, unrolled, captured, [round(float(l), 5) for l in lb])
    assert all(torch.isfinite(l) for l in lb) and float(lb[0]) != float(lb[-1])
    assert all(torch.equal(a, b) for a, b in zip(la, lb))
    assert all(torch.equal(a, b) for a, b in zip(pa, pb))
