"""GPU tests of the device-resident evaluation (msmp_pde_amd.evaluate, msmp_eval_window_f32): one launch gives, per graph and column, the
float64 sums of (pred - y)^2 and y^2 against the labels of the creator path and writes pos[:, 0] of the next window; a graph's numbers
do not depend on its batch; invalid device-side indices give NaN entries and touch nothing else; the launch can be captured; and
evaluate.rollout / timestep_losses reproduce the reference's loops restated over GraphCreator, predictions bit for bit."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'
S = 5
VARS = {'CE': ('alpha', 'beta', 'gamma'), 'KS': (), 'AD': ('a', 'b')}
SENTINEL = -7.0


@pytest.fixture(scope='module')
def mp():
    import msmp_pde_amd
    assert torch.cuda.is_available()
    return msmp_pde_amd


def make_pde(mp, name, nt, nx):
    from msmp_pde_amd.pde import _PDE
    if name == 'CE':
        return mp.CE(tmin=0.0, tmax=4.0, grid_size=[nt, nx], L=16.0)
    if name == 'AD':
        return mp.AD(tmin=0.0, tmax=1.0, grid_size=[nt, nx], L=16.0)
    pde = _PDE(tmin=0.0, tmax=10.0, grid_size=[nt, nx], L=16.0)          # KS: GraphCreator reads the name and the grid only
    pde.name = name
    return pde


def seeded(mp, name, tw, nx, seed=0):
    """(dataset, creator, float32 trajectories in the creator's layout) for a seeded float32 store of S samples, nt = 3 tw + 3."""
    nt = 3 * tw + 3
    comps = 2 if name == 'AD' else 1
    gen = torch.Generator().manual_seed(seed + 1000 * tw + nx)
    store = torch.randn(S, nt, comps, nx, generator=gen).to(DEV)
    x = torch.linspace(0, 16, nx, dtype=torch.float64).float().double()
    variables = {k: (0.1 + torch.rand(S, generator=gen)).float() for k in VARS[name]}
    pde = make_pde(mp, name, nt, nx)
    ds = mp.DeviceDataset(pde, store, x, variables, DEV)
    creator = mp.GraphCreator(pde, neighbors=2, time_window=tw, t_resolution=nt, x_resolution=nx, device=DEV)
    return ds, creator, (store if comps == 2 else store[:, :, 0])


def index_sets(tw, nt):
    """B in {1, 3, 16}: repeated sample indices, steps at both ends of tw .. nt - tw and in between."""
    lo, hi = tw, nt - tw
    return [([3], [hi]), ([4, 0, 4], [lo, hi, lo + 1]),
            ([(7 * j + 2) % S for j in range(16)], [lo + (5 * j) % (hi - lo + 1) for j in range(14)] + [lo, hi])]


def creator_labels(creator, u, idx, steps):
    """graph.y of the creator path: [B nx, comps tw] float32."""
    _, labels = creator.create_data(u[torch.as_tensor(idx, device=DEV, dtype=torch.long)], list(steps))
    return creator._flatten(labels)


def float64_tables(pred, y, bsz):
    """((pred - y).double() ** 2, y.double() ** 2) summed over the nodes of each graph: [B, comps tw] each"""
    cols = y.shape[1]
    return ((pred - y).double() ** 2).view(bsz, -1, cols).sum(1), (y.double() ** 2).view(bsz, -1, cols).sum(1)


def launch(ds, idx, steps, tw, pred, pad=0, pos=None):
    """One msmp_eval_window_f32 launch into rows of sentinel-filled tables `pad` columns wider than comps tw."""
    from msmp_pde_amd import evaluate as E
    cols = ds.comps * tw
    table = torch.full((2, len(idx), cols + pad), SENTINEL, dtype=torch.float64, device=DEV)
    ix = torch.tensor([list(idx), list(steps)], dtype=torch.int32, device=DEV)
    err, nrm = E.window_errors(ds, ix[0], ix[1], pred, tw, err=table[0, :, :cols], nrm=table[1, :, :cols], pos=pos)
    assert err.data_ptr() == table[0].data_ptr() and nrm.data_ptr() == table[1].data_ptr()
    return err, nrm, table


def assert_within(got, want, nx, what):
    """relative to the float64 reference: nx * 2^-52 covers two sums of nx non-negative terms in different orders (each within
    (nx - 1) 2^-53 of the exact sum) and the rounding of a fused multiply-add against a multiply and an add (2^-53 per term)"""
    bound = nx * 2.0 ** -52
    rel = ((got - want).abs() / want.abs().clamp_min(torch.finfo(torch.float64).tiny)).max().item()
    assert rel <= bound, what + (rel, bound)


@pytest.mark.parametrize('name', ['KS', 'AD'])                        # one and two components
@pytest.mark.parametrize('tw', [1, 20, 25, 50, 64])
def test_the_kernel_against_float64(mp, name, tw):
    """Both tables and pos[:, 0] of one launch at node counts on both sides of the 64-node chunk (a lone node, a partial chunk, the
    edge, a one-node tail, three chunks), for batches of 1, 3 and 16 with repeated samples and steps at both ends of their range, into
    tables three columns wider than the rows written."""
    for nx in (1, 33, 64, 65, 130):
        ds, creator, u = seeded(mp, name, tw, nx)
        for idx, steps in index_sets(tw, ds.nt):
            bsz, what = len(idx), (name, tw, nx, len(idx))
            y = creator_labels(creator, u, idx, steps)
            pred = torch.randn(y.shape, generator=torch.Generator().manual_seed(nx + bsz)).to(DEV)
            pos = torch.full((bsz * nx, 2), SENTINEL, dtype=torch.float32, device=DEV)
            err, nrm, table = launch(ds, idx, steps, tw, pred, pad=3, pos=pos)
            want_err, want_nrm = float64_tables(pred, y, bsz)
            assert_within(err, want_err, nx, what + ('err',))
            assert_within(nrm, want_nrm, nx, what + ('nrm',))
            assert (table[:, :, ds.comps * tw:] == SENTINEL).all(), what
            p = torch.tensor(steps, device=DEV)
            want_t = torch.where(p + tw <= ds.nt - tw, ds.t32[(p + tw).clamp(max=ds.nt - 1)], torch.full((), SENTINEL, device=DEV))
            assert torch.equal(pos[:, 0], want_t.repeat_interleave(nx)), what
            assert (pos[:, 1] == SENTINEL).all(), what
    torch.cuda.synchronize()


@pytest.mark.parametrize('name,tw,nx', [('AD', 25, 130), ('KS', 20, 65), ('KS', 64, 33), ('AD', 1, 64)])
def test_a_graph_alone_is_its_row_in_the_batch_of_16_and_two_runs_agree(mp, name, tw, nx):
    ds, creator, u = seeded(mp, name, tw, nx, seed=1)
    idx, steps = index_sets(tw, ds.nt)[2]
    pred = torch.randn(16 * nx, ds.comps * tw, generator=torch.Generator().manual_seed(7)).to(DEV)
    err, nrm, _ = launch(ds, idx, steps, tw, pred)
    err2, nrm2, _ = launch(ds, idx, steps, tw, pred, pad=5)
    assert torch.equal(err, err2) and torch.equal(nrm, nrm2)
    for b in range(16):
        e1, n1, _ = launch(ds, idx[b:b + 1], steps[b:b + 1], tw, pred[b * nx:(b + 1) * nx].clone())
        assert torch.equal(e1[0], err[b]) and torch.equal(n1[0], nrm[b]), (name, tw, nx, b)


@pytest.mark.parametrize('bad_index,bad_step', [(-1, None), (S, None), (None, -1), (None, +1)])
@pytest.mark.parametrize('name', ['CE', 'AD'])
def test_an_invalid_device_index_gives_nan_entries_and_nothing_else(mp, name, bad_index, bad_step):
    """A device-side index outside 0 .. S - 1, or a step of tw - 1 / nt - tw + 1, in the middle graph of a batch of three: that graph's
    entries of both tables are NaN, the two other graphs' are bitwise those of the clean batch, pos[:, 0] comes from the clamped step,
    and the run ends clean (the bounds check at work: nothing outside the store is read)."""
    tw, nx = 20, 100
    ds, creator, u = seeded(mp, name, tw, nx, seed=3)
    good_idx, good_steps = [2, 0, 4], [tw, tw + 2, ds.nt - tw]
    idx, steps = list(good_idx), list(good_steps)
    if bad_index is not None:
        idx[1] = bad_index
    if bad_step is not None:
        steps[1] = tw - 1 if bad_step < 0 else ds.nt - tw + 1
    pred = torch.randn(3 * nx, ds.comps * tw, generator=torch.Generator().manual_seed(9)).to(DEV)
    clean_err, clean_nrm, _ = launch(ds, good_idx, good_steps, tw, pred)
    pos = torch.full((3 * nx, 2), SENTINEL, dtype=torch.float32, device=DEV)
    err, nrm, table = launch(ds, idx, steps, tw, pred, pad=2, pos=pos)
    torch.cuda.synchronize()
    assert torch.isnan(err[1]).all() and torch.isnan(nrm[1]).all()
    for b in (0, 2):
        assert torch.equal(err[b], clean_err[b]) and torch.equal(nrm[b], clean_nrm[b]), b
    assert (table[:, :, ds.comps * tw:] == SENTINEL).all()
    nxt = [min(max(s, tw), ds.nt - tw) + tw for s in steps]
    want_t = torch.stack([ds.t32[n] if n <= ds.nt - tw else torch.full((), SENTINEL, device=DEV) for n in nxt])
    assert torch.equal(pos[:, 0], want_t.repeat_interleave(nx)) and (pos[:, 1] == SENTINEL).all()


def test_a_captured_launch_replays_on_new_steps_and_predictions(mp):
    from msmp_pde_amd import evaluate as E
    tw, nx = 25, 100
    ds, creator, u = seeded(mp, 'AD', tw, nx, seed=5)
    cols = ds.comps * tw
    idx = torch.tensor([4, 0, 4], dtype=torch.int32, device=DEV)
    stp = torch.tensor([tw, ds.nt - tw, tw + 1], dtype=torch.int32, device=DEV)
    pred = torch.randn(3 * nx, cols, generator=torch.Generator().manual_seed(1)).to(DEV)
    err = torch.empty(3, cols, dtype=torch.float64, device=DEV)
    nrm = torch.empty_like(err)
    pos = torch.full((3 * nx, 2), SENTINEL, dtype=torch.float32, device=DEV)
    E.window_errors(ds, idx, stp, pred, tw, err=err, nrm=nrm, pos=pos)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        E.window_errors(ds, idx, stp, pred, tw, err=err, nrm=nrm, pos=pos)
    new_steps = [tw + 3, tw + 2, ds.nt - tw]
    stp.copy_(torch.tensor(new_steps, dtype=torch.int32))
    pred.copy_(torch.randn(3 * nx, cols, generator=torch.Generator().manual_seed(2)))
    err.fill_(SENTINEL), nrm.fill_(SENTINEL), pos.fill_(SENTINEL)
    graph.replay()
    torch.cuda.synchronize()
    eager_pos = torch.full((3 * nx, 2), SENTINEL, dtype=torch.float32, device=DEV)
    eager_err, eager_nrm, _ = launch(ds, [4, 0, 4], new_steps, tw, pred, pos=eager_pos)
    assert torch.equal(err, eager_err) and torch.equal(nrm, eager_nrm) and torch.equal(pos, eager_pos)
    assert (pos[:2 * nx, 0] != SENTINEL).all() and (pos[2 * nx:, 0] == SENTINEL).all()


# ---- end to end -------------------------------------------------------------------------------------------------------------------
def restated_rollout(model, c, variables32, x32, order, bs, nr_gt_steps):
    """test_unrolled_losses / compute_L2_norms (experiments/train_helper.py:230-277, :381-454) over GraphCreator on the float32 arrays:
    the predictions of every forward, and the two tables in float64 tensor expressions."""
    creator, tw, nx = c.creator, c.tw, c.u_super.shape[-1]
    preds, errs, nrms = [], [], []
    with torch.no_grad():
        for i0 in range(0, len(order), bs):
            idx = order[i0:i0 + bs]
            it = torch.tensor(idx, device=DEV)
            ub, vb, xb = c.u_super[it], {k: v[torch.tensor(idx)] for k, v in variables32.items()}, x32[None].repeat(len(idx), 1)
            e_w, n_w = [], []
            for w, step in enumerate(range(tw * nr_gt_steps, creator.t_res - tw + 1, tw)):
                same_steps = [step] * len(idx)
                data, labels = creator.create_data(ub, same_steps)
                graph = creator.create_graph(data, labels, xb, vb, same_steps) if w == 0 else creator.create_next_graph(graph, pred, labels, same_steps)
                pred = model(graph)
                preds.append(pred)
                e, n = float64_tables(pred, graph.y, len(idx))
                e_w.append(e), n_w.append(n)
            if hasattr(getattr(model, 'embedding_lem', None), 'reset_states'):
                model.embedding_lem.reset_states()
            errs.append(torch.stack(e_w, 1)), nrms.append(torch.stack(n_w, 1))
    return preds, torch.cat(errs), torch.cat(nrms)


def restated_timestep(model, c, variables32, x32, order, bs, steps):
    """test_timestep_losses (experiments/train_helper.py:171-203): predictions and {step: mean over batches of criterion / batch_size}"""
    creator, tw = c.creator, c.tw
    preds, means = [], {}
    with torch.no_grad():
        for step in steps:
            if step != tw and step % tw != 0:
                continue
            losses = []
            for i0 in range(0, len(order), bs):
                idx = order[i0:i0 + bs]
                it = torch.tensor(idx, device=DEV)
                same_steps = [step] * len(idx)
                data, labels = creator.create_data(c.u_super[it], same_steps)
                graph = creator.create_graph(data, labels, x32[None].repeat(len(idx), 1), {k: v[torch.tensor(idx)] for k, v in variables32.items()}, same_steps)
                pred = model(graph)
                preds.append(pred)
                losses.append(float64_tables(pred, graph.y, len(idx))[0].sum() / bs)
            if hasattr(getattr(model, 'embedding_lem', None), 'reset_states'):
                model.embedding_lem.reset_states()
            means[step] = torch.stack(losses).mean()
    return preds, means


def recorded(model, run):
    """what `run()` returns, and the output of every model.forward it made"""
    outs = []
    hook = model.register_forward_hook(lambda m, args, out: outs.append(out))
    try:
        result = run()
    finally:
        hook.remove()
    return result, outs


def close(got, want, rtol=1e-12):
    got, want = torch.as_tensor(got, dtype=torch.float64, device=DEV), torch.as_tensor(want, dtype=torch.float64, device=DEV)
    rel = ((got - want).abs() / want.abs()).max().item()
    assert rel <= rtol, (got, want, rel)


# The 1-D classes run at tw = 20, nt = 100 (four windows after one ground-truth window).  The 2-D classes exist for time windows 25
# and 50 only (experiments/models_gnn2D.py:79-88 has no tw = 20 decoder, and the constructor refuses it), so the AD case keeps the
# shape of the run -- four windows, nx = 40 -- at tw = 25, nt = 125.  The Save variant carries LEM states from batch to batch of a
# timestep pass, which needs equal batches: its timestep pass runs on the first four samples, its rollout on all five.
@pytest.mark.parametrize('name,exp,tw,nt', [('MP-PDE', 'E2', 20, 100), ('MSMP-PDE', 'E2', 20, 100), ('MSMP-PDE2D', 'MSWG3', 25, 125),
                                            ('SaveMSMP-PDE', 'E2', 20, 100)])
def test_rollout_and_timestep_losses_are_the_reference_loops(mp, name, exp, tw, nt):
    """S = 5 in batches of 2 (the last holds one sample), nr_gt_steps 1: every prediction of evaluate.rollout and
    evaluate.timestep_losses is torch.equal to the one the reference's loops make over create_data / create_graph / create_next_graph,
    the tables are the float64 restatement within nx 2^-52, and unrolled_losses, l2_norms and timestep_losses are the reference's
    formulas on the restated tables within 1e-12.  For 'SaveMSMP-PDE' the predictions only agree if the LEM states are reset exactly
    where the reference resets them."""
    from msmp_pde_amd import evaluate as E
    from msmp_pde_amd.synthetic import make_case
    nx, bs, nr = 40, 2, 1
    c = make_case(exp, S, seed=3, device=DEV, nt=nt, nx=nx, tw=tw, neighbors=2, dtype=torch.float32)
    variables32 = {k: v.float() for k, v in c.variables.items()}
    x32 = c.x[0].float().to(DEV)
    ds = mp.DeviceDataset(c.pde, c.u_super if c.u_super.dim() == 4 else c.u_super[:, :, None, :], c.x[0], variables32, DEV)
    torch.manual_seed(1)
    model = mp.MODEL_NAMES[name](c.pde, time_window=tw, eq_variables=c.eqv, hidden_layer=2).to(DEV).eval()
    everyone = list(range(S))

    want_preds, want_err, want_nrm = restated_rollout(model, c, variables32, x32, everyone, bs, nr)
    (err, nrm), preds = recorded(model, lambda: E.rollout(model, c.creator, ds, bs, nr))
    windows = len(range(tw * nr, nt - tw + 1, tw))
    assert windows == 4 and tuple(err.shape) == tuple(nrm.shape) == (S, windows, ds.comps * tw) and err.dtype == torch.float64
    assert len(preds) == len(want_preds) == 3 * windows
    for k, (a, b) in enumerate(zip(preds, want_preds)):
        assert torch.isfinite(a).all() and torch.equal(a, b), (name, 'rollout forward', k)
    assert_within(err, want_err, nx, (name, 'err'))
    assert_within(nrm, want_nrm, nx, (name, 'nrm'))

    per_sample = want_err.sum((1, 2))
    want_losses = torch.stack([per_sample[i0:i0 + bs].sum() / nx / bs for i0 in range(0, S, bs)])
    got_losses = E.unrolled_losses(err, bs, nx)
    assert tuple(got_losses.shape) == (3,) and got_losses.dtype == torch.float64
    close(got_losses, want_losses)
    cells = windows * tw * nx
    want_abs = torch.sqrt(want_err.sum((1, 2)) / cells).mean()
    want_rel = want_abs / torch.sqrt(want_nrm.sum((1, 2)) / cells).mean()
    l2_abs, l2_rel = E.l2_norms(err, nrm, nx, comps=ds.comps)
    close(torch.stack([l2_abs, l2_rel]), torch.stack([want_abs, want_rel]))

    order = everyone[:4] if name == 'SaveMSMP-PDE' else everyone
    steps = [tw, tw + 1, 2 * tw, nt - tw]
    want_preds, want_means = restated_timestep(model, c, variables32, x32, order, bs, steps)
    got_means, preds = recorded(model, lambda: E.timestep_losses(model, c.creator, ds, bs, steps=steps, indices=order))
    assert list(got_means) == list(want_means) == [tw, 2 * tw, nt - tw]
    assert len(preds) == len(want_preds) == 3 * len(range(0, len(order), bs))
    for k, (a, b) in enumerate(zip(preds, want_preds)):
        assert torch.equal(a, b), (name, 'timestep forward', k)
    close(torch.stack([got_means[s] for s in got_means]), torch.stack([want_means[s] for s in want_means]))


def test_test_reads_back_once_and_agrees_with_its_parts(mp):
    """evaluate.test on E2 shapes cut down: the numbers of its parts, as host floats; the base mean from u_base."""
    from msmp_pde_amd import evaluate as E
    from msmp_pde_amd.synthetic import make_case
    tw, nt, nx, bs = 20, 100, 40, 2
    c = make_case('E2', S, seed=4, device=DEV, nt=nt, nx=nx, tw=tw, neighbors=2, dtype=torch.float32)
    variables32 = {k: v.float() for k, v in c.variables.items()}
    u_base = (c.u_super.double() + 0.01).cpu().numpy()
    ds = mp.DeviceDataset(c.pde, c.u_super[:, :, None, :], c.x[0], variables32, DEV, u_base=u_base)
    torch.manual_seed(2)
    model = mp.MODEL_NAMES['MP-PDE'](c.pde, time_window=tw, eq_variables=c.eqv, hidden_layer=2).to(DEV).train()
    r = E.test(model, c.creator, ds, bs, 1, nx)
    assert not model.training
    err, nrm = E.rollout(model, c.creator, ds, bs, 1)
    close(r.unrolled, E.unrolled_losses(err, bs, nx).mean())
    l2 = E.l2_norms(err, nrm, nx)
    close([r.l2_abs, r.l2_rel], torch.stack(l2))
    steps = E.timestep_losses(model, c.creator, ds, bs)
    assert list(r.timestep) == list(steps) == [20, 40, 60, 80]
    close([r.timestep[s] for s in steps], torch.stack([steps[s] for s in steps]))
    # the base loss of u_base = u + 0.01 in float64: 4 windows of tw steps, nx nodes, per batch / nx / bs; batches of 2, 2 and 1
    d2 = ((c.u_super.double() + 0.01) - c.u_super.double()).square()[:, tw:nt].sum((1, 2))
    want = torch.stack([d2[i0:i0 + bs].sum() / nx / bs for i0 in range(0, S, bs)]).mean()
    close(r.base, want)
    assert all(isinstance(v, float) for v in (r.unrolled, r.l2_abs, r.l2_rel, r.base))
