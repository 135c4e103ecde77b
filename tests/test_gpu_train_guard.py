"""GPU tests of the guarded training step: the finite check over a list of tensors (msmp_grads_finite_f32), the guarded capturable
AdamW (msmp_adamw_guarded_f32), and the range policy of the optimisation step (train.CapturedTrainStep / train.training_step with
range_policy, optim.AdamW(skip_nonfinite=True)): a NaN label or a batch outside the range of the fp16-split path never reaches the
weights, and under 'auto' / 'sync' the trajectory is the one an eager run on the exact-fp32 kernels takes, bit for bit."""
import copy
import ctypes
import os
import sys
import warnings

import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TW = 25
KIND = 'MP_PDE_SolverLEMLinGated'
FLT_MAX = 3.4028234663852886e38
GRAD, SCALAR = 1, 2          # MSMP_NONFINITE_GRAD, MSMP_NONFINITE_SCALAR


@pytest.fixture(scope='module')
def mp():
    import msmp_pde_amd
    assert torch.cuda.is_available()
    return msmp_pde_amd


def _table(ts):
    return (ctypes.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])


def _numel(ts):
    return (ctypes.c_int64 * max(len(ts), 1))(*[t.numel() for t in ts])


# ---- 1. the finite check -----------------------------------------------------------------------------------------------------
SIZES = [12345, 0, 1, 4095, 4096, 4097] + [7] * 42 + [5000]          # 49 tensors: the 49th goes into a second launch
I4097 = SIZES.index(4097)


class Finite:
    """msmp_grads_finite_f32 on one workspace and one verdict word, both reused by every call"""

    def __init__(self, mp, tensors):
        self.mp, self.L, self.tensors = mp, mp.lib(), tensors
        self.ws = torch.empty(self.L.msmp_grads_finite_workspace_bytes(len(tensors), _numel(tensors)), dtype=torch.uint8, device='cuda')
        self.verdict = torch.full((1,), 0x5A5A, dtype=torch.int32, device='cuda')          # never zeroed: every call overwrites it

    def __call__(self, scalars=()):
        from msmp_pde_amd._lib import check, current_stream
        check(self.L.msmp_grads_finite_f32(len(self.tensors), _table(self.tensors), _numel(self.tensors), len(scalars), _table(list(scalars)),
                                           self.verdict.data_ptr(), self.ws.data_ptr(), self.ws.numel(), current_stream()), 'msmp_grads_finite_f32')
        return int(self.verdict.item())


def _finite_tensors():
    gen = torch.Generator(device='cuda').manual_seed(4)
    base = torch.randn(sum(SIZES) + 64, device='cuda', generator=gen)
    out, o = [], 16
    for n in SIZES:                      # slices of one buffer: the empty tensor has an address too
        out.append(base[o:o + n])
        o += n
    return out


def test_finite_check_passes_every_finite_value(mp):
    ts = _finite_tensors()
    for t in (ts[0], ts[I4097], ts[-1]):
        t[0], t[-1] = FLT_MAX, -FLT_MAX
        t[1], t[2], t[3] = 1e-45, 0.0, -0.0          # a denormal and both zeros
    assert float(ts[0][1]) > 0.0                       # the denormal is one (no flush on the way in)
    run = Finite(mp, ts)
    ok = torch.tensor([FLT_MAX], device='cuda')
    assert run() == 0 and run() == 0 and run([ok, torch.zeros(1, device='cuda')]) == 0
    assert Finite(mp, [])() == 0 and Finite(mp, [ts[1]])() == 0          # no tensor at all, and the empty one alone


@pytest.mark.parametrize('value', [float('nan'), float('inf'), -float('inf')], ids=['nan', 'inf', '-inf'])
def test_finite_check_finds_one_bad_element_anywhere(mp, value):
    ts = _finite_tensors()
    run = Finite(mp, ts)
    finite_scalar = torch.ones(1, device='cuda')
    assert run([finite_scalar]) == 0
    places = [(0, 0), (0, SIZES[0] - 1), (48, 0), (48, SIZES[48] - 1), (I4097, 4095), (I4097, 4096)]
    for t, i in places:
        keep = float(ts[t][i])
        ts[t][i] = value
        assert run([finite_scalar]) == GRAD, (t, i)
        assert run([finite_scalar]) == GRAD, (t, i)                   # two runs write the same word
        ts[t][i] = keep
        assert run([finite_scalar]) == 0, (t, i)                      # ... and a bad verdict does not leak into the next call
    # the single-element tensor and the last element before a chunk boundary
    for t, i in ((2, 0), (3, 4094), (4, 4095)):
        keep = float(ts[t][i])
        ts[t][i] = value
        assert run() == GRAD, (t, i)
        ts[t][i] = keep
    assert run() == 0


def test_finite_check_watches_scalars(mp):
    ts = _finite_tensors()
    run = Finite(mp, ts)
    good = torch.ones(1, device='cuda')
    for value in (float('nan'), float('inf'), -float('inf')):
        bad = torch.full((1,), value, device='cuda')
        assert run([bad]) == SCALAR and run([good, bad]) == SCALAR and run([good, good, good, bad]) == SCALAR
        assert run([good]) == 0
        ts[5][17] = value
        assert run([bad]) == (GRAD | SCALAR) and run([good]) == GRAD
        ts[5][17] = 0.5
    assert run([good]) == 0


# ---- 2. the guarded AdamW ----------------------------------------------------------------------------------------------------
class RawAdamW:
    """the capturable entries on explicit tensors: parameters, moments, device step / lr / verdict / skipped words"""

    def __init__(self, mp, params):
        self.L = mp.lib()
        self.p = [p.clone() for p in params]
        self.m, self.v = [torch.zeros_like(p) for p in params], [torch.zeros_like(p) for p in params]
        self.step = torch.zeros(1, dtype=torch.int64, device='cuda')
        self.lr = torch.full((1,), 1e-2, dtype=torch.float32, device='cuda')
        self.verdict = torch.zeros(1, dtype=torch.int32, device='cuda')
        self.skipped = torch.zeros(1, dtype=torch.int64, device='cuda')

    def __call__(self, grads, guarded):
        from msmp_pde_amd._lib import check, current_stream
        head = (len(self.p), _table(self.p), _table(grads), _table(self.m), _table(self.v), _numel(self.p), self.lr.data_ptr(), 0.9, 0.999, 1e-8, 1e-2,
                self.step.data_ptr())
        if guarded:
            check(self.L.msmp_adamw_guarded_f32(*head, self.verdict.data_ptr(), self.skipped.data_ptr(), current_stream()), 'msmp_adamw_guarded_f32')
        else:
            check(self.L.msmp_adamw_capturable_f32(*head, current_stream()), 'msmp_adamw_capturable_f32')

    def state(self):
        return [t.clone() for t in self.p + self.m + self.v + [self.step]]


def test_guarded_adamw_is_the_capturable_one_or_nothing(mp):
    torch.manual_seed(3)
    params = [torch.randn(n, device='cuda') for n in (1, 5000, 12345)]
    a, b = RawAdamW(mp, params), RawAdamW(mp, params)          # a: msmp_adamw_capturable_f32, b: guarded
    gen = torch.Generator(device='cuda').manual_seed(1)
    draw = lambda: [torch.randn(p.shape, device='cuda', generator=gen) for p in params]
    same = lambda: all(torch.equal(x, y) for x, y in zip(a.state(), b.state()))
    for it in range(6):
        g = draw()
        a(g, guarded=False)
        b(g, guarded=True)
        assert same(), it
    assert int(b.step.item()) == 6 and int(b.skipped.item()) == 0
    # a refused step: nothing moves but the skipped word
    before = b.state()
    bad = draw()
    bad[1][77] = float('nan')
    b.verdict.fill_(1)
    b(bad, guarded=True)
    assert all(torch.equal(x, y) for x, y in zip(before, b.state()))
    assert int(b.skipped.item()) == 1 and int(b.step.item()) == 6
    b.verdict.fill_(2)                                         # any non-zero word refuses
    b(bad, guarded=True)
    assert all(torch.equal(x, y) for x, y in zip(before, b.state())) and int(b.skipped.item()) == 2
    # the next good step is the unguarded trajectory's seventh: it never saw the bad ones
    b.verdict.zero_()
    g = draw()
    a(g, guarded=False)
    b(g, guarded=True)
    assert same() and int(b.step.item()) == 7 and int(b.skipped.item()) == 2


def test_optimizer_runs_check_and_guarded_step(mp):
    """optim.AdamW(skip_nonfinite=True).step(): finite check over the live gradients and the watched scalars, then the guarded
    kernel; the trajectory over the good steps is the unguarded optimizer's, and state_dict keeps its layout."""
    torch.manual_seed(3)
    wa = [torch.nn.Parameter(torch.randn(n, device='cuda')) for n in (1, 5000, 12345)]
    wb = [torch.nn.Parameter(w.detach().clone()) for w in wa]
    oa, ob = mp.optim.AdamW(wa, lr=1e-2, capturable=True), mp.optim.AdamW(wb, lr=1e-2, capturable=True, skip_nonfinite=True)
    loss = torch.ones(1, device='cuda')
    ob.watch(loss)
    gen = torch.Generator(device='cuda').manual_seed(1)
    for it in range(5):
        g = [torch.randn(p.shape, device='cuda', generator=gen) for p in wa]
        if it in (1, 3):                 # a bad gradient (1), a bad loss (3): the guarded optimizer skips, the other one is not asked
            if it == 1:
                g[2][12344] = float('inf')
            else:
                loss.fill_(float('nan'))
            for pb, gi in zip(wb, g):
                pb.grad = gi.clone()
            ob.step()
            assert ob.last_step_skipped
            loss.fill_(1.0)
            continue
        for pa, pb, gi in zip(wa, wb, g):
            pa.grad, pb.grad = gi.clone(), gi.clone()
        oa.step(); ob.step()
        assert not ob.last_step_skipped
        assert all(torch.equal(pa, pb) for pa, pb in zip(wa, wb)), it
    assert ob.skipped_steps == 2 and int(ob.param_groups[0]['_msmp_dev']['step'].item()) == 3
    sa, sb = oa.state_dict(), ob.state_dict()
    assert sa['param_groups'][0].keys() == sb['param_groups'][0].keys() and float(sb['state'][0]['step']) == 3.0
    assert all(torch.equal(sa['state'][i][k], sb['state'][i][k]) for i in range(3) for k in ('exp_avg', 'exp_avg_sq'))


# ---- 3 - 8. the range policy of the optimisation step ---------------------------------------------------------------------------
BSZ = 3


@pytest.fixture(scope='module')
def case(mp):
    from msmp_pde_amd.synthetic import make_case
    c = make_case('E2', BSZ, seed=9, device='cuda', dtype=torch.float32)
    c.batches = []
    for i in range(6):
        steps = [40 + 7 * i + (j % 5) for j in range(BSZ)]
        data, labels = c.creator.create_data(c.u_super, steps)
        c.batches.append(c.creator.create_graph(data, labels, c.x, c.variables, steps))
    return c


def _with(graph, **changes):
    g = copy.copy(graph)
    for k, v in changes.items():
        setattr(g, k, v)
    return g


def _out_of_range(graph):
    return _with(graph, x=graph.x + 1000)


def _nan_label(graph):
    y = graph.y.clone()
    y[0, 0] = float('nan')
    return _with(graph, y=y)


def _model(mp, c):
    torch.manual_seed(11)
    return getattr(mp, KIND)(c.pde, time_window=TW, eq_variables=c.eqv, hidden_layer=2).cuda()


def _count(opt):
    return int(opt.param_groups[0]['_msmp_dev']['step'].item())


def _params(model):
    return [p.detach().clone() for p in model.parameters()]


def _range_warnings(rec):
    import msmp_pde_amd as mp_
    return [w for w in rec if issubclass(w.category, mp_.MsmpRangeWarning)]


def run_captured(mp, c, batches, policy, sync_between=False, first=None):
    """A fresh, seeded model trained on `batches` by one CapturedTrainStep (built on an in-range batch).  Returns what the tests
    look at; the status word is read, then cleared, at the end."""
    from msmp_pde_amd import train as T
    model = _model(mp, c)
    opt = mp.optim.AdamW(model.parameters(), lr=1e-3, capturable=True, skip_nonfinite=True)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        step = T.CapturedTrainStep(model, opt, c.batches[0] if first is None else first, range_policy=policy)
        losses = []
        for g in batches:
            losses.append(step(g))
            if sync_between:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
    status = mp.last_status(reset=True)
    moments = [t for st in opt.state.values() for t in (st['exp_avg'], st['exp_avg_sq'])]
    return dict(model=model, opt=opt, step=step, losses=losses, params=_params(model), moments=moments, warnings=_range_warnings(rec), status=status,
                count=_count(opt), skipped=step.skipped_steps)


def run_eager(mp, c, plan):
    """The reference trajectory: a fresh, identically seeded model, `dp_loss_backward` + `optimizer.step()` (the unguarded
    capturable AdamW) per batch; plan = [(batch, exact)]: from the first exact entry on the model has `_range_exact = True`."""
    from msmp_pde_amd import train as T
    model = _model(mp, c)
    opt = mp.optim.AdamW(model.parameters(), lr=1e-3, capturable=True)
    losses = []
    for g, exact in plan:
        if exact:
            model._range_exact = True
        opt.zero_grad(set_to_none=True)
        losses.append(T.dp_loss_backward(model, g).detach().clone())
        opt.step()
    torch.cuda.synchronize()
    assert mp.last_status(reset=True) == 0
    return dict(params=_params(model), losses=losses, count=_count(opt))


def _all_finite(ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_nan_label_is_skipped_in_a_captured_loop(mp, case):
    b = case.batches
    got = run_captured(mp, case, [b[0], b[1], _nan_label(b[2]), b[3], b[4]], 'auto')
    assert _all_finite(got['params']) and _all_finite(got['moments'])
    assert got['skipped'] == 1 and got['count'] == 4
    assert got['status'] == 0 and not got['warnings'] and not got['step']._exact
    assert bool(torch.isnan(got['losses'][2])) and all(bool(torch.isfinite(l)) for i, l in enumerate(got['losses']) if i != 2)
    good = run_captured(mp, case, [b[0], b[1], b[3], b[4]], 'auto')
    assert good['skipped'] == 0 and good['count'] == 4
    assert _same(got['params'], good['params'])


def test_out_of_range_first_call_is_evaluated_again_on_exact_fp32(mp, case):
    """skipped_steps is 1 afterwards: the probe's replay on the split kernels, which the device skipped and the host then repeated on
    the exact-fp32 capture.  No step is dropped."""
    b = case.batches
    seq = [_out_of_range(b[1]), b[2], b[3]]
    got = run_captured(mp, case, seq, 'auto')
    assert len(got['warnings']) == 1 and '0 optimisation step(s) were dropped' in str(got['warnings'][0].message)
    assert got['model']._range_exact and got['step']._exact
    assert got['skipped'] == 1 and got['step'].dropped_steps == 0 and got['count'] == 3
    assert got['status'] == 0
    assert all(bool(torch.isfinite(l)) for l in got['losses'])
    ref = run_eager(mp, case, [(g, True) for g in seq])
    assert _same(got['losses'], [l.view_as(got['losses'][0]) for l in ref['losses']])
    assert _same(got['params'], ref['params'])


def _sequence(b):
    return [b[0], b[1], b[2], _out_of_range(b[3]), b[4], b[5]]


def test_sync_policy_drops_nothing(mp, case):
    seq = _sequence(case.batches)
    got = run_captured(mp, case, seq, 'sync')
    assert got['count'] == 6 and got['skipped'] == 1 and got['step'].dropped_steps == 0 and got['status'] == 0
    assert len(got['warnings']) == 1 and got['step']._exact
    assert all(bool(torch.isfinite(l)) for l in got['losses'])
    ref = run_eager(mp, case, [(g, i >= 3) for i, g in enumerate(seq)])
    assert ref['count'] == 6
    assert _same(got['params'], ref['params'])


def test_auto_policy_after_the_probe_drops_the_steps_the_host_did_not_see(mp, case):
    seq = _sequence(case.batches)
    got = run_captured(mp, case, seq, 'auto', sync_between=True)
    assert got['count'] == 5 and got['skipped'] == 1 and got['step'].dropped_steps == 1 and got['status'] == 0
    assert len(got['warnings']) == 1 and '1 optimisation step(s) were dropped' in str(got['warnings'][0].message)
    assert bool(torch.isnan(got['losses'][3])) and all(bool(torch.isfinite(l)) for i, l in enumerate(got['losses']) if i != 3)
    ref = run_eager(mp, case, [(g, i >= 3) for i, g in enumerate(seq) if i != 3])
    assert ref['count'] == 5
    assert _same(got['params'], ref['params'])


def test_model_switched_elsewhere_captures_again(mp, case):
    from msmp_pde_amd import train as T
    b = case.batches
    model = _model(mp, case)
    opt = mp.optim.AdamW(model.parameters(), lr=1e-3, capturable=True, skip_nonfinite=True)
    step = T.CapturedTrainStep(model, opt, b[0], range_policy='auto')
    step(b[0]); step(b[1])
    assert not step._exact and not model._range_exact
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        with torch.no_grad():
            model(_out_of_range(b[2]))                  # Solver.range_policy: evaluated again on exact fp32, the model stays there
        assert model._range_exact and len(_range_warnings(rec)) == 1
        loss = step(b[3])
    assert step._exact and bool(torch.isfinite(loss))
    assert _count(opt) == 3 and step.skipped_steps == 0 and step.dropped_steps == 0
    torch.cuda.synchronize()
    assert mp.last_status(reset=True) == 0


def test_eager_training_step_skips_a_nan_label(mp, case):
    from msmp_pde_amd import train as T
    c = case
    model = _model(mp, c)
    opt = mp.optim.AdamW(model.parameters(), lr=1e-3, capturable=True, skip_nonfinite=True)
    steps = [60] * BSZ
    bad = c.u_super.clone()
    bad[0, 63, 0] = float('nan')                        # inside the label window [60, 85) of sample 0
    before = _params(model)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        loss = T.training_step(model, c.creator, bad, c.x, c.variables, steps, 0, opt, captured=None, range_policy='sync')
    assert bool(torch.isnan(loss)) and opt.skipped_steps == 1 and _count(opt) == 0 and not _range_warnings(rec)
    assert _same(before, _params(model)) and not model._range_exact
    loss = T.training_step(model, c.creator, c.u_super, c.x, c.variables, steps, 0, opt, captured=None, range_policy='sync')
    assert bool(torch.isfinite(loss)) and opt.skipped_steps == 1 and _count(opt) == 1
    assert not _same(before, _params(model)) and _all_finite(_params(model))
    with pytest.raises(ValueError, match='skip_nonfinite'):
        T.training_step(model, c.creator, c.u_super, c.x, c.variables, steps, 0, mp.optim.AdamW(model.parameters(), capturable=True), range_policy='sync')
    assert mp.last_status(reset=True) == 0


def test_eager_training_step_repeats_an_out_of_range_step(mp, case):
    """training_step(captured=None, range_policy='sync') on a trajectory outside the range: the step is taken on the exact-fp32
    kernels, as an eager run with `_range_exact = True` from the start takes it."""
    from msmp_pde_amd import train as T
    c = case
    steps = [60] * BSZ
    far = c.u_super + 1000
    model = _model(mp, c)
    opt = mp.optim.AdamW(model.parameters(), lr=1e-3, capturable=True, skip_nonfinite=True)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        loss = T.training_step(model, c.creator, far, c.x, c.variables, steps, 0, opt, captured=None, range_policy='sync')
    assert len(_range_warnings(rec)) == 1 and model._range_exact and bool(torch.isfinite(loss))
    assert opt.skipped_steps == 1 and _count(opt) == 1
    ref_model = _model(mp, c)
    ref_model._range_exact = True
    ref_opt = mp.optim.AdamW(ref_model.parameters(), lr=1e-3, capturable=True)
    ref_loss = T.training_step(ref_model, c.creator, far, c.x, c.variables, steps, 0, ref_opt)
    assert torch.equal(loss, ref_loss) and _same(_params(model), _params(ref_model))
    torch.cuda.synchronize()
    assert mp.last_status(reset=True) == 0


# ---- 9. data parallelism ---------------------------------------------------------------------------------------------------------
def _dp_guard_worker(rank, world, port, out_dir, double):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK='0')
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, 'tests'))
    import msmp_pde_amd as mp_
    from msmp_pde_amd import dist as D, train as T
    from helpers import synthetic_case
    D.init_from_env(backend='gloo')
    case = synthetic_case(mp_, 'E2', bsz=4, seed=6)         # float64 node tensors: the loss sum is then PyTorch's, in float64
    case2 = synthetic_case(mp_, 'E2', bsz=4, seed=8)
    shards = [D.shard_graph(c.graph, rank, world).to('cuda') for c in (case, case2, case)]
    if not double:                                          # float32 node tensors: the library's loss sum, poisoned in place
        for g in shards:
            for k in g.keys():
                if torch.is_tensor(getattr(g, k)) and getattr(g, k).is_floating_point():
                    setattr(g, k, getattr(g, k).float())
    if rank == 1:                                           # step 2: only this rank's shard leaves the range
        shards[1].x = shards[1].x + 1000
    torch.manual_seed(5)                                    # same weights everywhere
    model = mp_.MP_PDE_SolverLEMLinGated(case.pde, time_window=TW, eq_variables=case.eqv, hidden_layer=2).cuda()
    opt = mp_.optim.AdamW(model.parameters(), lr=1e-3, capturable=True, skip_nonfinite=True)
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter('always')
        step = T.CapturedTrainStep(model, opt, shards[0], range_policy='sync')
        losses = [float(step(g)) for g in shards]
        torch.cuda.synchronize()
    torch.save({'params': [p.detach().cpu().clone() for p in model.parameters()], 'skipped': step.skipped_steps, 'dropped': step.dropped_steps,
                'count': int(opt.param_groups[0]['_msmp_dev']['step'].item()), 'losses': losses, 'exact': bool(step._exact),
                'range_warnings': sum(issubclass(w.category, mp_.MsmpRangeWarning) for w in rec), 'status': mp_.last_status(reset=True)},
               os.path.join(out_dir, f'rank{rank}.pt'))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


@pytest.mark.parametrize('double', [False, True], ids=['float32', 'float64'])
def test_data_parallel_ranks_skip_and_recover_together(mp, tmp_path, double):
    """Two ranks (gloo, both on the one GPU), three captured steps under 'sync'; in the second only rank 1's shard is out of range.
    Its status poison makes S, the loss and every gradient NaN on both ranks, both skip, both capture again on the exact-fp32 kernels
    and repeat the step: the same skipped count, the same finite parameters, nothing dropped."""
    import torch.multiprocessing as tmp
    ctx = tmp.get_context('spawn')
    port = 29500 + (os.getpid() % 200) + 200 * int(double)
    procs = [ctx.Process(target=_dp_guard_worker, args=(r, 2, port, str(tmp_path), double)) for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(400)
        assert p.exitcode == 0
    r0, r1 = (torch.load(str(tmp_path / f'rank{r}.pt'), weights_only=True) for r in range(2))
    print('DP losses', r0['losses'], r1['losses'], 'skipped', r0['skipped'], r1['skipped'])
    assert r0['skipped'] == r1['skipped'] == 1 and r0['dropped'] == r1['dropped'] == 0 and r0['count'] == r1['count'] == 3
    assert all(torch.equal(a, b) for a, b in zip(r0['params'], r1['params']))
    assert all(bool(torch.isfinite(a).all()) for a in r0['params'])
    assert r0['losses'] == r1['losses'] and all(l == l for l in r0['losses'])
    assert r0['exact'] and r1['exact'] and r0['status'] == r1['status'] == 0
