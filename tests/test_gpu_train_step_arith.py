"""GPU tests of the arithmetic every training iteration ends in, each kernel against a plain float64 restatement of the same
operation: the three AdamW forms (msmp_adamw_f32, msmp_adamw_capturable_f32, msmp_adamw_guarded_f32) one step at a time, the two
deterministic reductions (msmp_colsum_f32, msmp_sqerr_sum_f32) and the weight-gradient GEMM (msmp_grad_weights_f32 / _cat_f32).

Everything a kernel writes (parameters, moments, outputs, workspaces) is torch.empty(...) and then filled, so the guard bands of
conftest.py surround it.  Integer operands make the reductions and the GEMM exact in fp32: there a dropped, doubled or misplaced
element is a difference of at least 1 and the assertion is torch.equal.  Real operands are held to worst-case bars counted from the
roundings in the kernels' own expressions (u = 2^-24):

  AdamW, per element, against the float64 rule on the fp32 pre-step state, hyper-parameters rounded to fp32 first:
      m: |d| <=  4u (|b1 m| + |(1 - b1) g|)        v: |d| <= 8u v_ref
      p: |d| <= 24u (|p| + lr / bc1 (|b1 m| + |(1 - b1) g|) / denom_ref)
  colsum: (ceil(rows / blocks) + ceil(blocks group / 256) + 9) u sum|x| over each output's own terms
  sqerr:  (ceil(n / 32768) + 24) u ref

Worst ratios measured on an MI355X, in units of u of the magnitudes above (the tests print them: `pytest -s`):
  AdamW        m      v      p       (bars 4 / 8 / 24; the worst over every test of the form)
  eager        1.91   2.82   4.29
  capturable   1.96   2.82   4.38
  guarded      1.96   2.82   4.38
  grad_weights, real operands with row scales 10^U(-6, 3), 1601 rows, worst |d_ij| / sum_r |a_ri b_rj| in u:
  (ksplit, k2)   kernel   torch's fp32 A^T B
  (31, 64)       5.78     14.25
  (164, 200)     5.61     16.97
  (161, 200)     6.84     19.14
  (318, 319)     6.13     20.26
  colsum on randn stays below 0.1u of sum|x| and sqerr_sum below 1u of the sum; their bars are worst-case depths (19u ... 157u, 28u).

A zero-element CUDA tensor has a null data_ptr() on this stack (the optimizer test prints it), so the optimizer-level case of part 2
needs the same rule as the raw NULL case: both fail on a library that refuses a NULL pointer with numel == 0.
"""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
BAR_M, BAR_V, BAR_P = 4.0, 8.0, 24.0
FORMS = ('eager', 'capturable', 'guarded')
#          lr    beta1 beta2   eps    weight_decay
HYPER = [(1e-3, 0.9, 0.999, 1e-8, 1e-2),
         (1e-2, 0.0, 0.99, 1e-8, 0.0),
         (3e-4, 0.3, 0.5, 1e-6, 0.5),
         (1e-4, 0.95, 0.9999, 1e-10, 1e-2)]


@pytest.fixture(scope='module')
def mp():
    import msmp_pde_amd
    assert torch.cuda.is_available()
    return msmp_pde_amd


def f32(x):
    """the value a C float argument (or a float32 device word) takes for the Python float x"""
    return ctypes.c_float(x).value


# ---- the float64 restatement of the rule in the header of optim_kernels.hip ----------------------------------------------------
def adamw_f64(p, g, m, v, hyper, t):
    """One step from the fp32 state (p, g, m, v): (p', m', v') in float64 and the magnitudes the bars are relative to."""
    lr, b1, b2, eps, wd = (f32(x) for x in hyper)
    p, g, m, v = p.double(), g.double(), m.double(), v.double()
    mag_m = (b1 * m).abs() + ((1.0 - b1) * g).abs()
    m_ref = b1 * m + (1.0 - b1) * g
    v_ref = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    denom = v_ref.sqrt() / math.sqrt(bc2) + eps
    p_ref = p * (1.0 - lr * wd) - lr / bc1 * (m_ref / denom)
    mag_p = p.abs() + lr / bc1 * mag_m / denom
    return (p_ref, m_ref, v_ref), (mag_p, mag_m, v_ref)


def _worst(got, ref, mag):
    """max |got - ref| / (u mag); an element whose magnitude is 0 must be exact"""
    d = (got.double() - ref).abs()
    r = torch.where(mag > 0, d / (U * mag), torch.where(d == 0, torch.zeros_like(d), torch.full_like(d, float('inf'))))
    return float(r.max().item()) if r.numel() else 0.0


def adamw_ratios(pre, post, hyper, t):
    """(m, v, p) worst ratios of one kernel step pre = (p, g, m, v) -> post = (p, m, v)"""
    (p_ref, m_ref, v_ref), (mag_p, mag_m, mag_v) = adamw_f64(*pre, hyper, t)
    return (_worst(post[1], m_ref, mag_m), _worst(post[2], v_ref, mag_v), _worst(post[0], p_ref, mag_p))


class Worst:
    """the worst (m, v, p) ratios of a test, asserted against the bars step by step"""

    def __init__(self):
        self.r = [0.0, 0.0, 0.0]

    def take(self, ratios, what):
        self.r = [max(a, b) for a, b in zip(self.r, ratios)]
        assert ratios[0] <= BAR_M and ratios[1] <= BAR_V and ratios[2] <= BAR_P, (what, 'm v p ratios in u', ratios)

    def report(self, label):
        print(f'ADAMW {label}: worst m {self.r[0]:.2f}u  v {self.r[1]:.2f}u  p {self.r[2]:.2f}u  (bars {BAR_M:g} / {BAR_V:g} / {BAR_P:g})')


# ---- inputs: every intermediate a normal fp32 number or an exact zero --------------------------------------------------------
def _gen(seed):
    return torch.Generator(device='cuda').manual_seed(seed)


def _log_uniform(n, lo, hi, gen):
    return 10.0 ** (lo + (hi - lo) * torch.rand(n, device='cuda', dtype=torch.float64, generator=gen))


def draw_grad(n, gen):
    """+-10^U(-12, 3), 5 % exact zeros"""
    mag = _log_uniform(n, -12, 3, gen)
    sign = torch.where(torch.rand(n, device='cuda', generator=gen) < 0.5, -1.0, 1.0)
    g = (mag * sign).float()
    g[torch.rand(n, device='cuda', generator=gen) < 0.05] = 0.0
    return g


def draw_params(n, gen):
    return torch.randn(n, device='cuda', generator=gen)


def draw_mature(n, gen):
    m = (torch.randn(n, device='cuda', dtype=torch.float64, generator=gen) * _log_uniform(n, -12, 3, gen)).float()
    v = _log_uniform(n, -24, 6, gen).float()
    return m, v


# ---- the three entries on explicit buffers ------------------------------------------------------------------------------------
class RawAdamW:
    """One tensor list for msmp_adamw_f32 / _capturable_f32 / _guarded_f32.  Every buffer is torch.empty and refilled by load();
    an empty tensor gets the address of a live buffer, or NULL with null_empty=True."""

    def __init__(self, mp, sizes, null_empty=False):
        self.L, self.sizes, self.n = mp.lib(), list(sizes), len(sizes)
        mk = lambda: [torch.empty(n, dtype=torch.float32, device='cuda') if n else None for n in self.sizes]
        self.p, self.g, self.m, self.v = mk(), mk(), mk(), mk()
        self.anchor = torch.empty(4, dtype=torch.float32, device='cuda')
        self.step = torch.empty(1, dtype=torch.int64, device='cuda')
        self.lr = torch.empty(1, dtype=torch.float32, device='cuda')
        self.verdict = torch.empty(1, dtype=torch.int32, device='cuda')
        self.skipped = torch.empty(1, dtype=torch.int64, device='cuda')
        self.verdict.zero_()
        self.skipped.zero_()
        empty = None if null_empty else self.anchor.data_ptr()
        table = lambda ts: (ctypes.c_void_p * self.n)(*[t.data_ptr() if t is not None else empty for t in ts])
        self.tables = [table(ts) for ts in (self.p, self.g, self.m, self.v)]
        self.numel = (ctypes.c_int64 * self.n)(*self.sizes)

    def load(self, p, g, m, v):
        """the flat state, cut into the tensors of the list"""
        for bufs, flat in ((self.p, p), (self.g, g), (self.m, m), (self.v, v)):
            for b, src in zip(bufs, torch.split(flat, self.sizes)):
                if b is not None:
                    b.copy_(src)

    def flat(self, bufs):
        return torch.cat([b for b in bufs if b is not None] + [torch.zeros(0, device='cuda')])

    def run(self, form, hyper, t):
        """one step with step count t; returns the entry's return code"""
        from msmp_pde_amd._lib import current_stream
        lr, b1, b2, eps, wd = hyper
        if form == 'eager':
            return self.L.msmp_adamw_f32(self.n, *self.tables, self.numel, lr, b1, b2, eps, wd, t, current_stream())
        self.step.fill_(t - 1)
        self.lr.fill_(lr)
        head = (self.n, *self.tables, self.numel, self.lr.data_ptr(), b1, b2, eps, wd, self.step.data_ptr())
        if form == 'capturable':
            return self.L.msmp_adamw_capturable_f32(*head, current_stream())
        return self.L.msmp_adamw_guarded_f32(*head, self.verdict.data_ptr(), self.skipped.data_ptr(), current_stream())

    def check_words(self, form, t):
        if form != 'eager':
            assert int(self.step.item()) == t, 'the device step word advances once per call'
        if form == 'guarded':
            assert int(self.skipped.item()) == 0 and int(self.verdict.item()) == 0


def one_step(raw, form, state, g, hyper, t, worst, what):
    """state = (p, m, v) flat fp32 -> the kernel's (p, m, v), held to the bars against float64 from that same state"""
    p, m, v = state
    raw.load(p, g, m, v)
    rc = raw.run(form, hyper, t)
    assert rc == 0, (what, rc, raw.L.msmp_last_error())
    post = (raw.flat(raw.p), raw.flat(raw.m), raw.flat(raw.v))
    worst.take(adamw_ratios((p, g, m, v), post, hyper, t), what)
    assert torch.equal(raw.flat(raw.g), g), (what, 'the gradients are read only')
    raw.check_words(form, t)
    return post


def trajectory(raw, form, hyper, seed, worst, young=range(1, 8), mature=(1000, 100000)):
    """steps `young` from zero moments, each from the kernel's own previous output, then the `mature` step counts on a mature state"""
    total, gen = sum(raw.sizes), _gen(seed)
    state = (draw_params(total, gen), torch.zeros(total, device='cuda'), torch.zeros(total, device='cuda'))
    for t in young:
        state = one_step(raw, form, state, draw_grad(total, gen), hyper, t, worst, (form, hyper, t))
    for t in mature:
        state = (draw_params(total, gen),) + draw_mature(total, gen)
        one_step(raw, form, state, draw_grad(total, gen), hyper, t, worst, (form, hyper, t))


# ---- 1. AdamW: one step against float64, all three forms ---------------------------------------------------------------------------
SIZES = [0, 1, 255, 256, 257, 0, 4095, 4096, 4097, 8192, 12289, 0]          # an empty tensor first, in the middle and last


@pytest.mark.parametrize('form', FORMS)
def test_adamw_one_step_vs_float64_over_sizes_hypers_and_steps(mp, form):
    """Tensor sizes either side of a 256-thread trip and of the 4096-element chunk in one call, empty tensors (with an address)
    between them; four hyper-parameter sets; steps 1-7 from zero moments, then t = 1000 and 100 000 on a mature state."""
    raw, worst = RawAdamW(mp, SIZES), Worst()
    for k, hyper in enumerate(HYPER):
        trajectory(raw, form, hyper, 100 + k, worst)
    worst.report(f'{form} sizes')


def _count_sizes(count):
    return [4097 if i in (47, 48, 95, 96) else 7 for i in range(count)]


@pytest.mark.parametrize('count', [48, 49, 96, 97])
@pytest.mark.parametrize('form', FORMS)
def test_adamw_one_step_vs_float64_over_tensor_counts(mp, form, count):
    """48 descriptors per launch: lists that end at, and one past, the first and the second launch, with a two-chunk tensor as the
    last descriptor of a launch and as the first of the next.  Every tensor is compared."""
    raw, worst = RawAdamW(mp, _count_sizes(count)), Worst()
    trajectory(raw, form, HYPER[0], 200 + count, worst, young=(1, 2), mature=(1000,))
    trajectory(raw, form, HYPER[2], 300 + count, worst, young=(1,), mature=(100000,))
    worst.report(f'{form} {count} tensors')


# ---- 2. empty tensors --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form', FORMS)
def test_adamw_entries_step_past_an_empty_tensor_with_null_pointers(mp, form):
    """A numel == 0 entry whose four pointers are NULL is legal in all three entries (as in msmp_grads_finite_f32, and as a
    zero-element parameter is for torch.optim.AdamW): MSMP_OK, every other tensor updated within the bars, the step word advanced once."""
    worst = Worst()
    for sizes in ([0, 5000, 0, 1, 0], [7] * 47 + [0, 0, 4097], [0]):
        raw = RawAdamW(mp, sizes, null_empty=True)
        assert all(tab[i] is None for tab in raw.tables for i, n in enumerate(sizes) if n == 0)
        trajectory(raw, form, HYPER[0], 400 + len(sizes), worst, young=(1, 2), mature=(1000,))
    worst.report(f'{form} null-pointer empties')


OPTIMIZER_FORMS = {'eager': {}, 'capturable': dict(capturable=True), 'guarded': dict(capturable=True, skip_nonfinite=True)}


def _new_param(n, gen):
    p = torch.empty(n, dtype=torch.float32, device='cuda')
    if n:
        p.copy_(draw_params(n, gen))
    return torch.nn.Parameter(p)


def _moments(opt, p):
    st = opt.state.get(p)
    if not st:
        return torch.zeros_like(p), torch.zeros_like(p)
    return st['exp_avg'].detach().clone(), st['exp_avg_sq'].detach().clone()


def optimizer_step(opt, params, gen, t, worst, what):
    """fresh log-uniform gradients, opt.step(), and every parameter held to the bars from its pre-step state"""
    g = opt.param_groups[0]
    hyper = (g['lr'], g['betas'][0], g['betas'][1], g['eps'], g['weight_decay'])
    pre = []
    for p in params:
        p.grad = draw_grad(p.numel(), gen)
        pre.append((p.detach().clone(), p.grad.clone()) + _moments(opt, p))
    opt.step()
    for i, (p, before) in enumerate(zip(params, pre)):
        assert p.shape == before[0].shape
        if p.numel():
            worst.take(adamw_ratios(before, (p.detach(),) + _moments(opt, p), hyper, t), (what, 'tensor', i, 'step', t))


@pytest.mark.parametrize('form', FORMS)
def test_optimizer_steps_past_an_empty_parameter_like_torch(mp, form):
    """optim.AdamW over [Parameter(empty(0)), Parameter(randn(5000))] with gradients on both: no form raises, as torch.optim.AdamW
    does not on the same list; the other parameter follows the rule."""
    gen, worst = _gen(7), Worst()
    params = [_new_param(0, gen), _new_param(5000, gen)]
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    print('data_ptr of a zero-element CUDA tensor:', params[0].data_ptr(), torch.zeros(0, device='cuda').data_ptr())
    ours, theirs = mp.optim.AdamW(params, lr=1e-3, **OPTIMIZER_FORMS[form]), torch.optim.AdamW(twins, lr=1e-3)
    for t in (1, 2, 3):
        optimizer_step(ours, params, gen, t, worst, form)
        for p, q in zip(params, twins):
            q.grad = p.grad.clone()
        theirs.step()
        # the same trajectory as torch's, loosely (float64 above is the reference): |p| < 8, so one fp32 rounding is at most 4.8e-7, and two
        # fp32 evaluations of the rule differ by a few of them per step over three steps
        assert (params[1].detach() - twins[1].detach()).abs().max().item() <= 1e-5
    if form == 'guarded':
        assert ours.skipped_steps == 0
    assert [float(s['step']) for s in ours.state_dict()['state'].values()] == [float(s['step']) for s in theirs.state_dict()['state'].values()] == [3.0, 3.0]
    worst.report(f'{form} optimizer with an empty parameter')


# ---- 3. optim.AdamW across a resume ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('first,second', [('eager', 'capturable'), ('capturable', 'eager')])
def test_optimizer_resumes_in_the_other_form(mp, first, second):
    """Three steps in one form, state_dict() into a fresh optimizer of the other form, three more, a MultiStepLR milestone inside the
    second half; every step within the one-step bars against float64, and every step count 6 at the end."""
    gen, worst = _gen(11), Worst()
    params = [_new_param(n, gen) for n in (1, 5000, 12345)]
    MultiStepLR = torch.optim.lr_scheduler.MultiStepLR
    a = mp.optim.AdamW(params, lr=1e-3, **OPTIMIZER_FORMS[first])
    sa = MultiStepLR(a, milestones=[4], gamma=0.1)
    for t in (1, 2, 3):
        optimizer_step(a, params, gen, t, worst, first)
        sa.step()
    b = mp.optim.AdamW(params, lr=1e-3, **OPTIMIZER_FORMS[second])
    b.load_state_dict(a.state_dict())
    for group in b.param_groups:          # load_state_dict carries the saved group's flag over, as in torch.optim.AdamW: the form is set after it
        group['capturable'] = second == 'capturable'
    sb = MultiStepLR(b, milestones=[4], gamma=0.1)
    sb.load_state_dict(sa.state_dict())
    lrs = []
    for t in (4, 5, 6):
        lrs.append(b.param_groups[0]['lr'])
        optimizer_step(b, params, gen, t, worst, second)
        sb.step()
    assert lrs[0] == 1e-3 and lrs[1] == lrs[2] == pytest.approx(1e-4, rel=1e-12), lrs          # the milestone fell inside the second half
    assert ('_msmp_dev' in b.param_groups[0]) == (second == 'capturable'), 'the second half ran in the other form'
    if second == 'capturable':
        assert int(b.param_groups[0]['_msmp_dev']['step'].item()) == 6
    sd = b.state_dict()
    assert [float(sd['state'][i]['step']) for i in range(3)] == [6.0, 6.0, 6.0]
    worst.report(f'{first} -> {second} resume')


# ---- 4. reductions: exact on integers, bounded on reals -------------------------------------------------------------------------------
COLSUM_ROWS = [127, 128, 129, 130, 255, 256, 257, 16385]          # 129 ... 255: the trailing blocks of the partial kernel own no rows
COLSUM_SHAPES = [(1, 1), (255, 1), (256, 1), (257, 1), (513, 1), (25, 25), (304, 38), (512, 512)]          # (cols, group)
RED_BLOCKS = 128


def _ints(shape, gen):
    return torch.randint(-4, 5, shape, device='cuda', generator=gen).float()


@pytest.mark.parametrize('rows', COLSUM_ROWS)
def test_colsum_is_exact_on_integers(mp, rows):
    """Integers in -4 ... 4: every partial sum is an integer far below 2^24, so fp32 is exact in any order and the result must EQUAL
    the integer sum -- a dropped, doubled or misplaced row or column is a difference of at least 1.  Run to run: the same bits."""
    from msmp_pde_amd import reductions as R
    gen = _gen(rows)
    for cols, group in COLSUM_SHAPES:
        x = _ints((rows, cols), gen)
        ref = x.long().view(rows, cols // group, group).sum((0, 2))
        assert int(ref.abs().max().item()) < 2 ** 24
        got = R.colsum(x, group)
        assert got.shape == ref.shape and torch.equal(got, ref.float()), (rows, cols, group, int((got.long() - ref).abs().max().item()))
        assert torch.equal(got, R.colsum(x, group))


SQERR_N = [1, 255, 256, 257, 32767, 32768, 32769, 100003]          # either side of one block and of the 128 x 256 grid stride


@pytest.mark.parametrize('n', SQERR_N)
def test_sqerr_sum_is_exact_on_integers(mp, n):
    """Differences in -8 ... 8: the sum is at most 64 n < 2^24, exact in fp32 in any order."""
    from msmp_pde_amd import reductions as R
    gen = _gen(n)
    a, b = _ints((n,), gen), _ints((n,), gen)
    ref = ((a.long() - b.long()) ** 2).sum()
    assert 64 * n < 2 ** 24
    got = R.sqerr_sum(a, b)
    assert got.shape == () and float(got.item()) == float(ref.item()), (n, float(got.item()), int(ref.item()))
    assert torch.equal(got, R.sqerr_sum(a, b))


@pytest.mark.parametrize('rows,cols,group', [(1000, 12, 3), (257, 25, 25), (16385, 304, 38)])
def test_colsum_rounding_on_reals(mp, rows, cols, group):
    """randn data against float64 with the worst-case bar of the summation depth in the code: a thread's serial sum over its block's
    rows, the final kernel's serial trips (two at group 3: 128 x 3 > 256; 13 and 19 at the others), the 8-level tree."""
    from msmp_pde_amd import reductions as R
    x = torch.randn(rows, cols, device='cuda', generator=_gen(rows + cols))
    blocks = min(rows, RED_BLOCKS)
    depth = math.ceil(rows / blocks) + math.ceil(blocks * group / 256) + 9
    view = x.double().view(rows, cols // group, group)
    ref, mag = view.sum((0, 2)), view.abs().sum((0, 2))
    got = R.colsum(x, group)
    ratio = ((got.double() - ref).abs() / (U * mag)).max().item()
    print(f'COLSUM {rows} x {cols} / {group}: worst {ratio:.2f}u of sum|x|, bar {depth}u')
    assert ratio <= depth
    assert torch.equal(got, R.colsum(x, group))


def _sqerr_bar(n):
    return math.ceil(n / (RED_BLOCKS * 256)) + 24


def test_sqerr_sum_rounding_on_reals(mp):
    from msmp_pde_amd import reductions as R
    n, gen = 100003, _gen(5)
    a, b = torch.randn(n, device='cuda', generator=gen), torch.randn(n, device='cuda', generator=gen)
    ref = ((a.double() - b.double()) ** 2).sum().item()
    got = R.sqerr_sum(a, b)
    ratio = abs(got.item() - ref) / (U * ref)
    print(f'SQERR n {n}: {ratio:.2f}u of the sum, bar {_sqerr_bar(n)}u')
    assert ratio <= _sqerr_bar(n)
    assert torch.equal(got, R.sqerr_sum(a, b))


def test_sqerr_sum_does_not_expand_the_square(mp):
    """a = 1000 + randn and b = a + 1e-4 randn, both fp32: (a - b)^2 is 1e-14 of a^2, so a kernel that sums a^2 - 2 a b + b^2 loses
    everything; the difference itself is exact in fp32 and the same bar holds."""
    from msmp_pde_amd import reductions as R
    n, gen = 100003, _gen(6)
    a = 1000.0 + torch.randn(n, device='cuda', generator=gen)
    b = (a.double() + 1e-4 * torch.randn(n, device='cuda', dtype=torch.float64, generator=gen)).float()
    ref = ((a.double() - b.double()) ** 2).sum().item()
    got = R.sqerr_sum(a, b)
    ratio = abs(got.item() - ref) / (U * ref)
    print(f'SQERR cancellation n {n}: {ratio:.2f}u of the sum, bar {_sqerr_bar(n)}u')
    assert ref > 0 and ratio <= _sqerr_bar(n)


# ---- 5. grad_weights: the _cat route and the missing edges -------------------------------------------------------------------------
GW_MAX_JOBS = 10


def _gw_job(rows, k2, ksplit, wide_a, draw):
    """(A, B) or (A, B1, B2): A a column slice of a [rows, 512] matrix (lda = 512) or contiguous (lda = 128); B, B1 and B2 column
    slices of wider matrices (ldb > their width)"""
    a_full = draw((rows, 512))
    a = a_full[:, 128:256] if wide_a else a_full[:, :128].contiguous()
    if ksplit is None:
        return (a, draw((rows, k2 + 5))[:, :k2])
    return (a, draw((rows, ksplit + 3))[:, 1:1 + ksplit], draw((rows, k2 - ksplit + 7))[:, 2:2 + k2 - ksplit])


def _gw_reference(job):
    a, b = job[0].double(), torch.cat([x.double() for x in job[1:]], dim=1)
    return a.t() @ b, a.sum(0), b


def _gw_exact(jobs, specs):
    from msmp_pde_amd.autograd import grad_weights
    assert len(jobs) <= GW_MAX_JOBS
    out = grad_weights(jobs)
    for i, job in enumerate(jobs):
        rw, rb, _ = _gw_reference(job)
        assert float(rw.abs().max().item()) < 2 ** 24
        dw, db = out[2 * i], out[2 * i + 1]
        assert dw.shape == rw.shape and db.shape == rb.shape
        assert torch.equal(dw, rw.float()), (specs[i], 'dW', (dw.double() - rw).abs().max().item(), int((dw.double() != rw).sum().item()))
        assert torch.equal(db, rb.float()), (specs[i], 'db', (db.double() - rb).abs().max().item())
    again = grad_weights(jobs)
    assert all(torch.equal(x, y) for x, y in zip(out, again))


GW_SMALL_ROWS = [15, 16, 17, 127, 128, 129]          # either side of a 16-row block and of the 128-row split
GW_K2 = [31, 32, 287, 288]                           # either side of one 32-column tile; k2 + 1 exactly 9 and 10 tiles
GW_LARGE = {0: (32768, 287), 1: (32769, 288)}        # either side of the change of split policy, one job each


@pytest.mark.parametrize('call', range(4))
def test_grad_weights_plain_route_is_exact_on_integers(mp, call):
    """Integers in -4 ... 4 are exact in bf16 and every sum stays below 2^24: dW = A^T B and db must EQUAL the integer result, so one
    dropped ragged row is a difference, not a tolerance event.  The four calls hold the full cross of the small row counts with k2."""
    gen = _gen(50 + call)
    draw = lambda shape: _ints(shape, gen)
    specs = [(rows, GW_K2[(i + call) % 4]) for i, rows in enumerate(GW_SMALL_ROWS)]
    if call in GW_LARGE:
        specs.append(GW_LARGE[call])
    jobs = [_gw_job(rows, k2, None, i % 2 == 1, draw) for i, (rows, k2) in enumerate(specs)]
    _gw_exact(jobs, specs)


GW_CAT = [(1, 33), (31, 64), (32, 64), (33, 64), (128, 164), (164, 200), (150, 200), (160, 200), (161, 200), (318, 319), (1, 319)]          # (ksplit, k2)
GW_CAT_SPECS = [(rows, k2, ksplit) for rows in (129, 1601) for ksplit, k2 in GW_CAT]


@pytest.mark.parametrize('call', range(3))
def test_grad_weights_cat_route_is_exact_on_integers(mp, call):
    """The virtual concatenation [B1 | B2] with the seam inside a tile, on a tile edge, on the 160-column group edge and either side
    of it, one column from either end; the third call mixes plain pairs with triples."""
    gen = _gen(60 + call)
    draw = lambda shape: _ints(shape, gen)
    specs = GW_CAT_SPECS[10 * call:10 * call + 10]
    if call == 2:
        specs = specs + [(129, 288, None), (17, 31, None), (1601, 160, None)] + GW_CAT_SPECS[3:6]
    jobs = [_gw_job(rows, k2, ksplit, i % 2 == 0, draw) for i, (rows, k2, ksplit) in enumerate(specs)]
    assert call != 2 or ({len(j) for j in jobs} == {2, 3})
    _gw_exact(jobs, specs)


@pytest.mark.parametrize('ksplit,k2', [(31, 64), (164, 200), (161, 200), (318, 319)])
def test_grad_weights_cat_route_keeps_fp32_on_reals_of_any_magnitude(mp, ksplit, k2):
    """Rows scaled by 10^U(-6, 3) in both operands.  The kernel's worst componentwise error |d_ij| / sum_r |a_ri b_rj| against float64
    stays within 4x of the same figure for torch's own fp32 A^T B on the same operands (the summation orders differ; a lost product
    of the six-MFMA split would cost about 2^-16, two orders)."""
    from msmp_pde_amd.autograd import grad_weights
    rows, gen = 1601, _gen(70 + ksplit)
    scaled = lambda shape: (torch.randn(shape, device='cuda', dtype=torch.float64, generator=gen)
                            * _log_uniform(shape[0], -6, 3, gen)[:, None]).float()
    job = _gw_job(rows, k2, ksplit, True, scaled)
    rw, _, b64 = _gw_reference(job)
    mag = job[0].double().abs().t() @ b64.abs()
    dw = grad_weights([job])[0]
    lib = job[0].t() @ b64.float()
    ours = ((dw.double() - rw).abs() / (U * mag)).max().item()
    theirs = ((lib.double() - rw).abs() / (U * mag)).max().item()
    print(f'GW_CAT ksplit {ksplit} k2 {k2} rows {rows}: kernel {ours:.2f}u, torch fp32 {theirs:.2f}u')
    assert ours <= 4.0 * theirs
