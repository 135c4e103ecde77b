"""GPU tests of msmp_wide_layer_bwd_f32 (wide_layer_bwd_kernel.hip), the backward of one GNN_LayerLin / gated pair at any hidden width,
and of the host path that takes it (layers.mp_layer with msmp_tune("wide_bwd") != 0).

Reference: float64 torch.autograd over autograd.layer_reference (width-generic, no kernel of the library involved), built as
tests/test_gpu_backward_sizes.py builds it.  Bars, from that file: dh 2e-4 max(|ref|max, 1); each parameter 1e-4 |ref|max + 2e-5 (largest
gradient entry); or FLOOR_FACTOR times the error of float32 torch.autograd over the same restatement, whichever is larger.  Rows of the
1- and 2-node graphs are masked out of dh (InstanceNorm's derivative is ill-conditioned there): at most 2 % of the rows."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from helpers import record_parity, FLOOR_FACTOR, ld_of, tuned, synthetic_case

pytestmark = pytest.mark.gpu

RG_SMALL_ROWS = 32768                 # rows_gemm: rows_gemm_small_kernel below, rows_gemm_kernel from here on
GRID_CAP = 32768                      # grid_for: at most 32 768 blocks of 256 threads, a thread = (row, 16-byte channel group)
PATTERN = [1, 100, 3, 130, 2]         # nodes per graph, repeated; every ragged batch ends in one more 100-node graph
EPS = 1e-5


@pytest.fixture(scope='module')
def mp():
    import msmp_pde_amd
    assert torch.cuda.is_available()
    msmp_pde_amd.lib()
    return msmp_pde_amd


_cache = {}           # at most one batch and one reference at a time (the tests that share them are adjacent)


@pytest.fixture(scope='module', autouse=True)
def _release_memory():
    yield
    from msmp_pde_amd import autograd as A
    _cache.clear()
    A._wide_bwd_ws.clear()
    A._bwd_ws.clear()
    torch.cuda.empty_cache()


def _inputs(k, e, W, tw, nv, sizes=None):
    """The ragged batch PATTERN * k + [100] (or `sizes`) with e random edges inside its graphs of 100 nodes and more, whose last 7 nodes
    stay without in-edges, and random layer inputs at width W."""
    key = (k, e, W, tw, nv, tuple(sizes or ()))
    if _cache.get('inputs_key') == key:
        return _cache['inputs']
    _cache.clear()
    torch.cuda.empty_cache()
    from msmp_pde_amd.graph import GraphStructure
    ragged = sizes is None
    sizes = torch.tensor(PATTERN * k + [100] if ragged else sizes)
    n = int(sizes.sum())
    starts = torch.cumsum(sizes, 0) - sizes
    g = torch.Generator(device='cpu').manual_seed(21 + k + e % 97)
    big = torch.nonzero(sizes >= 100)[:, 0]
    pick = big[torch.randint(0, big.numel(), (e,), generator=g)]
    z, s0 = sizes[pick], starts[pick]
    src = s0 + torch.minimum((torch.rand(e, generator=g, dtype=torch.float64) * z).long(), z - 1)
    dst = s0 + torch.minimum((torch.rand(e, generator=g, dtype=torch.float64) * (z - 7)).long(), z - 8)
    c = SimpleNamespace(key=key, n=n, e=e, W=W, tw=tw, nv=nv, k=k, n_graphs=int(sizes.numel()))
    c.ei = torch.stack([src, dst]).cuda()
    c.batch = torch.repeat_interleave(torch.arange(sizes.numel()), sizes).cuda()
    c.gs = GraphStructure(c.ei, c.batch, n)
    assert c.gs.n_edges == e and c.gs.n_graphs == c.n_graphs
    gc = torch.Generator(device='cuda').manual_seed(5 + k + W)
    r = lambda *s: torch.randn(*s, generator=gc, device='cuda')
    c.h, c.u, c.pos, c.var, c.gout = r(n, W), r(n, tw), r(n), r(n, nv), r(n, W)
    # rows compared in dh: all but the 1- and 2-node graphs
    c.multi = (sizes > 2).cuda()[c.batch]
    excluded = n - int(c.multi.sum())
    assert excluded == (3 * k if ragged else 0) and excluded <= 0.02 * n
    assert bool(c.multi[-1])              # the ragged last row block is compared, not masked
    _cache.update(inputs_key=key, inputs=c)
    return c


def _params(c, form, seed=0):
    g = torch.Generator(device='cpu').manual_seed(77 + c.k + len(form) + c.W + seed)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    W, k1, k3 = c.W, 2 * c.W + c.tw + 1 + c.nv, 2 * c.W + c.nv
    one = lambda: [r(W, k1) / k1 ** 0.5, r(W) * 0.1, r(W, W) / W ** 0.5, r(W) * 0.1, r(W, k3) / k3 ** 0.5, r(W) * 0.1, r(W, W) / W ** 0.5, r(W) * 0.1]
    return one() + (one() if form == 'gated' else [])


def _autograd(c, ps, form, dtype, eps=EPS):
    """dL/dh and the parameter gradients by torch.autograd over A.layer_reference in `dtype` (no kernel of the library involved)."""
    from msmp_pde_amd import autograd as A
    h = c.h.to(dtype, copy=True).requires_grad_(True)
    p = [q.detach().to(dtype, copy=True).requires_grad_(True) for q in ps]
    args = (c.u.to(dtype), c.pos.to(dtype), c.var.to(dtype), c.gs.col_long, c.gs.tgt_long, c.batch, c.n_graphs)
    if form == 'gated':
        tau = torch.sigmoid(A.layer_reference(h, *args, p[8:], True, eps))
        out = (1 - tau) * h + tau * A._swish(A.layer_reference(h, *args, p[:8], True, eps))
    else:
        out = A.layer_reference(h, *args, p, True, eps)
    out.backward(c.gout.to(dtype))
    return h.grad, [q.grad for q in p]


def _dh_err(c, dh, ref):
    return ((dh.double() - ref)[c.multi]).abs().max().item()


def _reference(c, form, ps=None, eps=EPS):
    """Float64 reference, the float32 floor against it (per tensor) and the bars, once per (batch, form, eps); ps: a model's parameters
    instead of random ones."""
    key = (c.key, form, eps)
    if ps is None and _cache.get('ref_key') == key:
        return _cache['ref']
    _cache.pop('ref', None)
    ps = _params(c, form) if ps is None else ps
    dh64, g64 = _autograd(c, ps, form, torch.float64, eps)
    dh32, g32 = _autograd(c, ps, form, torch.float32, eps)
    ref = SimpleNamespace(ps=ps, dh=dh64, grads=g64)
    ref.scale = max(q.abs().max().item() for q in g64)
    ref.dh_floor = _dh_err(c, dh32, dh64)
    ref.p_floor = [(a.double() - b).abs().max().item() for a, b in zip(g32, g64)]
    ref.dh_small = 2e-4 * max(dh64.abs().max().item(), 1.0)
    ref.p_small = [1e-4 * q.abs().max().item() + 2e-5 * ref.scale for q in g64]
    ref.dh_bar = max(ref.dh_small, FLOOR_FACTOR * ref.dh_floor)
    ref.p_bar = [max(s, FLOOR_FACTOR * f) for s, f in zip(ref.p_small, ref.p_floor)]
    del dh32, g32
    _cache.update(ref_key=key, ref=ref)
    return ref


def _padded(x, ld):
    out = torch.zeros(x.shape[0], ld, dtype=torch.float32, device='cuda')
    out[:, :x.shape[1]] = x
    return out


def _wide_bwd(mp, c, ps, form, eps=EPS):
    """msmp_wide_layer_bwd_f32 through the C-ABI: -> (return code, dh [N, ld], grads).  The workspace carries its own 1-KB guard bands (it
    can be larger than what conftest.py guards); dh and the gradients come from torch.empty (guarded there)."""
    from msmp_pde_amd._lib import ptr, current_stream
    L = mp.lib()
    gs, n, W, e, gated = c.gs, c.n, c.W, c.gs.n_edges, form == 'gated'
    ld = ld_of(W)
    hp, gp = _padded(c.h, ld), _padded(c.gout, ld)
    grads = [torch.empty(q.shape, dtype=torch.float32, device='cuda') for q in ps]
    dh = torch.empty(n, ld, dtype=torch.float32, device='cuda')
    dh.fill_(float('nan'))
    need = L.msmp_wide_layer_bwd_workspace_bytes(n, e, c.tw, c.nv, W, int(gated))
    assert need > 0
    raw = torch.full((need + 2048,), 0x5A, dtype=torch.uint8, device='cuda')
    arr = lambda ts: (ctypes.c_void_p * 8)(*[t.data_ptr() for t in ts])
    perm32, src_rowptr = gs.by_source32() if e else (None, None)
    rc = L.msmp_wide_layer_bwd_f32(ptr(gp), ptr(hp), ptr(c.u), ptr(c.pos), ptr(c.var), ptr(gs.rowptr), ptr(gs.col), ptr(gs.tgt), ptr(src_rowptr),
                                   ptr(perm32), ptr(gs.graph_ptr), n, e, gs.n_graphs, c.tw, c.nv, W, ld, arr(ps[:8]), arr(ps[8:]) if gated else None,
                                   eps, ptr(dh), arr(grads[:8]), arr(grads[8:]) if gated else None, raw.data_ptr() + 1024, need, current_stream())
    torch.cuda.synchronize()
    assert bool((raw[:1024] == 0x5A).all()) and bool((raw[1024 + need:] == 0x5A).all()), 'workspace guard band overwritten'
    del raw
    return rc, dh, grads


def _narrow_bwd(mp, c, ps, form):
    """msmp_mp_layer_bwd_f32 (the 128-wide entry, its default path) on the same inputs"""
    from msmp_pde_amd._lib import ptr, current_stream
    L = mp.lib()
    gs, n, e, gated = c.gs, c.n, c.gs.n_edges, form == 'gated'
    assert c.W == 128
    grads = [torch.empty(q.shape, dtype=torch.float32, device='cuda') for q in ps]
    dh = torch.empty(n, 128, dtype=torch.float32, device='cuda')
    need = L.msmp_mp_layer_bwd_workspace_bytes(n, e, c.tw, c.nv, int(gated))
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    arr = lambda ts: (ctypes.c_void_p * 8)(*[t.data_ptr() for t in ts])
    perm32, src_rowptr = gs.by_source32()
    rc = L.msmp_mp_layer_bwd_f32(ptr(c.gout), ptr(c.h), ptr(c.u), ptr(c.pos), ptr(c.var), ptr(gs.rowptr), ptr(gs.col), ptr(gs.tgt),
                                 ptr(src_rowptr), ptr(perm32), ptr(gs.graph_ptr), n, e, gs.n_graphs, c.tw, c.nv, arr(ps[:8]),
                                 arr(ps[8:]) if gated else None, 1, EPS, ptr(dh), arr(grads[:8]), arr(grads[8:]) if gated else None, ptr(ws), need,
                                 current_stream())
    torch.cuda.synchronize()
    assert rc == 0, (rc, L.msmp_last_error())
    return dh, grads


def _check(mp, c, ref, form, label, dh, grads):
    """dh (its padding columns exactly 0) and every gradient against the reference at the bars; every figure printed and recorded first"""
    W = c.W
    assert torch.isfinite(dh).all() and all(torch.isfinite(g).all() for g in grads)
    assert dh.shape[1] == ld_of(W) and bool((dh[:, W:] == 0).all()), 'padding columns of dh_out'
    dh_err = _dh_err(c, dh[:, :W], ref.dh)
    p_err = [(g.double() - q).abs().max().item() for g, q in zip(grads, ref.grads)]
    worst = max(range(len(p_err)), key=lambda i: p_err[i] / ref.p_bar[i])
    print(f'{label}: dh err {dh_err:.3e} floor {ref.dh_floor:.3e} bar {ref.dh_bar:.3e}; worst parameter {worst}: '
          f'err {p_err[worst]:.3e} floor {ref.p_floor[worst]:.3e} bar {ref.p_bar[worst]:.3e}')
    record_parity('wide_layer_backward', label, n_nodes=c.n, n_edges=c.e, dh_err=dh_err, dh_floor=ref.dh_floor, dh_bar=ref.dh_bar,
                  dh_ratio=dh_err / ref.dh_bar, worst_param=worst, param_err=p_err[worst], param_floor=ref.p_floor[worst],
                  param_bar=ref.p_bar[worst], param_ratio=p_err[worst] / ref.p_bar[worst])
    assert dh_err < ref.dh_bar, (dh_err, ref.dh_floor, ref.dh_bar)
    for i, (got, q) in enumerate(zip(grads, ref.grads)):
        assert got.shape == q.shape
        assert p_err[i] < ref.p_bar[i], (i, p_err[i], ref.p_floor[i], ref.p_bar[i])


# widths: 164 (second 128-column group with a 36-column tail), 132 (4-column tail), 96 (one partial group), 256 (two full groups), 128
_SMALL = [(W, 25, nv) for W in (164, 132, 96, 256, 128) for nv in (2, 3)] + [(164, 50, 3)]


@pytest.mark.parametrize('form', ['lin', 'gated'])
@pytest.mark.parametrize('W,tw,nv', _SMALL, ids=[f'w{W}-tw{tw}-nv{nv}' for W, tw, nv in _SMALL])
def test_entry_vs_float64_autograd(mp, W, tw, nv, form):
    """336 nodes in the ragged batch [1, 100, 3, 130, 2, 100], 2 000 random edges inside the 100- and 130-node graphs (the last 7 nodes of
    each without in-edges): dh [N, ld] and all 8 / 16 parameter gradients against float64 autograd; padding columns of dh exactly 0."""
    c = _inputs(1, 2000, W, tw, nv)
    assert c.n == 336
    ref = _reference(c, form)
    rc, dh, grads = _wide_bwd(mp, c, ref.ps, form)
    assert rc == 0, (rc, mp.lib().msmp_last_error())
    _check(mp, c, ref, form, f'small/w{W}-tw{tw}-nv{nv}/{form}', dh, grads)


@pytest.mark.parametrize('form', ['lin', 'gated'])
def test_width_128_agrees_with_the_128_wide_entry(mp, form):
    """Two implementations of one formula on the same inputs: dh and all 8 / 16 gradients of msmp_wide_layer_bwd_f32 at width 128 are within
    the bars (those of the float64 reference) of msmp_mp_layer_bwd_f32."""
    c = _inputs(1, 2000, 128, 25, 3)
    ref = _reference(c, form)
    rc, dh, grads = _wide_bwd(mp, c, ref.ps, form)
    assert rc == 0, (rc, mp.lib().msmp_last_error())
    dh_n, grads_n = _narrow_bwd(mp, c, ref.ps, form)
    d = _dh_err(c, dh[:, :128], dh_n.double())
    pd = [(a - b).abs().max().item() for a, b in zip(grads, grads_n)]
    print(f'width 128 {form}: dh wide vs narrow {d:.3e} (bar {ref.dh_bar:.3e}); parameters {max(pd):.3e}')
    assert d < ref.dh_bar
    assert len(pd) == (16 if form == 'gated' else 8)
    for i, x in enumerate(pd):
        assert x < ref.p_bar[i], (i, x, ref.p_bar[i])


# case -> (pattern repeats, edges, forms)
_BIG = {'edge-big': (5, 33001, ('lin', 'gated')), 'node-big': (139, 20000, ('lin', 'gated')), 'strided': (557, 140001, ('lin',))}


@pytest.mark.parametrize('case,form', [(k, f) for k, v in _BIG.items() for f in v[2]])
def test_entry_at_the_sizes_where_kernels_switch(mp, case, form):
    """Width 164.  edge-big (E = 33 001 >= 32 768 > N = 1 280): the edge-row GEMMs on rows_gemm_kernel, the node rows on the small one;
    node-big (N = 32 904 >= 32 768 > E): the other way round;  strided (N = 131 552, E = 140 001: more than 32 768 * 256 (row, 16-byte
    group) pairs at 64 groups per row): every grid_for launch takes a second grid-stride pass.  edge-big / gated: two calls give the same bits."""
    k, e, _ = _BIG[case]
    c = _inputs(k, e, 164, 25, 3)
    if case == 'edge-big':
        assert c.e >= RG_SMALL_ROWS > c.n and c.e % 128
    elif case == 'node-big':
        assert c.n >= RG_SMALL_ROWS > c.e and c.n % 128
    else:
        assert c.n * 64 > GRID_CAP * 256 and c.e * 64 > GRID_CAP * 256
    ref = _reference(c, form)
    rc, dh, grads = _wide_bwd(mp, c, ref.ps, form)
    assert rc == 0, (rc, mp.lib().msmp_last_error())
    _check(mp, c, ref, form, f'{case}/{form}', dh, grads)
    if case == 'edge-big' and form == 'gated':          # no atomics anywhere: bitwise reproducible
        rc2, dh2, grads2 = _wide_bwd(mp, c, ref.ps, form)
        assert rc2 == 0
        assert torch.equal(dh, dh2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


@pytest.mark.parametrize('form', ['lin', 'gated'])
def test_edgeless_batch(mp, form):
    """E = 0: the gradients of message_net_1 / _2 are exactly zero, dh and the update layers are within the bars."""
    c = _inputs(1, 0, 164, 25, 3)
    ref = _reference(c, form)
    rc, dh, grads = _wide_bwd(mp, c, ref.ps, form)
    assert rc == 0, (rc, mp.lib().msmp_last_error())
    for head in range(2 if form == 'gated' else 1):
        for i in range(4):
            assert bool((grads[8 * head + i] == 0).all()), (head, i)
            assert bool((ref.grads[8 * head + i] == 0).all())
    _check(mp, c, ref, form, f'edgeless/{form}', dh, grads)


@pytest.mark.parametrize('form', ['lin', 'gated'])
def test_one_graph_and_eps(mp, form):
    """A batch of one 100-node graph, once with the default eps and once with eps = 1e-2 (InstanceNorm takes it from the call)."""
    c = _inputs(0, 600, 164, 25, 3, sizes=[100])
    assert c.n == 100 and c.n_graphs == 1
    for eps in (EPS, 1e-2):
        ref = _reference(c, form, eps=eps)
        rc, dh, grads = _wide_bwd(mp, c, ref.ps, form, eps=eps)
        assert rc == 0, (rc, mp.lib().msmp_last_error())
        _check(mp, c, ref, form, f'one-graph/eps{eps:g}/{form}', dh, grads)
    ref_default = _reference(c, form, eps=EPS)
    assert (ref_default.dh - ref.dh).abs().max().item() > 2 * ref.dh_bar       # the bars tell the two eps apart


# ---- the host path ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def glu_layers(mp):
    """one gated pair of layers of an MSGMP-PDE model (hidden width 164)"""
    torch.manual_seed(3)
    case = synthetic_case(mp, 'E2', bsz=2, seed=4)
    model = mp.MODEL_NAMES['MSGMP-PDE'](case.pde, time_window=25, eq_variables=case.eqv, hidden_layer=2).cuda()
    main, gate = model.gnn_layers[0], model.gnn_layers_gate[0]
    assert main.hidden_features == 164 and main.wide and main.time_window == 25
    return main, gate


def _host_grads(mp, c, main, gate):
    from msmp_pde_amd import layers
    params = list(main._params8()) + list(gate._params8())
    h = c.h.clone().requires_grad_(True)
    out = layers.mp_layer(h, c.u, c.pos, c.var, c.gs, main, gate, EPS)
    grads = torch.autograd.grad(out, [h] + params, c.gout)
    torch.cuda.synchronize()
    return out, grads[0], list(grads[1:])


def _check_host(mp, c, ref, label, dh, grads):
    ld = ld_of(c.W)
    _check(mp, c, ref, 'gated', label, _padded(dh, ld), grads)


@pytest.mark.parametrize('setting', [1, 0])
def test_host_layer_under_autograd(mp, glu_layers, setting):
    """layers.mp_layer on one gated pair of an MSGMP-PDE model under autograd with "wide_bwd" forced to 1 and to 0: the gradients of h and of
    the 16 parameters are within the bars of the float64 reference on both; on 1 MPLayerFunction is on the graph and two backward passes
    are bitwise equal."""
    main, gate = glu_layers
    c = _inputs(1, 2000, 164, 25, main.n_variables)
    ps = [p.detach() for p in list(main._params8()) + list(gate._params8())]
    ref = _reference(c, 'gated', ps=ps)
    with tuned(mp.lib(), wide_bwd=setting):
        out, dh, grads = _host_grads(mp, c, main, gate)
        on_graph = 'MPLayerFunction' in type(out.grad_fn).__name__
        assert on_graph == bool(setting), type(out.grad_fn).__name__
        _check_host(mp, c, ref, f'host/wide_bwd{setting}', dh, grads)
        if setting:
            _, dh2, grads2 = _host_grads(mp, c, main, gate)
            assert torch.equal(dh, dh2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


def test_host_layer_falls_back_where_the_entry_refuses(mp, glu_layers, monkeypatch):
    """Sizes the entry refuses by value (its workspace query returns 0) keep the PyTorch ops, and still meet the bars."""
    main, gate = glu_layers
    c = _inputs(1, 2000, 164, 25, main.n_variables)
    ps = [p.detach() for p in list(main._params8()) + list(gate._params8())]
    ref = _reference(c, 'gated', ps=ps)
    L = mp.lib()
    monkeypatch.setattr(L, 'msmp_wide_layer_bwd_workspace_bytes', lambda *a: 0)
    with tuned(L, wide_bwd=1):
        out, dh, grads = _host_grads(mp, c, main, gate)
    assert 'MPLayerFunction' not in type(out.grad_fn).__name__
    _check_host(mp, c, ref, 'host/refused', dh, grads)


def test_capture(mp, glu_layers):
    """Forward + backward of one gated layer at width 164 captured with torch.cuda.graph on one stream after a warm-up, replayed with two
    different h / grad_out contents copied into the static tensors: each replay equals the eager call bit for bit."""
    from msmp_pde_amd import layers
    main, gate = glu_layers
    c = _inputs(1, 2000, 164, 25, main.n_variables)
    params = list(main._params8()) + list(gate._params8())
    gen = torch.Generator(device='cuda').manual_seed(9)
    contents = [(torch.randn(c.n, 164, generator=gen, device='cuda'), torch.randn(c.n, 164, generator=gen, device='cuda')) for _ in range(2)]
    h_s = c.h.clone().requires_grad_(True)
    g_s = c.gout.clone()

    def step():
        out = layers.mp_layer(h_s, c.u, c.pos, c.var, c.gs, main, gate, EPS)
        return [out] + list(torch.autograd.grad(out, [h_s] + params, g_s))

    with tuned(mp.lib(), wide_bwd=1):
        eager = []
        for hv, gv in contents:
            with torch.no_grad():
                h_s.copy_(hv)
                g_s.copy_(gv)
            eager.append([t.detach().clone() for t in step()])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                step()
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static = step()
        for (hv, gv), want in zip(contents, eager):
            with torch.no_grad():
                h_s.copy_(hv)
                g_s.copy_(gv)
                for t in static:
                    t.detach().fill_(float('nan'))
            graph.replay()
            torch.cuda.synchronize()
            assert len(static) == 18
            assert all(torch.equal(a.detach(), b) for a, b in zip(static, want))
        assert not torch.equal(eager[0][1], eager[1][1])
