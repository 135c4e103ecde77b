"""GPU tests of the training backward at the sizes where its kernels switch (layer_bwd_kernel.hip, rows_gemm_kernel.hip).

`rows_gemm` runs `rows_gemm_small_kernel` (32-row workgroups, no LDS) below RG_SMALL_ROWS = 32 768 rows and `rows_gemm_kernel`
(128-row workgroups, weights double-buffered through LDS, 16-byte epilogue stores) from there on; the elementwise and scatter
kernels of the backward cap their grids (`grid_for`: 32 768 blocks; `msmp_edge_concat_f32`: 16 384; `msmp_mean_bwd_dswish_f32`:
65 536) and rely on a grid-stride loop beyond the cap.  The other test files stay on the small side of every one of these
switches; this file crosses each of them, and also runs the call form of `msmp_mp_layer_bwd_f32` without the by-source arrays
(per-edge message_net_1, `scatter_source_kernel` with float atomics) that the host layer never uses."""
import ctypes
from types import SimpleNamespace

import pytest
import torch

from helpers import record_parity, FLOOR_FACTOR

pytestmark = pytest.mark.gpu

RG_SMALL_ROWS = 32768                 # rows_gemm: rows_gemm_small_kernel below, rows_gemm_kernel from here on
GRID_FOR_ROWS = 32768 * 256 // 32     # grid_for: 32 768 blocks of 256 threads, a thread = (row, 16-byte channel group): 262 144 rows
PATTERN = [1, 100, 3, 130, 2]         # nodes per graph, repeated; every batch ends in one more 100-node graph
EPS = 1e-5
UNSUPPORTED = -2                      # MSMP_ERR_UNSUPPORTED (include/msmp_pde.h)

# case -> (pattern repeats, edges, time window, variables)
CASES = {
    'edge-big': (5, 33001, 25, 3),
    'node-big': (139, 20000, 25, 3),
    'wide-tail': (139, 33001, 100, 3),
    'strided': (1111, 270001, 25, 3),
}
# P1: own GEMMs, factorised message_net_1 (the default);  P2: own GEMMs, per-edge message_net_1 and the atomic source scatter
# (src_rowptr = src_perm = NULL);  P3: rocblas_sgemm + the separate epilogue kernels (tune "bwd_gemm" = 0)
PATHS = {'P1': dict(by_source=True, bwd_gemm=2), 'P2': dict(by_source=False, bwd_gemm=2), 'P3': dict(by_source=True, bwd_gemm=0)}
SUB_REPEATS = 60                      # the sub-batch of the node-big row comparison: 14 160 nodes, on the small kernels


@pytest.fixture(scope='module')
def mp():
    import msmp_pde_amd
    assert torch.cuda.is_available()
    return msmp_pde_amd


_cache = {}           # at most one batch and one reference at a time (the tests that share them are adjacent)


@pytest.fixture(scope='module', autouse=True)
def _release_memory():
    yield
    from msmp_pde_amd import autograd as A
    _cache.clear()
    A._bwd_ws.clear()
    torch.cuda.empty_cache()


def _inputs(case):
    """The ragged batch of `case` and random layer inputs, the same for every form and path."""
    if _cache.get('inputs_key') == case:
        return _cache['inputs']
    _cache.clear()
    torch.cuda.empty_cache()
    from msmp_pde_amd.graph import GraphStructure
    k, e, tw, nv = CASES[case]
    sizes = torch.tensor(PATTERN * k + [100])
    n = int(sizes.sum())
    starts = torch.cumsum(sizes, 0) - sizes
    g = torch.Generator(device='cpu').manual_seed(21 + k)
    # random edges inside the 100- and 130-node graphs only; the last 7 nodes of each stay without in-edges
    big = torch.nonzero(sizes >= 100)[:, 0]
    pick = big[torch.randint(0, big.numel(), (e,), generator=g)]
    z, s0 = sizes[pick], starts[pick]
    src = s0 + torch.minimum((torch.rand(e, generator=g, dtype=torch.float64) * z).long(), z - 1)
    dst = s0 + torch.minimum((torch.rand(e, generator=g, dtype=torch.float64) * (z - 7)).long(), z - 8)
    c = SimpleNamespace(case=case, n=n, e=e, tw=tw, nv=nv, k=k, n_graphs=int(sizes.numel()))
    c.ei = torch.stack([src, dst]).cuda()
    c.batch = torch.repeat_interleave(torch.arange(sizes.numel()), sizes).cuda()
    c.gs = GraphStructure(c.ei, c.batch, n)
    assert c.gs.n_edges == e and c.gs.n_graphs == c.n_graphs
    gc = torch.Generator(device='cuda').manual_seed(5 + k)
    r = lambda *s: torch.randn(*s, generator=gc, device='cuda')
    c.h, c.u, c.pos, c.var, c.gout = r(n, 128), r(n, tw), r(n), r(n, nv), r(n, 128)
    # rows compared in dh: all but the 1- and 2-node graphs (InstanceNorm's derivative is ill-conditioned there)
    gi = c.batch
    c.multi = ~((gi < 5 * k) & ((gi % 5 == 0) | (gi % 5 == 4)))
    excluded = n - int(c.multi.sum())
    assert excluded == 3 * k and excluded <= 0.02 * n
    assert sizes[-1] == 100 and bool(c.multi[-1])          # the ragged last row block is compared, not masked
    _cache.update(inputs_key=case, inputs=c)
    return c


def _params(c, form):
    g = torch.Generator(device='cpu').manual_seed(77 + c.k + len(form))
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    k1, k3 = 256 + c.tw + 1 + c.nv, 256 + c.nv
    one = lambda: [r(128, k1) / k1 ** 0.5, r(128) * 0.1, r(128, 128) / 128 ** 0.5, r(128) * 0.1,
                   r(128, k3) / k3 ** 0.5, r(128) * 0.1, r(128, 128) / 128 ** 0.5, r(128) * 0.1]
    return one() + (one() if form == 'gated' else [])


def _autograd(c, ps, form, dtype):
    """dL/dh and the parameter gradients by torch.autograd over A.layer_reference in `dtype` (no kernel of the library involved)."""
    from msmp_pde_amd import autograd as A
    h = c.h.to(dtype, copy=True).requires_grad_(True)
    p = [q.to(dtype, copy=True).requires_grad_(True) for q in ps]
    args = (c.u.to(dtype), c.pos.to(dtype), c.var.to(dtype), c.gs.col_long, c.gs.tgt_long, c.batch, c.n_graphs)
    if form == 'gated':
        tau = torch.sigmoid(A.layer_reference(h, *args, p[8:], True, EPS))
        out = (1 - tau) * h + tau * A._swish(A.layer_reference(h, *args, p[:8], True, EPS))
    else:
        out = A.layer_reference(h, *args, p, form == 'lin', EPS)
    out.backward(c.gout.to(dtype))
    return h.grad, [q.grad for q in p]


def _dh_err(c, dh, ref):
    return ((dh.double() - ref)[c.multi]).abs().max().item()


def _reference(c, form):
    """Float64 reference, the float32 floor against it (per tensor) and the bars, once per (case, form)."""
    key = (c.case, form)
    if _cache.get('ref_key') == key:
        return _cache['ref']
    _cache.pop('ref', None)
    ps = _params(c, form)
    dh64, g64 = _autograd(c, ps, form, torch.float64)
    dh32, g32 = _autograd(c, ps, form, torch.float32)
    ref = SimpleNamespace(ps=ps, dh=dh64, grads=g64)
    ref.scale = max(q.abs().max().item() for q in g64)
    ref.dh_floor = _dh_err(c, dh32, dh64)
    ref.p_floor = [(a.double() - b).abs().max().item() for a, b in zip(g32, g64)]
    # the bars of the small-size test (test_layer_backward_entry_vs_float64_autograd), or twice what float32 autograd delivers
    ref.dh_small = 2e-4 * max(dh64.abs().max().item(), 1.0)
    ref.p_small = [1e-4 * q.abs().max().item() + 2e-5 * ref.scale for q in g64]
    ref.dh_bar = max(ref.dh_small, FLOOR_FACTOR * ref.dh_floor)
    ref.p_bar = [max(s, FLOOR_FACTOR * f) for s, f in zip(ref.p_small, ref.p_floor)]
    del dh32, g32
    _cache.update(ref_key=key, ref=ref)
    return ref


def _layer_bwd(mp, c, ps, form, by_source=True, bwd_gemm=2, sub=None):
    """msmp_mp_layer_bwd_f32 through the C-ABI, modelled on autograd.layer_backward_native: -> (return code, dh, grads).
    by_source=False passes NULL for src_rowptr and src_perm; `bwd_gemm` is set for the call only.  The workspace carries its own
    1-KB guard bands (it is larger than what conftest.py guards); dh and the gradients come from torch.empty (guarded there).
    sub = (GraphStructure, n): run on the first n rows of the inputs with that structure."""
    from msmp_pde_amd._lib import check, ptr, current_stream
    L = mp.lib()
    gs, n = sub if sub else (c.gs, c.n)
    e, gated = gs.n_edges, form == 'gated'
    h, u, pos, var, gout = (t[:n] for t in (c.h, c.u, c.pos, c.var, c.gout))
    grads = [torch.empty(q.shape, dtype=torch.float32, device='cuda') for q in ps]
    dh = torch.empty(n, 128, dtype=torch.float32, device='cuda')
    need = L.msmp_mp_layer_bwd_workspace_bytes(n, e, c.tw, c.nv, int(gated))
    assert need > 0
    raw = torch.full((need + 2048,), 0x5A, dtype=torch.uint8, device='cuda')
    arr = lambda ts: (ctypes.c_void_p * 8)(*[t.data_ptr() for t in ts])
    perm32, src_rowptr = gs.by_source32() if by_source else (None, None)
    p_main, p_gate, g_main, g_gate = arr(ps[:8]), arr(ps[8:]) if gated else None, arr(grads[:8]), arr(grads[8:]) if gated else None
    prev = L.msmp_tune_query(b'bwd_gemm')
    check(L.msmp_tune(b'bwd_gemm', bwd_gemm), 'tune')
    try:
        rc = L.msmp_mp_layer_bwd_f32(ptr(gout), ptr(h), ptr(u), ptr(pos), ptr(var), ptr(gs.rowptr), ptr(gs.col), ptr(gs.tgt),
                                     ptr(src_rowptr), ptr(perm32), ptr(gs.graph_ptr), n, e, gs.n_graphs, c.tw, c.nv, p_main, p_gate,
                                     0 if form == 'residual' else 1, EPS, ptr(dh), g_main, g_gate, raw.data_ptr() + 1024, need,
                                     current_stream())
    finally:
        check(L.msmp_tune(b'bwd_gemm', prev), 'tune')
    torch.cuda.synchronize()
    assert bool((raw[:1024] == 0x5A).all()) and bool((raw[1024 + need:] == 0x5A).all()), 'workspace guard band overwritten'
    del raw
    return rc, dh, grads


def _assert_crossed(c):
    """Every case must stay on its side of the switches, whatever becomes of the shapes."""
    if c.case == 'edge-big':
        assert c.e >= RG_SMALL_ROWS > c.n and c.e % 128 == 105
    elif c.case == 'node-big':
        assert c.n >= RG_SMALL_ROWS > c.e and c.n % 128 == 8
    elif c.case == 'wide-tail':
        assert c.n >= RG_SMALL_ROWS and c.e >= RG_SMALL_ROWS and c.tw + 1 + c.nv > 64
        assert 128 + 32 * ((c.tw + 1 + c.nv + 31) // 32) == 256         # fact_ldf: 8 chunks
    else:
        assert c.n > GRID_FOR_ROWS and c.e > GRID_FOR_ROWS


_MAIN = [(case, form, path)
         for case, forms, paths in (('edge-big', ('residual', 'lin', 'gated'), ('P1', 'P2', 'P3')),
                                    ('node-big', ('residual', 'lin', 'gated'), ('P1', 'P2', 'P3')),
                                    ('wide-tail', ('residual', 'gated'), ('P1',)),
                                    ('strided', ('residual', 'gated'), ('P1', 'P2', 'P3')))
         for form in forms for path in paths]


@pytest.mark.parametrize('case,form,path', _MAIN, ids=['-'.join(t) for t in _MAIN])
def test_layer_backward_vs_float64_at_switching_sizes(mp, case, form, path):
    """msmp_mp_layer_bwd_f32: dL/dh and all 8 / 16 parameter gradients against float64 torch.autograd over A.layer_reference.
    edge-big (E = 33 001 >= 32 768 > N): the edge-row GEMMs on rows_gemm_kernel<0, 2, 3> with a ragged last 128-row block (E % 128 =
    105), K = 285 (9 chunks, K % 4 = 1) on P2;  node-big (N = 32 904 >= 32 768 > E): the node-row GEMMs on rows_gemm_kernel<0, 1, 2, 3,
    5>, K = 259 and ldf = 160;  wide-tail (tw + 1 + nv = 104 > 64): factorised only, ldf = 256 = 8 chunks, both row counts on the big
    kernel;  strided (N, E > 262 144): every grid_for launch takes a second grid-stride pass.  P1 factorised message_net_1, P2 per-edge
    message_net_1 with scatter_source_kernel (atomics), P3 rocblas_sgemm + separate epilogues.  Bar per tensor: the small-size bar
    of test_layer_backward_entry_vs_float64_autograd or twice the error of float32 torch.autograd on the same inputs, whichever
    is larger.  P1 and P3 repeat bit for bit."""
    c = _inputs(case)
    _assert_crossed(c)
    ref = _reference(c, form)
    rc, dh, grads = _layer_bwd(mp, c, ref.ps, form, **PATHS[path])
    assert rc == 0, (rc, mp.lib().msmp_last_error())
    assert torch.isfinite(dh).all() and all(torch.isfinite(g).all() for g in grads)
    dh_err = _dh_err(c, dh, ref.dh)
    p_err = [(g.double() - q).abs().max().item() for g, q in zip(grads, ref.grads)]
    worst = max(range(len(p_err)), key=lambda i: p_err[i] / ref.p_bar[i])
    print(f'{case}/{form}/{path}: dh err {dh_err:.3e} floor {ref.dh_floor:.3e} bar {ref.dh_bar:.3e}; worst parameter {worst}: '
          f'err {p_err[worst]:.3e} floor {ref.p_floor[worst]:.3e} bar {ref.p_bar[worst]:.3e}')
    record_parity('layer_backward_sizes', f'{case}/{form}/{path}', n_nodes=c.n, n_edges=c.e, dh_err=dh_err, dh_floor=ref.dh_floor,
                  dh_bar=ref.dh_bar, dh_ratio=dh_err / ref.dh_bar, worst_param=worst, param_err=p_err[worst],
                  param_floor=ref.p_floor[worst], param_bar=ref.p_bar[worst], param_ratio=p_err[worst] / ref.p_bar[worst])
    assert dh_err < ref.dh_bar, (dh_err, ref.dh_floor, ref.dh_bar)
    for i, (got, q) in enumerate(zip(grads, ref.grads)):
        assert got.shape == q.shape
        assert p_err[i] < ref.p_bar[i], (i, p_err[i], ref.p_floor[i], ref.p_bar[i])
    if path != 'P2':          # no atomics on these paths: bitwise reproducible (P2's source scatter does not fix the summation order)
        rc2, dh2, grads2 = _layer_bwd(mp, c, ref.ps, form, **PATHS[path])
        assert rc2 == 0
        assert torch.equal(dh, dh2) and all(torch.equal(a, b) for a, b in zip(grads, grads2))


@pytest.mark.parametrize('form', ['residual', 'gated'])
@pytest.mark.parametrize('path', ['P2', 'P3'])
def test_wide_tail_refuses_per_edge_and_rocblas_paths(mp, form, path):
    """tw + 1 + nv = 104 > 64 at N, E >= 32 768: without the by-source arrays (P2) or with rocblas_sgemm (P3) the per-edge weight
    gradient would have 360 columns, past the weight-gradient kernel: the entry returns MSMP_ERR_UNSUPPORTED before any launch."""
    c = _inputs('wide-tail')
    _assert_crossed(c)
    rc, dh, grads = _layer_bwd(mp, c, _params(c, form), form, **PATHS[path])
    assert rc == UNSUPPORTED, rc


@pytest.mark.parametrize('form', ['residual', 'lin', 'gated'])
def test_node_big_rows_equal_small_kernel_rows(mp, form):
    """The claim at rows_gemm_small_kernel ("same arithmetic order per output element as rows_gemm_kernel: bit-identical results") for
    epilogues 0, 1, 2, 3 and 5 inside the layer backward: the dh rows of the node-big batch (N = 32 904: node-row GEMMs on
    rows_gemm_kernel) equal, bit for bit, the dh rows of its first 60 pattern repeats evaluated on their own (14 160 nodes with their
    own edges: everything on rows_gemm_small_kernel).  Every other step is per row or per graph with a fixed order."""
    from msmp_pde_amd.graph import GraphStructure
    c = _inputs('node-big')
    _assert_crossed(c)
    n_sub = SUB_REPEATS * sum(PATTERN)
    ei_sub = c.ei[:, c.ei[1] < n_sub]
    assert bool((ei_sub[0] < n_sub).all())
    gs_sub = GraphStructure(ei_sub.contiguous(), c.batch[:n_sub], n_sub)
    assert n_sub < RG_SMALL_ROWS and 0 < gs_sub.n_edges < RG_SMALL_ROWS and gs_sub.n_graphs == 5 * SUB_REPEATS
    ps = _params(c, form)
    rc, dh, _ = _layer_bwd(mp, c, ps, form)
    rc_sub, dh_sub, _ = _layer_bwd(mp, c, ps, form, sub=(gs_sub, n_sub))
    assert rc == 0 and rc_sub == 0
    assert torch.isfinite(dh).all()
    diff = (dh[:n_sub] != dh_sub).any(1)
    assert torch.equal(dh[:n_sub], dh_sub), f'{int(diff.sum())} of {n_sub} rows differ, first {int(torch.nonzero(diff)[0])}'


ROWS = RG_SMALL_ROWS + 77             # a ragged last 128-row block, and no multiple of 32 either
SPLIT = 16384                         # the same rows in two calls of 16 384 and 16 461 rows: both on rows_gemm_small_kernel


@pytest.mark.parametrize('k,n_out,mode', [(4, 128, 1), (28, 5, 0), (64, 164, 2), (164, 164, 1), (331, 164, 1), (1024, 300, 0)])
def test_linear_on_128_row_kernel(mp, k, n_out, mode):
    """msmp_linear_f32 at 32 845 rows (>= 32 768: rows_gemm_kernel<1>, <4>, <5>; 32 845 % 128 = 77): one chunk (k = 4), one partial
    chunk (28), two chunks (64: the even branch of the chunk loop), six chunks with K % 32 != 0 (164), eleven chunks with K % 4 != 0
    (331: odd count, scalar tail loads), 32 chunks with three column groups and a partial last one (1024 -> 300).  Against the float64
    product at the bar of test_general_linear_kernel; the same rows in two calls that stay on rows_gemm_small_kernel must give the
    same bits (the "bit-identical" claim at rows_gemm_small_kernel)."""
    from msmp_pde_amd._lib import check, ptr, current_stream
    L = mp.lib()
    assert ROWS >= RG_SMALL_ROWS and ROWS % 128 and ROWS % 32 and SPLIT < RG_SMALL_ROWS and ROWS - SPLIT < RG_SMALL_ROWS
    g = torch.Generator(device='cpu').manual_seed(ROWS + k)
    ldx = (k + 3) // 4 * 4 + 4
    groups = 128 * ((n_out + 127) // 128)
    ld_out = groups + 8
    x = torch.randn(ROWS, ldx, generator=g).cuda()
    w = (torch.randn(n_out, k, generator=g) / k ** 0.5).cuda()
    b = torch.randn(n_out, generator=g).cuda()
    need = L.msmp_linear_workspace_bytes(k, n_out)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')

    def run(r0, r1, out):
        check(L.msmp_linear_f32(x[r0:].data_ptr(), ldx, r1 - r0, k, ptr(w), k, ptr(b), n_out, mode, out[r0:].data_ptr(), ld_out,
                                ptr(ws), need, current_stream()), 'msmp_linear_f32')

    out = torch.empty(ROWS, ld_out, dtype=torch.float32, device='cuda').fill_(0.25)
    run(0, ROWS, out)
    acc = x[:, :k].double() @ w.double().t()
    z = acc + b.double()
    ref = {0: z, 1: z * torch.sigmoid(z), 2: acc + 0.25}[mode]
    err = (out[:, :n_out].double() - ref).abs().max().item()
    print(f'linear {ROWS}x{k}->{n_out} mode {mode}: max error {err:.2e}')
    assert err < 2e-6 * max(1.0, ref.abs().max().item())
    assert bool((out[:, n_out:groups] == (0.25 if mode == 2 else 0.0)).all())      # padded columns: f(0 + 0) (accumulate: untouched + 0)
    assert bool((out[:, groups:] == 0.25).all())                                   # beyond the groups: untouched
    halves = torch.empty(ROWS, ld_out, dtype=torch.float32, device='cuda').fill_(0.25)
    run(0, SPLIT, halves)
    run(SPLIT, ROWS, halves)
    assert torch.equal(out, halves)


@pytest.mark.parametrize('k,n_out', [(36, 128), (288, 384)])
def test_linear_swish_on_128_row_kernel(mp, k, n_out):
    """msmp_linear_swish_f32 at 32 845 rows (rows_gemm_kernel<4>, ragged last 128-row block): two chunks with K % 32 = 4, and nine
    chunks (odd count) with three column groups.  Against float64 at the bar of test_linear_swish_vs_float64, and bit for bit
    against the same rows in two calls on rows_gemm_small_kernel."""
    from msmp_pde_amd._lib import check, ptr, current_stream
    L = mp.lib()
    assert ROWS >= RG_SMALL_ROWS and SPLIT < RG_SMALL_ROWS and ROWS - SPLIT < RG_SMALL_ROWS
    g = torch.Generator(device='cpu').manual_seed(ROWS + k)
    x = torch.randn(ROWS, k, generator=g).cuda()
    w = (torch.randn(n_out, k, generator=g) / k ** 0.5).cuda()
    b = (torch.randn(n_out, generator=g) * 0.1).cuda()
    need = L.msmp_linear_swish_workspace_bytes(k, n_out)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')

    def run(r0, r1, out):
        check(L.msmp_linear_swish_f32(x[r0:].data_ptr(), r1 - r0, k, ptr(w), ptr(b), n_out, out[r0:].data_ptr(), ptr(ws), need,
                                      current_stream()), 'msmp_linear_swish_f32')

    out = torch.empty(ROWS, n_out, dtype=torch.float32, device='cuda').fill_(float('nan'))
    run(0, ROWS, out)
    z = x.double() @ w.double().t() + b.double()
    ref = z * torch.sigmoid(z)
    err = (out.double() - ref).abs().max().item()
    print(f'linear_swish {ROWS}x{k}->{n_out}: max error {err:.2e}')
    assert err < 2e-6 * max(ref.abs().max().item(), 1.0)
    halves = torch.empty(ROWS, n_out, dtype=torch.float32, device='cuda').fill_(float('nan'))
    run(0, SPLIT, halves)
    run(SPLIT, ROWS, halves)
    assert torch.equal(out, halves)


def test_glue_entry_points_past_their_grid_caps(mp):
    """msmp_edge_concat_f32 at E = 65 536 + 9 (its grid is capped at 16 384 blocks of four waves, a wave per edge: from 65 537 edges on
    a wave takes a second edge), bit-exact against the torch gather and concat for tails of 29 and 104 columns; msmp_mean_bwd_dswish_f32
    at E = 524 288 + 9 (capped at 65 536 blocks, a thread per edge and 16-byte channel group: a second grid-stride pass from 524 289
    edges on) against float64 autograd at the 1e-5 of test_backward_glue_kernels_match_float64_autograd."""
    from msmp_pde_amd._lib import check, ptr, current_stream
    from msmp_pde_amd import autograd as A
    L = mp.lib()
    g = torch.Generator(device='cpu').manual_seed(5)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    n = 3000

    def edges(e):
        tgt = torch.sort(torch.randint(0, n - 7, (e,), generator=g))[0].int().cuda()       # the last nodes have no in-edges
        col = torch.randint(0, n, (e,), generator=g).int().cuda()
        return tgt, col

    e = 65536 + 9
    assert (e + 3) // 4 > 16384
    tgt, col = edges(e)
    i, j = tgt.long(), col.long()
    h = r(n, 128)
    for tw, nv in ((25, 3), (100, 3)):
        u, pos, var = r(n, tw), r(n), r(n, nv)
        k = 256 + tw + 1 + nv
        ld = (k + 3) // 4 * 4
        out = torch.empty(e, ld, dtype=torch.float32, device='cuda').fill_(float('nan'))
        check(L.msmp_edge_concat_f32(ptr(h), ptr(u), ptr(pos), ptr(var), ptr(tgt), ptr(col), e, tw, nv, ld, ptr(out),
                                     current_stream()), 'edge_concat')
        ref = torch.cat((h[i], h[j], u[i] - u[j], (pos[i] - pos[j])[:, None], var[i]), 1)
        assert torch.equal(out[:, :k], ref)
        del out, ref

    e = 524288 + 9
    assert (e * 32 + 255) // 256 > 65536
    tgt, col = edges(e)
    i = tgt.long()
    rowptr = torch.zeros(n + 1, dtype=torch.int32, device='cuda')
    rowptr[1:] = torch.cumsum(torch.bincount(i, minlength=n), 0).int()
    gc = torch.Generator(device='cuda').manual_seed(6)
    a2, dagg = torch.randn(e, 128, generator=gc, device='cuda'), r(n, 128)
    got = torch.empty_like(a2)
    check(L.msmp_mean_bwd_dswish_f32(ptr(dagg), ptr(rowptr), ptr(tgt), ptr(a2), e, ptr(got), current_stream()), 'mean_bwd')
    a64 = a2.double().requires_grad_(True)
    A._seg_mean(A._swish(a64), i, n).backward(dagg.double())
    err = (got.double() - a64.grad).abs().max().item()
    print(f'mean_bwd_dswish E = {e}: max error {err:.2e}')
    assert err < 1e-5
    del a64, got, a2
