"""The message-passing layer at a hidden width other than 128 (the GLU classes: 164): GNN_LayerLin, or a gated pair of them, on the
width-generic HIP kernels (experiments/models_gnn.py:88-149, 1486-1489).

Every piece has a fused edition (one launch, operands packed per layer: `_MPLayerBase.wide_blob`) and the unfused one it replaced (row
GEMMs of msmp_linear_f32 around the HBM-bound kernels of wide_kernels.hip, operands: `_MPLayerBase.wide_weights`):
  projections P, Q   msmp_wide_node_proj_f32   |  concatenation + two row GEMMs per head
  message + mean     msmp_wide_message_f32     |  gather-Swish + row GEMM + scatter-mean
  node tail          msmp_wide_node_tail_f32   |  concatenation + two row GEMMs per head + norm / blend
`_wide_fused` is the one test of the switches; a fused entry that refuses its arguments by value (`_entry_taken`) leaves the piece to
the unfused edition.  `layers.mp_layer` dispatches here.
"""
import torch
import torch.nn.functional as F

from ._lib import lib, check, ptr, current_stream, node_features, _Workspace, MsmpError, MSMP_ERR_UNSUPPORTED, MSMP_LAYER_LIN


def row_stride(W):
    """Row stride of the [N, W] activations of this path: W rounded up to the 128-column groups msmp_linear_f32 writes."""
    return 128 * ((W + 127) // 128)


def _wide_fused(*keys):
    """True while every switch of the fused width-generic path is on: "wide_msg", "split", "lem_wide" and the given further keys.
    (msmp_tune("lem_wide", 0) selects the unfused width-generic path as a WHOLE: the model is then independent of "split", bitwise the
    exact-fp32 evaluation, which is what that setting is compared against; each switch at 0 keeps selecting exactly the path it
    selected before the later kernels existed.)"""
    L = lib()
    return all(L.msmp_tune_query(k) for k in keys + (b'wide_msg', b'split', b'lem_wide'))


def _entry_taken(name, rc):
    """The return-code rule of the fused entries: MSMP_ERR_UNSUPPORTED (refused by value, nothing launched) -> False, the caller takes
    its fallback; any other code goes through `check` -> True, the piece is done."""
    if rc == MSMP_ERR_UNSUPPORTED:
        return False
    check(rc, name)
    return True


def _wide_linear(x, k, w, bias, n_out, mode, out, ws):
    L = lib()
    check(L.msmp_linear_f32(ptr(x), x.shape[1], x.shape[0], k, ptr(w), w.shape[1], ptr(bias), n_out, mode, ptr(out), out.shape[1],
                            ptr(ws), ws.numel(), current_stream()), 'msmp_linear_f32')


def lemoutput_mlp(mlp, y):
    """lemoutput_mlp (models_gnn.py:1287-1291: Linear + Swish + Linear + Swish) at a width other than 128 as two msmp_linear_f32
    calls with the bias + Swish epilogue (mode 1)."""
    n, W = y.shape
    ld = row_stride(W)
    x = F.pad(y, (0, (-W) % 4)).contiguous()
    w = [p.detach().to(torch.float32).contiguous() for p in (mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias)]
    ws = _Workspace.get(lib().msmp_linear_workspace_bytes(W, W), y.device)
    a = torch.empty(n, ld, dtype=torch.float32, device=y.device)
    b = torch.empty(n, ld, dtype=torch.float32, device=y.device)
    _wide_linear(x, W, w[0], w[1], W, 1, a, ws)
    _wide_linear(a, W, w[2], w[3], W, 1, b, ws)
    b._msmp_keep = w            # the kernels read the weights after this returns
    return b[:, :W].contiguous()


def _padded_rows(x):
    """x [N, K] with K zero-padded to a multiple of 4, contiguous: the row layout msmp_linear_f32 reads."""
    pad = (-x.shape[1]) % 4
    return (F.pad(x, (0, pad)) if pad else x).contiguous()


def _wide_projections(hp, h, u, pos_x, variables, feat, heads, ld, ws):
    """P and Q [N, ld] of every head: the per-node projections of the factorised message_net_1 (experiments/models_gnn.py:132-138)."""
    L = lib()
    n, dev = hp.shape[0], hp.device
    W, tw, nv = heads[0].hidden_features, u.shape[1], variables.shape[1]
    PQ = [(torch.empty(n, ld, dtype=torch.float32, device=dev), torch.empty(n, ld, dtype=torch.float32, device=dev)) for _ in heads]
    # all of them as ONE launch, nothing concatenated in memory (wide_node_proj_kernel.hip); more feature columns than the kernel takes are
    # refused by value and take the row GEMMs below
    if _wide_fused(b'wide_proj') and heads[0].time_window == tw and heads[0].n_variables == nv:
        blobs = [layer.wide_blob('proj') for layer in heads]
        if all(b is not None for b in blobs):
            if feat is None:
                feat = node_features(u, pos_x, variables)
            gated = len(heads) == 2
            rc = L.msmp_wide_node_proj_f32(ptr(hp), ptr(feat), n, tw, nv, W, ld, ptr(blobs[0]), ptr(blobs[1]) if gated else None, ptr(PQ[0][0]),
                                           ptr(PQ[0][1]), ptr(PQ[1][0]) if gated else None, ptr(PQ[1][1]) if gated else None, current_stream())
            if _entry_taken('msmp_wide_node_proj_f32', rc):
                return PQ
    feat_cat = torch.cat((h, u, pos_x.reshape(-1, 1), variables), 1)
    k_feat = feat_cat.shape[1]
    feat_cat = _padded_rows(feat_cat)
    for layer, (P, Q) in zip(heads, PQ):
        wp, wq, b1 = layer.wide_weights()[:3]
        _wide_linear(feat_cat, k_feat, wp, b1, W, 0, P, ws)
        _wide_linear(feat_cat, k_feat, wq, None, W, 0, Q, ws)
    return PQ


def _wide_head_aggregate(P, Q, gs, layer, ld, ws):
    """The message half of one GNN_LayerLin head at hidden width W != 128 from its projections P, Q [N, ld]: the mean aggregate [N, ld]
    (experiments/models_gnn.py:132-138, :107)."""
    L = lib()
    n, W, e = P.shape[0], layer.hidden_features, gs.n_edges
    dev = P.device
    agg = torch.empty(n, ld, dtype=torch.float32, device=dev)
    # the message half as ONE launch, nothing edge-sized in memory (wide_message_kernel.hip); an in-degree above the kernel's cap
    # (msmp_wide_message_max_in_degree) is refused by value and takes the three launches below, like msmp_edge_aggregate_f32 above 256
    if _wide_fused():
        blob = layer.wide_blob('msg')
        if blob is not None:
            rc = L.msmp_wide_message_f32(ptr(P), ptr(Q), ptr(gs.rowptr), ptr(gs.col), n, e, gs.max_in_degree, W, ld, ptr(blob), ptr(agg),
                                         current_stream())
            if _entry_taken('msmp_wide_message_f32', rc):
                return agg
    w2, b2 = layer.wide_weights()[3:5]
    a1 = torch.empty(max(e, 1), ld, dtype=torch.float32, device=dev)
    check(L.msmp_wide_gather_swish_f32(ptr(P), ptr(Q), ptr(gs.tgt), ptr(gs.col), e, W, ld, ptr(a1), current_stream()), 'msmp_wide_gather_swish_f32')
    msg = torch.empty(max(e, 1), ld, dtype=torch.float32, device=dev)
    if e:
        _wide_linear(a1[:e], W, w2, b2, W, 1, msg[:e], ws)
    check(L.msmp_wide_scatter_mean_f32(ptr(msg), ptr(gs.rowptr), n, W, ld, ptr(agg), current_stream()), 'msmp_wide_scatter_mean_f32')
    return agg


def _wide_head_update(h, agg, variables, layer, ld, ws):
    """The update half of one head as two row GEMMs, up to its pre-norm output [N, ld] (experiments/models_gnn.py:140-149)."""
    n, W, dev = h.shape[0], layer.hidden_features, h.device
    w3, b3, w4, b4 = layer.wide_weights()[5:9]
    upd_in = _padded_rows(torch.cat((h[:, :W], agg[:, :W], variables), 1))
    z = torch.empty(n, ld, dtype=torch.float32, device=dev)
    _wide_linear(upd_in, 2 * W + variables.shape[1], w3, b3, W, 1, z, ws)
    y = torch.empty(n, ld, dtype=torch.float32, device=dev)
    _wide_linear(z, W, w4, b4, W, 0, y, ws)
    return y


def _mp_layer_wide(h, u, pos_x, variables, gs, main, gate, eps, feat=None):
    """GNN_LayerLin (or a gated pair of them) at a hidden width other than 128: the HIP path of wide_kernels.hip.  h [N, W].
    feat: the rows of node_features(u, pos_x, variables) where the caller has them (the solvers: once per forward)."""
    L = lib()
    W = main.hidden_features
    if main.MODE != MSMP_LAYER_LIN:
        raise MsmpError('the width-generic layer path implements GNN_LayerLin (the layer of the GLU classes)')
    ld = row_stride(W)
    n = h.shape[0]
    hp = torch.zeros(n, ld, dtype=torch.float32, device=h.device)
    hp[:, :W] = h
    k_max = max(W + u.shape[1] + 1 + variables.shape[1] + 3, 2 * W + variables.shape[1] + 3)
    ws = _Workspace.get(L.msmp_linear_workspace_bytes(k_max, W), h.device)
    heads = [main] if gate is None else [main, gate]
    PQ = _wide_projections(hp, h, u, pos_x, variables, feat, heads, ld, ws)
    aggs = [_wide_head_aggregate(P, Q, gs, layer, ld, ws) for layer, (P, Q) in zip(heads, PQ)]
    out = torch.empty(n, ld, dtype=torch.float32, device=h.device)
    # the node half of the layer as ONE launch (wide_node_tail_kernel.hip).  A graph above the kernel's cap
    # (msmp_wide_node_tail_max_graph_nodes) is refused by value and takes the GEMMs below, like msmp_node_tail_f32 above 128
    if _wide_fused(b'wide_tail') and gs.max_graph_nodes <= L.msmp_wide_node_tail_max_graph_nodes(min(W, 256)):
        blobs = [layer.wide_blob('tail') for layer in heads]
        if all(b is not None for b in blobs):
            rc = L.msmp_wide_node_tail_f32(ptr(hp), ptr(aggs[0]), ptr(aggs[1]) if gate is not None else None, ptr(variables), ptr(gs.graph_ptr), n,
                                           gs.n_graphs, gs.max_graph_nodes, variables.shape[1], W, ld, ptr(blobs[0]),
                                           ptr(blobs[1]) if gate is not None else None, eps, ptr(out), current_stream())
            if _entry_taken('msmp_wide_node_tail_f32', rc):
                return out[:, :W].contiguous()
    ys = [_wide_head_update(hp, agg, variables, layer, ld, ws) for layer, agg in zip(heads, aggs)]
    check(L.msmp_wide_norm_blend_f32(ptr(hp), ptr(ys[1]) if gate is not None else None, ptr(ys[0]), ptr(gs.graph_ptr), gs.n_graphs, W, ld, eps, ptr(out),
                                     current_stream()), 'msmp_wide_norm_blend_f32')
    return out[:, :W].contiguous()


def _mp_layer_wide_autograd(h, u, pos_x, variables, gs, main, gate, eps):
    """The same layer as differentiable PyTorch-ROCm ops: gathers, F.linear, index_add_ mean, InstanceNorm and the blend, formula by
    formula as experiments/models_gnn.py:124-149, 1486-1489.  What layers.mp_layer takes under autograd with msmp_tune("wide_bwd") at 0,
    for float64 inputs and for sizes msmp_wide_layer_bwd_f32 refuses; otherwise training runs _mp_layer_wide + that entry."""
    i, j = gs.tgt_long, gs.col_long
    n = h.shape[0]
    deg = (gs.rowptr[1:] - gs.rowptr[:-1]).clamp(min=1).to(h.dtype)[:, None]
    batch = torch.repeat_interleave(torch.arange(gs.n_graphs, device=h.device), (gs.graph_ptr[1:] - gs.graph_ptr[:-1]).long())
    cnt = (gs.graph_ptr[1:] - gs.graph_ptr[:-1]).clamp(min=1).to(h.dtype)[:, None]
    pos = pos_x.reshape(-1, 1)

    def head(layer):
        sw = lambda x: x * torch.sigmoid(x)
        cat = torch.cat((h[i], h[j], u[i] - u[j], pos[i] - pos[j], variables[i]), -1)
        m = sw(layer.message_net_2[0](sw(layer.message_net_1[0](cat))))
        agg = torch.zeros(n, m.shape[1], dtype=m.dtype, device=m.device).index_add_(0, i, m) / deg
        y = layer.update_net_2[0](sw(layer.update_net_1[0](torch.cat((h, agg, variables), -1))))
        mean = torch.zeros(gs.n_graphs, y.shape[1], dtype=y.dtype, device=y.device).index_add_(0, batch, y) / cnt
        yc = y - mean[batch]
        var = torch.zeros_like(mean).index_add_(0, batch, yc * yc) / cnt
        return yc / torch.sqrt(var + eps)[batch]

    out = head(main)
    if gate is None:
        return out
    tau = torch.sigmoid(head(gate))
    return (1.0 - tau) * h + tau * (out * torch.sigmoid(out))
