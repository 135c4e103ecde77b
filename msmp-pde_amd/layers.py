"""Message-passing layers with the reference's module / parameter names, running on the HIP kernels.

Reference: experiments/models_gnn.py:12-21 (Swish), 23-86 (GNN_Layer), 88-149 (GNN_LayerLin).
state_dict keys are identical (`message_net_1.0.weight` [128, 2*128+tw+1+nv], `message_net_2.0.*`,
`update_net_1.0.weight` [128, 2*128+nv], `update_net_2.0.*`; InstanceNorm has no parameters), so
reference checkpoints load unchanged.  Parameters are created in float32 whatever the default dtype
is (the reference's import side effect makes it float64, temporal/solvers.py:10).
"""
import ctypes

import torch
from torch import nn

from . import _lib
from ._lib import lib, check, ptr, current_stream, HIDDEN, PackedCache, _Workspace, _f32c
from ._lib import node_features      # noqa: F401  (part of this module's interface: the solvers, the scripts and the tests import it from here)
from .graph import GraphStructure
from .wide import _mp_layer_wide, _mp_layer_wide_autograd


class Swish(nn.Module):
    """x * sigmoid(beta x); experiments/models_gnn.py:12-21."""

    def __init__(self, beta=1):
        super().__init__()
        self.beta = beta

    def forward(self, x):
        return x * torch.sigmoid(self.beta * x)


def _linear(i, o):
    return nn.Linear(i, o, dtype=torch.float32)


# The packed operands of the fused width-generic kernels (wide.py), one row per kind: the slice of _params8() it packs, its size entry,
# its pack entry, and the integer arguments of both from (W, tw, nv).  `_MPLayerBase.wide_blob(kind)` builds and caches them.
_WIDE_BLOBS = {
    'proj': (slice(0, 2), 'msmp_packed_wide_proj_floats', 'msmp_pack_wide_proj_f32', lambda W, tw, nv: (W, tw, nv)),    # message_net_1
    'msg': (slice(2, 4), 'msmp_packed_wide_msg_floats', 'msmp_pack_wide_msg_f32', lambda W, tw, nv: (W,)),              # message_net_2
    'tail': (slice(4, 8), 'msmp_packed_wide_tail_floats', 'msmp_pack_wide_tail_f32', lambda W, tw, nv: (W, nv)),        # update_net_1 / _2
}


class _MPLayerBase(nn.Module):
    MODE = None

    def __init__(self, in_features, out_features, hidden_features, time_window, n_variables):
        super().__init__()
        if not (in_features == out_features == hidden_features):
            raise ValueError('in_features, hidden_features and out_features must be equal (they are in every class of the reference)')
        # hidden width 128: the fused kernels.  Any other width (the GLU classes: 164): the width-generic layer of wide_kernels.hip
        # around msmp_linear_f32 (same formulas, HBM-bound pieces; `mp_layer` dispatches on this flag)
        self.wide = hidden_features != HIDDEN
        if not 1 <= n_variables <= _lib.MSMP_MAX_VARS:
            raise ValueError(f'n_variables must be in 1..{_lib.MSMP_MAX_VARS}')
        self.in_features, self.out_features, self.hidden_features = in_features, out_features, hidden_features
        self.time_window, self.n_variables = time_window, n_variables
        self.message_net_1 = nn.Sequential(_linear(2 * in_features + time_window + 1 + n_variables, hidden_features), Swish())
        self.message_net_2 = nn.Sequential(_linear(hidden_features, hidden_features), Swish())
        self.update_net_1 = nn.Sequential(_linear(in_features + hidden_features + n_variables, hidden_features), Swish())
        self._make_update_net_2(hidden_features, out_features)
        # one PackedCache per operand, each a plain attribute: _lib.cached_operands finds them in vars(module)
        self._packed, self._wide_w = PackedCache(), PackedCache()
        for kind in _WIDE_BLOBS:
            setattr(self, '_wide_' + kind, PackedCache())
        self._ps = None

    def _params8(self):
        ps = self._ps
        if ps is None or ps[0] is not self.message_net_1[0].weight:      # (re-)collected when a Parameter object was replaced
            ps = self._ps = (self.message_net_1[0].weight, self.message_net_1[0].bias, self.message_net_2[0].weight,
                             self.message_net_2[0].bias, self.update_net_1[0].weight, self.update_net_1[0].bias,
                             self.update_net_2[0].weight, self.update_net_2[0].bias)
        return ps

    def packed(self):
        """Kernel-layout weight blob (msmp_pack_layer_f32), re-packed only when a parameter changed."""
        if self.wide:
            raise _lib.MsmpError(f'the packed layer blob exists for hidden width {HIDDEN} only')
        ps = self._params8()

        def build():
            L = lib()
            blob = torch.empty(L.msmp_packed_layer_floats(self.time_window, self.n_variables), dtype=torch.float32, device=ps[0].device)
            f = [_f32c(p) for p in ps]
            check(L.msmp_pack_layer_f32(*[ptr(t) for t in f], self.time_window, self.n_variables, ptr(blob),
                                        current_stream()), 'msmp_pack_layer_f32')
            return blob
        return self._packed.get(ps, build)

    def wide_weights(self):
        """The wide path's operands, cached per parameter version: message_net_1 factorised per node (models_gnn.py:132-138):
        P = Wp [h | u | pos | vars] + b1 for the edge's target, Q = Wq [h | u | pos | vars] for its source, with
        Wp = [W1[:, :W] | W1[:, 2W:]], Wq = [W1[:, W:2W] | -W1[:, 2W:2W+tw+1] | 0]."""
        ps = self._params8()

        def build():
            w1 = ps[0].detach().to(torch.float32)
            W, tw = self.hidden_features, self.time_window
            wp = torch.cat((w1[:, :W], w1[:, 2 * W:]), 1).contiguous()
            wq = torch.cat((w1[:, W:2 * W], -w1[:, 2 * W:2 * W + tw + 1], torch.zeros_like(w1[:, 2 * W + tw + 1:])), 1).contiguous()
            return (wp, wq) + tuple(_f32c(p) for p in ps[1:])
        return self._wide_w.get(ps, build)

    def wide_blob(self, kind):
        """One packed operand of the fused width-generic kernels (_WIDE_BLOBS: 'proj', 'msg' or 'tail': fp16 hi / lo fragments of the
        scaled weights, scaled biases), cached per version of the parameters it packs like wide_weights(); None where the kernel does not
        exist (its size entry returns no size: hidden width above 256, more than 128 feature columns)."""
        params, size, pack, ints = _WIDE_BLOBS[kind]
        L = lib()
        ints = ints(self.hidden_features, self.time_window, self.n_variables)
        n_floats = getattr(L, size)(*ints)
        if n_floats <= 0:
            return None
        ps = self._params8()[params]

        def build():
            blob = torch.empty(n_floats, dtype=torch.float32, device=ps[0].device)
            f = [_f32c(p) for p in ps]
            check(getattr(L, pack)(*[ptr(t) for t in f], *ints, ptr(blob), current_stream()), pack)
            return blob
        return getattr(self, '_wide_' + kind).get(ps, build)

    def warm(self):
        """Build every operand an inference forward of this layer can read, on the CURRENT stream (Solver.warm_caches)."""
        if not self.wide:
            self.packed()
            return
        self.wide_weights()
        for kind in _WIDE_BLOBS:
            self.wide_blob(kind)

    def forward(self, x, u, pos, variables, edge_index, batch, structure=None):
        """Same signature as the reference's layer forward (experiments/models_gnn.py:61-67 / 124-130);
        `structure` lets the solver pass the cached CSR instead of rebuilding it from edge_index."""
        if structure is None:
            structure = GraphStructure(edge_index, batch, x.shape[0])
        return mp_layer(x, u, pos, variables, structure, self, None)


class GNN_Layer(_MPLayerBase):
    """experiments/models_gnn.py:23-86: Swish on the last linear and residual x + update."""
    MODE = _lib.MSMP_LAYER_RESIDUAL_SWISH

    def _make_update_net_2(self, h, o):
        self.update_net_2 = nn.Sequential(_linear(h, o), Swish())


class GNN_LayerLin(_MPLayerBase):
    """experiments/models_gnn.py:88-149: no final activation, no residual."""
    MODE = _lib.MSMP_LAYER_LIN

    def _make_update_net_2(self, h, o):
        self.update_net_2 = nn.Sequential(_linear(h, o))


DENSE_MESSAGE = False     # True: evaluate message_net_1 on the per-edge concatenation (reference order of operations)


def _mp_layer_hip(h, u, pos_x, variables, gs, main, gate, eps, dense_message=None, feat=None):
    """The HIP call proper (no autograd): msmp_mp_layer_f32."""
    L = lib()
    n = h.shape[0]
    out = torch.empty_like(h)
    gated = gate is not None
    dense = DENSE_MESSAGE if dense_message is None else dense_message
    mode = main.MODE | (_lib.MSMP_LAYER_DENSE_MESSAGE if dense else 0)
    ws_bytes = L.msmp_mp_layer_workspace_bytes(n, gs.n_edges, int(gated), gs.max_in_degree)
    ws = _Workspace.get(ws_bytes, h.device)
    tiles = gs.tiles()
    check(L.msmp_mp_layer_f32(ptr(h), ptr(u), ptr(pos_x), ptr(variables), ptr(feat), ptr(gs.rowptr), ptr(gs.col), ptr(gs.tgt),
                              None if tiles is None else ctypes.byref(tiles[0]), ptr(gs.graph_ptr), n, gs.n_edges, gs.n_graphs, gs.max_in_degree, gs.max_graph_nodes, main.time_window,
                              main.n_variables,
                              ptr(main.packed()), ptr(gate.packed()) if gated else None, mode, eps, ptr(out),
                              ptr(ws), ws.numel(), current_stream()), 'msmp_mp_layer_f32')
    return out


def mp_layer(h, u, pos_x, variables, structure, main, gate=None, eps=1e-5, dense_message=None, feat=None):
    """One message-passing layer (or one gated pair) on the device through msmp_mp_layer_f32.
    h [N,128], u [N,Tw], pos_x [N,1] or [N], variables [N,nv]: float32 CUDA tensors.
    dense_message: None -> module default (factorised message_net_1); True -> literal per-edge GEMM.
    Under autograd (training) the forward is the same HIP call and the backward one msmp_mp_layer_bwd_f32 call (layer_bwd_kernel.hip): an
    explicit recompute on the library's own bf16x3 row GEMMs (rows_gemm_kernel.hip), its glue kernels and the weight-gradient kernels of
    grad_weights_kernel.hip (msmp_pde_amd.autograd)."""
    gs = structure
    if gs is None or h.device.type != 'cuda':
        raise _lib.MsmpError('mp_layer needs CUDA tensors and a GraphStructure (HIP path only, no CPU fallback)')
    need_grad = torch.is_grad_enabled() and (h.requires_grad or any(p.requires_grad for p in main._params8()))
    if main.wide:
        if need_grad:
            # msmp_tune("wide_bwd") != 0: HIP forward (saving only the layer inputs) + one msmp_wide_layer_bwd_f32 call, as at width 128;
            # float64 inputs and sizes the entry refuses by value keep the PyTorch ops
            if h.dtype == torch.float32 and main.MODE == _lib.MSMP_LAYER_LIN and lib().msmp_tune_query(b'wide_bwd'):
                from .autograd import MPLayerFunction, wide_layer_bwd_taken
                if wide_layer_bwd_taken(h.shape[0], gs.n_edges, u.shape[1], variables.shape[1], h.shape[1], gate is not None):
                    params = list(main._params8()) + (list(gate._params8()) if gate is not None else [])
                    return MPLayerFunction.apply(h.contiguous(), _f32c(u), _f32c(pos_x).reshape(-1), _f32c(variables), gs, main, gate, eps,
                                                 _mp_layer_wide, *params)
            return _mp_layer_wide_autograd(h, u.to(h.dtype), pos_x, variables.to(h.dtype), gs, main, gate, eps)
        return _mp_layer_wide(_f32c(h), _f32c(u), _f32c(pos_x).reshape(-1), _f32c(variables), gs, main, gate, eps, feat)
    hd, u, pos_x, variables = _f32c(h), _f32c(u), _f32c(pos_x).reshape(-1), _f32c(variables)
    n = hd.shape[0]
    assert n == gs.n_nodes and hd.shape[1] == HIDDEN and u.shape[1] == main.time_window
    assert variables.shape[1] == main.n_variables and pos_x.numel() == n
    if not need_grad:
        return _mp_layer_hip(hd, u, pos_x, variables, gs, main, gate, eps, dense_message, feat)

    from .autograd import MPLayerFunction
    params = list(main._params8()) + (list(gate._params8()) if gate is not None else [])
    hin = h if (h.dtype == torch.float32 and h.is_contiguous()) else h.to(torch.float32).contiguous()
    return MPLayerFunction.apply(hin, u, pos_x, variables, gs, main, gate, eps, _mp_layer_hip, *params)
