"""The gradient gate (G2) of MP_PDE_Solver2DLEMLinG2 between the two layer calls of a pair (experiments/models_gnn2D.py:598-611):

    t = Swish(a);   tau_i = tanh(mean over the out-edges i -> j of (t_i - t_j)^2);   out = (1 - tau) h + tau Swish(b)

with a the gate layer's output and b the main layer's.  `g2_gate_blend` is the one place where the route is chosen: one
msmp_g2_gate_blend_f32 launch (g2_gate_kernel.hip; under autograd with tau saved and msmp_g2_gate_blend_bwd_f32 as the backward), or the
PyTorch-ROCm ops around msmp_scatter_mean_f32 that the class used before the kernels existed."""
import torch

from ._lib import lib, check, ptr, current_stream
from .layers import Swish

_swish = Swish()


class _OutEdgeMean(torch.autograd.Function):
    """Mean of a per-edge tensor [E,128] over each node's OUT-edges (torch_scatter `scatter(..., edge_index[0], reduce='mean')`,
    models_gnn2D.py:607-608) in a fixed summation order: edges regrouped by source once per graph structure, then
    msmp_scatter_mean_f32.  Nodes without out-edges get 0."""

    @staticmethod
    def forward(ctx, msg, gs):
        perm, rowptr = gs.by_source()
        m = msg.detach().to(torch.float32)[perm].contiguous()
        out = torch.empty(gs.n_nodes, m.shape[1], dtype=torch.float32, device=m.device)
        check(lib().msmp_scatter_mean_f32(ptr(m), ptr(rowptr), gs.n_nodes, ptr(out), current_stream()), 'msmp_scatter_mean_f32')
        ctx.gs = gs
        return out

    @staticmethod
    def backward(ctx, g):
        perm, rowptr = ctx.gs.by_source()
        deg = (rowptr[1:] - rowptr[:-1]).clamp(min=1).to(g.dtype)
        return (g / deg[:, None])[ctx.gs.col_long], None


def kernel_exists(width):
    """True at the widths msmp_g2_gate_blend_f32 / _bwd_f32 take."""
    return 4 <= width <= 256 and width % 4 == 0


def gate_blend_forward(h, a, b, gs, save_tau):
    """msmp_g2_gate_blend_f32 on contiguous fp32 rows h, a, b [N, W] -> (out, tau or None)."""
    n, w = h.shape
    out_rowptr, out_nbr = gs.out_edges32()
    out = torch.empty_like(h)
    tau = torch.empty_like(h) if save_tau else None
    check(lib().msmp_g2_gate_blend_f32(ptr(h), ptr(a), ptr(b), w, ptr(out_rowptr), ptr(out_nbr), n, gs.n_edges, w, ptr(out), ptr(tau),
                                       current_stream()), 'msmp_g2_gate_blend_f32')
    return out, tau


class _G2GateBlend(torch.autograd.Function):
    """The gate statistic, tanh and blend as one launch, saving h, a, b and tau; backward = one msmp_g2_gate_blend_bwd_f32 call (gathers over
    the out- and in-edge lists in a fixed order: no atomics, no memset, no read-back).  Allocates through torch only (hipGraph capture)."""

    @staticmethod
    def forward(ctx, h, a, b, gs):
        out, tau = gate_blend_forward(h, a, b, gs, True)
        ctx.save_for_backward(h, a, b, tau)
        ctx.gs = gs
        return out

    @staticmethod
    def backward(ctx, g):
        L = lib()
        h, a, b, tau = ctx.saved_tensors
        gs = ctx.gs
        n, w = h.shape
        out_rowptr, out_nbr = gs.out_edges32()
        g = g.to(torch.float32).contiguous()
        dh, da, db = torch.empty_like(h), torch.empty_like(h), torch.empty_like(h)      # every element is written by the kernels
        ws = torch.empty(L.msmp_g2_gate_blend_bwd_workspace_bytes(n, w), dtype=torch.uint8, device=h.device)
        check(L.msmp_g2_gate_blend_bwd_f32(ptr(g), ptr(h), ptr(a), ptr(b), ptr(tau), w, ptr(out_rowptr), ptr(out_nbr), ptr(gs.rowptr), ptr(gs.col),
                                           n, gs.n_edges, w, ptr(dh), ptr(da), ptr(db), ptr(ws), ws.numel(), current_stream()),
              'msmp_g2_gate_blend_bwd_f32')
        return dh, da, db, None


def g2_gate_blend(h, a, b, gs):
    """(1 - tau) h + tau Swish(b) with tau the gradient gate of t = Swish(a) over the graph `gs`.  The one place where the route is chosen:

        h, a, b CUDA float32 [N, W], W a multiple of 4 in 4 .. 256, msmp_tune "g2_gate" != 0:
            grad enabled and one of them requires grad     _G2GateBlend (msmp_g2_gate_blend_f32 with tau saved, msmp_g2_gate_blend_bwd_f32)
            otherwise                                      msmp_g2_gate_blend_f32 with tau_out = NULL: one launch, the same bits
        everything else (CPU, float64, switch 0, other widths)
            the PyTorch ops around _OutEdgeMean, exactly as before the kernels existed
    """
    rows = (h, a, b)
    if (all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape == h.shape for t in rows) and h.shape[0] > 0
            and kernel_exists(h.shape[1]) and lib().msmp_tune_query(b'g2_gate') != 0):
        h, a, b = (t.contiguous() for t in rows)
        if torch.is_grad_enabled() and any(t.requires_grad for t in rows):
            return _G2GateBlend.apply(h, a, b, gs)
        return gate_blend_forward(h, a, b, gs, False)[0]
    t = _swish(a)
    tau = torch.tanh(_OutEdgeMean.apply((t[gs.col_long] - t[gs.tgt_long]) ** 2, gs))
    return (1.0 - tau) * h + tau * _swish(b)
