"""The CNN decoder of the solver classes under autograd on the HIP kernels: forward = the decoder's own one-launch kernel through its
forward-for-training entry (msmp_decoder*_train_fwd_f32, decoder_kernel.hip), backward = ONE msmp_decoder*_bwd_f32 call
(decoder_bwd_kernel.hip) that recomputes what it needs from the rows, so nothing but the inputs is saved.

  kind        rows                       networks                                       classes
  '1d'        h  [N, 128]                output_mlp                                     the 1-D classes at width 128 (u None: RETURN_DIFF)
  '2d'        hd [N, 2, 128]             output_mlp                                     the *2D classes at width 128
  'gated'     h  [N, 164]                output_mlp_gate, output_mlp_diff               MSGMP-PDE
  'gated2d'   hd [N, 2, 164]             output_mlp_gate, output_mlp_diff               MSGMP-PDE2D
(hd = double_mlp(h): mlp.swish_mlp, or the PyTorch module.)  `decode` returns None where the entries refuse the sizes by value; the solvers then
keep their PyTorch ops (solvers._decode).  Switch: msmp_tune("dec_bwd").
"""
import torch
from torch.autograd.function import once_differentiable

from ._lib import lib, check, ptr, current_stream

_ENTRIES = {'1d': ('msmp_decoder_train_fwd_f32', 'msmp_decoder_bwd_f32', 1, 0),
            '2d': ('msmp_decoder2d_train_fwd_f32', 'msmp_decoder2d_bwd_f32', 2, 0),
            'gated': ('msmp_decoder_gated_train_fwd_f32', 'msmp_decoder_gated_bwd_f32', 1, 1),
            'gated2d': ('msmp_decoder2d_gated_train_fwd_f32', 'msmp_decoder2d_gated_bwd_f32', 2, 1)}


def supported(kind, width, tw):
    """Whether the backward entry of `kind` exists for this width and time window (its size query: by value, nothing launched)."""
    _, _, comps, gated = _ENTRIES[kind]
    return lib().msmp_decoder_bwd_workspace_bytes(comps, gated, width, tw) > 0


def _f32(ts):
    return [t.detach().to(torch.float32).contiguous() for t in ts]


class DecoderFunction(torch.autograd.Function):
    """out [N, comps tw] = decoder(rows, u) with the weights of one network (w1, b1, w2, b2) or of the gated pair (gate's four, then diff's).
    Gradients for the rows and the weights; none for u, dt.  The workspace of the backward is a per-call torch.empty (under a capture it
    comes from the graph's pool); nothing is cached and nothing synchronises."""

    @staticmethod
    def forward(ctx, kind, rows, u, tw, dt, *weights):
        fwd, _, comps, gated = _ENTRIES[kind]
        L = lib()
        rows = rows.detach()
        n, width = rows.shape[0], rows.shape[-1]
        ld = comps * width
        if gated and rows.dim() == 3 and n > 1 and rows.stride()[1:] == (width, 1) and rows.stride(0) >= ld:
            ld = rows.stride(0)         # the rows of mlp.swish_mlp, written at the stride of the width-generic path: read in place
        else:
            rows = rows.contiguous()
        w = _f32(weights)
        u = None if u is None else u.detach().contiguous()
        out = torch.empty(n, comps * tw, dtype=torch.float32, device=rows.device)
        if gated:
            check(getattr(L, fwd)(ptr(rows), ld, ptr(u), n, width, tw, *[ptr(t) for t in w], float(dt), ptr(out), current_stream()), fwd)
        else:
            check(getattr(L, fwd)(ptr(rows), ptr(u), n, tw, *[ptr(t) for t in w], float(dt), ptr(out), current_stream()), fwd)
        ctx.save_for_backward(rows, *([u] if u is not None else []), *w)      # the weights stay alive until the backward has been issued
        ctx.kind, ctx.tw, ctx.dt, ctx.has_u, ctx.ld = kind, tw, float(dt), u is not None, ld
        ctx.dtypes = [p.dtype for p in weights]
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        _, bwd, comps, gated = _ENTRIES[ctx.kind]
        L = lib()
        rows, *rest = ctx.saved_tensors
        u, w = (rest[0], rest[1:]) if ctx.has_u else (None, rest)
        n, width, tw = rows.shape[0], rows.shape[-1], ctx.tw
        g = grad_out.to(torch.float32).contiguous()
        dh = torch.empty(rows.shape, dtype=rows.dtype, device=rows.device)      # compact; every element of every output is written by the kernels
        grads = [torch.empty_like(t) for t in w]
        ws = torch.empty(L.msmp_decoder_bwd_workspace_bytes(comps, gated, width, tw), dtype=torch.uint8, device=rows.device)
        tail = [ptr(dh)] + [ptr(t) for t in grads] + [ptr(ws), ws.numel(), current_stream()]
        if gated:
            rc = getattr(L, bwd)(ptr(g), ptr(rows), ctx.ld, ptr(u), n, width, tw, *[ptr(t) for t in w], ctx.dt, *tail)
        elif comps == 2:
            rc = getattr(L, bwd)(ptr(g), ptr(rows), n, tw, *[ptr(t) for t in w], ctx.dt, *tail)
        else:
            rc = getattr(L, bwd)(ptr(g), ptr(rows), n, tw, int(ctx.has_u), *[ptr(t) for t in w], ctx.dt, *tail)
        check(rc, bwd)
        dh._msmp_keep = (g, ws, w)          # read by the kernels after this returns
        need = ctx.needs_input_grad
        wg = [t.to(d) if need[5 + i] else None for i, (t, d) in enumerate(zip(grads, ctx.dtypes))]
        return (None, dh if need[1] else None, None, None, None, *wg)


def _params(net):
    return (net[0].weight, net[0].bias, net[2].weight, net[2].bias)


def decode(kind, rows, u, tw, dt, *nets):
    """The decoder of `kind` on float32 CUDA rows through DecoderFunction; nets: the Conv1d -> Swish -> Conv1d modules (one, or gate and
    diff).  None where the entries do not exist for the sizes."""
    if not supported(kind, rows.shape[-1], tw):
        return None
    return DecoderFunction.apply(kind, rows, u, tw, dt, *[p for net in nets for p in _params(net)])
