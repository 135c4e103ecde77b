"""The Swish MLPs around the encoder and decoder under autograd on the HIP kernels of mlp_train_kernel.hip: forward = ONE
msmp_mlp_train_fwd_f32 launch that also saves the pre-activations, backward = ONE msmp_mlp_train_bwd_f32 call (one kernel down to dx,
then the weight gradients as msmp_grad_weights_f32 jobs issued inside the call).

  form                                              modules                                          classes
  Sequential(Linear, Swish, Linear, Swish)          embedding_mlp, lemoutput_mlp, lstmoutput_mlp     every class (encoder)
  Sequential(Linear, Swish[, Unflatten]), heads 2   double_mlp: Linear(W, 2 W)                       the *2D classes (decoder)

`swish_mlp` returns None where the kernels do not apply; the solvers then call the PyTorch module.  Switch: msmp_tune("mlp_train").
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from ._lib import lib, check, ptr, current_stream, PackedCache
from .layers import Swish


def _rows(t):
    """t [N, C] float32 as rows of unit element stride -> (t, row stride); anything else (an expanded gradient, a transposed view) is copied."""
    if t.dtype != torch.float32:
        t = t.to(torch.float32)
    if t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t, (t.stride(0) if t.shape[0] > 1 else t.shape[1])


class SwishMLPFunction(torch.autograd.Function):
    """out [N, heads W] (rows ld_out floats apart; a view of the buffer the kernel writes where ld_out > heads W) of the two-layer
    (w2, b2 given) or one-layer form.  Gradients for x (skipped, with its GEMM, where x does not require grad) and the parameters that
    require grad.  `blob`: the packed parameters (msmp_pack_mlp_train_f32).  The saved pre-activations and the workspace of the backward are
    per-call torch.empty (under a capture they come from the graph's pool); nothing synchronises."""

    @staticmethod
    def forward(ctx, x, blob, heads, ld_out, w1, b1, w2, b2):
        L = lib()
        layers = 1 if w2 is None else 2
        x, ldx = _rows(x.detach())
        n, k = x.shape
        width = w1.shape[0] // heads
        saved = torch.empty(L.msmp_mlp_train_saved_floats(n, layers, heads, width), dtype=torch.float32, device=x.device)
        buf = torch.empty(n, ld_out, dtype=torch.float32, device=x.device)
        check(L.msmp_mlp_train_fwd_f32(ptr(x), ldx, n, layers, heads, k, width, ptr(blob), ptr(saved), ptr(buf), ld_out, current_stream()),
              'msmp_mlp_train_fwd_f32')
        ctx.save_for_backward(x, saved, blob)        # the blob of THESE parameter values: the cache may hold a newer one by the backward
        ctx.dims = (layers, heads, k, width, ldx)
        return buf if ld_out == heads * width else buf[:, :heads * width]

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        L = lib()
        x, saved, blob = ctx.saved_tensors
        layers, heads, k, width, ldx = ctx.dims
        n, dev = x.shape[0], x.device
        g, ldg = _rows(grad_out)
        need = ctx.needs_input_grad
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)       # every element of every output is written by the kernels
        dx = new(n, k) if need[0] else None
        dw1, db1 = new(heads * width, k), new(heads * width)
        dw2, db2 = (new(width, width), new(width)) if layers == 2 else (None, None)
        ws = torch.empty(L.msmp_mlp_train_bwd_workspace_bytes(n, layers, heads, k, width), dtype=torch.uint8, device=dev)
        check(L.msmp_mlp_train_bwd_f32(ptr(g), ldg, ptr(x), ldx, ptr(saved), n, layers, heads, k, width, ptr(blob), ptr(dx), k, ptr(dw1), ptr(db1),
                                       ptr(dw2), ptr(db2), ptr(ws), ws.numel(), current_stream()), 'msmp_mlp_train_bwd_f32')
        dw1._msmp_keep = (g, ws)            # read by the kernels after this returns
        grads = [t if t is not None and need[4 + i] else None for i, t in enumerate((dw1, db1, dw2, db2))]
        return (dx, None, None, None, *grads)


def _form(seq, heads):
    """(linear 1, linear 2 or None, Unflatten or None) of a Sequential the kernels evaluate, else None."""
    m = list(seq)
    if len(m) < 2 or not (isinstance(m[0], nn.Linear) and isinstance(m[1], Swish) and m[1].beta == 1 and m[0].bias is not None):
        return None
    if len(m) == 4 and heads == 1 and isinstance(m[2], nn.Linear) and isinstance(m[3], Swish) and m[3].beta == 1 and m[2].bias is not None:
        return (m[0], m[2], None) if m[2].in_features == m[2].out_features == m[0].out_features else None
    if m[0].out_features % heads:
        return None
    if len(m) == 2:
        return m[0], None, None
    if len(m) == 3 and isinstance(m[2], nn.Unflatten) and m[2].dim == 1 and tuple(m[2].unflattened_size) == (heads, m[0].out_features // heads):
        return m[0], None, m[2]
    return None


def swish_mlp(seq, x, heads=1, ld_out=None):
    """seq(x) for x [N, K] through SwishMLPFunction, or None where the kernels do not apply: switch "mlp_train" 0, a Sequential of another
    form, a tensor or parameter that is not float32 on the GPU, grad disabled or nothing that requires grad, no rows, and sizes the entries
    refuse by value (remembered on the module: not asked again).  heads: the independent W-wide halves of a one-layer Linear(K, heads W);
    ld_out: the row stride of the result (default heads W: contiguous).  The packed blob is cached per parameter version (PackedCache on the
    module) and built on the CURRENT stream."""
    ok = lambda t: t.is_cuda and t.dtype == torch.float32
    if not (torch.is_tensor(x) and x.dim() == 2 and ok(x) and x.shape[0] > 0 and torch.is_grad_enabled()):
        return None
    form = _form(seq, heads)
    if form is None or getattr(seq, '_mlp_train_refused', False):
        return None
    lin1, lin2, unflatten = form
    ps = [lin1.weight, lin1.bias] + ([lin2.weight, lin2.bias] if lin2 is not None else [])
    if not all(ok(p) for p in ps) or not (x.requires_grad or any(p.requires_grad for p in ps)):
        return None
    L = lib()
    if L.msmp_tune_query(b'mlp_train') == 0:
        return None
    layers, k, width = len(ps) // 2, lin1.in_features, lin1.out_features // heads
    floats = L.msmp_packed_mlp_train_floats(layers, heads, k, width)
    if x.shape[1] != k or not floats:
        seq._mlp_train_refused = not floats
        return None

    def build():
        blob = torch.empty(floats, dtype=torch.float32, device=x.device)
        f = [p.detach().contiguous() for p in ps] + [None] * (4 - len(ps))
        check(L.msmp_pack_mlp_train_f32(*[ptr(t) for t in f], layers, heads, k, width, ptr(blob), current_stream()), 'msmp_pack_mlp_train_f32')
        return blob
    if getattr(seq, '_mlp_train_blob', None) is None:
        seq._mlp_train_blob = PackedCache()
    blob = seq._mlp_train_blob.get(ps, build)
    out = SwishMLPFunction.apply(x, blob, heads, heads * width if ld_out is None else ld_out, *ps, *([None] * (4 - len(ps))))
    return out if unflatten is None else out.unflatten(1, (heads, width))
