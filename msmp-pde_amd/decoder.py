"""Everything after the last message-passing layer: the CNN decoder of the solver classes with its Euler update, `double_mlp` of the *2D
classes in front of it, and `decode_state`, the one place where a class's decode route is chosen (its docstring has the route table).

  kind        rows                       networks                                       classes
  '1d'        h  [N, 128]                output_mlp                                     the 1-D classes at width 128 (u None: RETURN_DIFF)
  '2d'        hd [N, 2, 128]             output_mlp                                     the *2D classes at width 128
  'gated'     h  [N, 164]                output_mlp_gate, output_mlp_diff               MSGMP-PDE
  'gated2d'   hd [N, 2, 164]             output_mlp_gate, output_mlp_diff               MSGMP-PDE2D
(hd = double_mlp(h).)  Every network is `cnn(...)`: Conv1d -> Swish -> Conv1d, the convolutions as Toeplitz GEMMs (_Conv1dNoMIOpen).

Without grad the decoder is one launch of decoder_kernel.hip.  Under autograd it is DecoderFunction: forward = the same kernel through its
forward-for-training entry, backward = ONE msmp_decoder*_bwd_f32 call (decoder_bwd_kernel.hip) that recomputes what it needs from the
rows, so nothing but the inputs is saved.  The PyTorch formulas of the reference are the one fallback (`_formula`).
Switches: msmp_tune("dec_bwd") for the training pair, msmp_tune("wide_dec") for the gated launch without grad.
"""
import torch
from torch import nn
from torch.autograd.function import once_differentiable

from ._lib import lib, check, ptr, current_stream, _Workspace
from .layers import Swish
from .reductions import bias_add
from .wide import _wide_fused, _wide_linear, _padded_rows, _entry_taken, row_stride

_DECODER = {20: (15, 4, 10), 25: (16, 3, 14), 50: (12, 2, 10)}   # time window -> (k1, stride1, k2): models_gnn.py:210-224; models_gnn2D.py:79-88
_DECODER_GLU = (6, 2, 15)       # each network of the gated pair, on half of the 164 features: models_gnn.py:1455-1456; models_gnn2D.py:1291-1298

#           inference entry             forward for training                  backward                        comps  gated
_ENTRIES = {'1d': ('msmp_decoder_f32', 'msmp_decoder_train_fwd_f32', 'msmp_decoder_bwd_f32', 1, 0),
            '2d': ('msmp_decoder2d_f32', 'msmp_decoder2d_train_fwd_f32', 'msmp_decoder2d_bwd_f32', 2, 0),
            'gated': ('msmp_decoder_gated_f32', 'msmp_decoder_gated_train_fwd_f32', 'msmp_decoder_gated_bwd_f32', 1, 1),
            'gated2d': ('msmp_decoder2d_gated_f32', 'msmp_decoder2d_gated_train_fwd_f32', 'msmp_decoder2d_gated_bwd_f32', 2, 1)}

_TOEPLITZ = {}


def _conv1d_as_matmul(x, weight, bias, stride):
    """Conv1d(x [N, Cin, Lin]; weight [Cout, Cin, k], stride) as ONE dense GEMM [N, Cin Lin] x T [Cin Lin, Cout Lout], T the
    convolution's Toeplitz matrix, itself the weight times a fixed 0/1 shift tensor (differentiable both ways as small GEMMs).
    The decoder's convolutions have 1-2 input and 8 output channels: as unfold + einsum they are [N L, 16] x [16, 8] products for
    which the library picked a 32x16-tile kernel (3.7 ms of a 48-ms training iteration at batch 512, plus the unfold backward);
    as Toeplitz products they are [N,128] x [128,304] and [N,304] x [304,25]: well-shaped GEMMs forward and backward."""
    cout, cin, k = weight.shape
    n, _, lin = x.shape
    lout = (lin - k) // stride + 1
    key = (k, lin, stride, x.device, weight.dtype)
    if key not in _TOEPLITZ:
        # E[tap, i, l] = 1 where input position i feeds output position l through that tap (i = stride l + tap): T = w . E is a
        # [Cout Cin, k] x [k, Lin Lout] product forward and backward (a gather's backward would be a sorted index_put, a dense
        # selection matrix over all of T's entries a 20-MB GEMV per call)
        i = torch.arange(lin, device=x.device)[None, :, None]
        l = torch.arange(lout, device=x.device)[None, None, :]
        tap = torch.arange(k, device=x.device)[:, None, None]
        _TOEPLITZ[key] = (i == stride * l + tap).to(weight.dtype).reshape(k, lin * lout)
    t = (weight.reshape(cout * cin, k) @ _TOEPLITZ[key]).view(cout, cin, lin, lout).permute(1, 2, 0, 3).reshape(cin * lin, cout * lout)
    out = x.reshape(n, cin * lin) @ t
    return bias_add(out, bias, lout).view(n, cout, lout)


class _Conv1dNoMIOpen(nn.Conv1d):
    """nn.Conv1d (same parameters and state_dict keys: `weight`, `bias`) whose forward is a Toeplitz GEMM.  Under autograd the
    library path of these decoder shapes ([N, C, 128], kernel 16 / stride 3 and [N, 8, 38], kernel 14) reaches MIOpen's
    implicit-GEMM backward-data kernel, which faulted on MI355X (igemm_bwd_gtcx35_nhwc_fp32, round 1); `model.output_mlp(x)`
    called the reference's way therefore never dispatches a MIOpen convolution, forward or backward."""

    def forward(self, x):
        return _conv1d_as_matmul(x, self.weight, self.bias, self.stride[0])


def cnn(comps, k1, s1, k2):
    """One decoder network on `comps` components: Conv1d(comps, 8, k1, stride s1) -> Swish -> Conv1d(8, comps, k2)."""
    return nn.Sequential(_Conv1dNoMIOpen(comps, 8, k1, stride=s1, dtype=torch.float32), Swish(),
                         _Conv1dNoMIOpen(8, comps, k2, stride=1, dtype=torch.float32))


def supported(kind, width, tw):
    """Whether the backward entry of `kind` exists for this width and time window (its size query: by value, nothing launched)."""
    comps, gated = _ENTRIES[kind][3:]
    return lib().msmp_decoder_bwd_workspace_bytes(comps, gated, width, tw) > 0


def _f32(ts):
    """The tensors as the kernels read them: detached, float32, contiguous.  A kernel reads them after the Python call has returned, so
    the caller hangs them on its result (`result._msmp_keep = ...`)."""
    return [t.detach().to(torch.float32).contiguous() for t in ts]


def _params(*nets):
    return [p for net in nets for p in (net[0].weight, net[0].bias, net[2].weight, net[2].bias)]


class DecoderFunction(torch.autograd.Function):
    """out [N, comps tw] = decoder(rows, u) with the weights of one network (w1, b1, w2, b2) or of the gated pair (gate's four, then diff's).
    Gradients for the rows and the weights; none for u, dt.  The workspace of the backward is a per-call torch.empty (under a capture it
    comes from the graph's pool); nothing is cached and nothing synchronises."""

    @staticmethod
    def forward(ctx, kind, rows, u, tw, dt, *weights):
        _, fwd, _, comps, gated = _ENTRIES[kind]
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
        _, _, bwd, comps, gated = _ENTRIES[ctx.kind]
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


def _double_mlp_128(lin, h):
    """double_mlp of the plain *2D classes without grad (models_gnn2D.py:66-70: Linear(128, 256) + Swish + Unflatten) as one HIP row GEMM
    with the bias and the Swish in its epilogue (msmp_linear_swish_f32); returns [N, 2, 128]."""
    w = _f32((lin.weight, lin.bias))
    h = h.contiguous()
    n_out, k = w[0].shape
    need = lib().msmp_linear_swish_workspace_bytes(k, n_out)
    if not need:
        raise RuntimeError(f'double_mlp of {k} -> {n_out} features is outside msmp_linear_swish_f32')
    ws = _Workspace.get(need, h.device)         # per (device, stream); the layers are done with it by now
    out = torch.empty(h.shape[0], 2, n_out // 2, dtype=torch.float32, device=h.device)
    check(lib().msmp_linear_swish_f32(ptr(h), h.shape[0], k, ptr(w[0]), ptr(w[1]), n_out, ptr(out), ptr(ws), ws.numel(), current_stream()),
          'msmp_linear_swish_f32')
    out._msmp_keep = w
    return out


def double_mlp(lin, h):
    """double_mlp of the 2-D GLU class without grad (models_gnn2D.py:1279-1283: Linear(W, 2 W) + Swish; the Unflatten is a view) at a
    width other than 128 as one msmp_linear_f32 call with the bias + Swish epilogue (mode 1).  Returns (hd, ld): node n's component c is
    hd[n, c W : (c + 1) W], rows ld = row_stride(2 W) floats apart -- the buffer the row GEMM writes, which the decoder reads in place.
    (None, ld) at a width outside msmp_linear_f32."""
    n, W = h.shape
    ld = row_stride(2 * W)
    need = lib().msmp_linear_workspace_bytes(W, 2 * W)
    if not need:
        return None, ld
    w = _f32((lin.weight, lin.bias))
    ws = _Workspace.get(need, h.device)
    hd = torch.empty(n, ld, dtype=torch.float32, device=h.device)
    _wide_linear(_padded_rows(h), W, w[0], w[1], 2 * W, 1, hd, ws)
    hd._msmp_keep = w
    return hd, ld


def _infer_plain(model, kind, h, u, tw, nets):
    """The decoder of the plain kinds as one launch, conv -> Swish -> conv -> u + cumsum(dt) * diff (2-D: behind double_mlp as one row
    GEMM); RETURN_DIFF passes no u and gets diff."""
    name = _ENTRIES[kind][0]
    rows = _double_mlp_128(model.double_mlp[0], h) if model.TWO_D else h.contiguous()
    w = _f32(_params(*nets))
    out = torch.empty_like(u)
    check(getattr(lib(), name)(ptr(rows), None if model.RETURN_DIFF else ptr(u), u.shape[0], tw, *[ptr(t) for t in w], float(model.pde.dt),
                               ptr(out), current_stream()), name)
    out._msmp_keep = (rows, w)
    return out


def _infer_gated(model, kind, h, u, tw, nets):
    """The gated pair with its Euler update as ONE launch on the rows of h (2-D: on those of double_mlp, one row GEMM, read in place);
    None where an entry refuses the sizes by value (a width or time window other than the reference's 164 / 25)."""
    name = _ENTRIES[kind][0]
    W = h.shape[1]
    h, u = h.contiguous(), u.contiguous()
    rows, ld = double_mlp(model.double_mlp[0], h) if model.TWO_D else (h, W)
    if rows is None:
        return None
    w = _f32(_params(*nets))
    out = torch.empty_like(u)
    rc = getattr(lib(), name)(ptr(rows), ld, ptr(u), u.shape[0], W, tw, *[ptr(t) for t in w], float(model.pde.dt), ptr(out), current_stream())
    if not _entry_taken(name, rc):
        return None
    out._msmp_keep = (rows, w)
    return out


def _train(model, kind, h, u, tw, nets):
    """DecoderFunction on h (2-D: on double_mlp through model._mlp, for 'gated2d' straight into rows of the stride the width-generic path
    gives them, read in place); None where the entries do not exist for the sizes."""
    rows = model._mlp(model.double_mlp, h, 2, row_stride(2 * h.shape[1]) if kind == 'gated2d' else None) if model.TWO_D else h
    if not supported(kind, h.shape[1], tw):
        return None
    return DecoderFunction.apply(kind, rows, None if model.RETURN_DIFF else u, tw, model.pde.dt, *_params(*nets))


def _formula(model, kind, h, u, dt, tw):
    """The reference's decoder as PyTorch ops, differentiable by torch.autograd (the convolutions are Toeplitz GEMMs: _Conv1dNoMIOpen)."""
    if kind == '1d':            # models_gnn.py:275-279
        diff = model.output_mlp(h[:, None]).squeeze(1)
        return diff if model.RETURN_DIFF else u[:, -1:] + dt.view(1, tw) * diff
    if kind == '2d':            # models_gnn2D.py:125-141
        diff = model.output_mlp(model._mlp(model.double_mlp, h, 2))
        return (u.view(-1, 2, tw) + dt.view(1, 1, tw) * diff).flatten(1, 2)
    if kind == 'gated':         # models_gnn.py:1511-1521
        half = h.shape[1] // 2
        scale = model.output_mlp_gate(h[:, :half][:, None]).squeeze(1)
        diff = model.output_mlp_diff(h[:, half:][:, None]).squeeze(1)
        return (1.0 - scale) * u[:, -1:] + dt.view(1, tw) * (scale * diff)
    hd = model._mlp(model.double_mlp, h, 2)         # models_gnn2D.py:1349-1366; hd [N, 2, W]
    half = hd.shape[2] // 2
    diff = model.output_mlp_diff(hd[:, :, half:])
    scale = model.output_mlp_gate(hd[:, :, :half])
    return ((1.0 - scale) * u.view(-1, 2, tw) + dt.view(1, 1, tw) * scale * diff).flatten(1, 2)


def decode_state(model, h, u, u_in, dt, tw):
    """h [N, W] after the last layer, u [N, comps tw] float32, dt = cumsum(pde.dt) [tw] -> the class's prediction [N, comps tw] in the dtype
    of u_in.  The one place where a solver class chooses its decode route.  kind: '2d' / 'gated2d' where model.TWO_D, gated where the
    model has output_mlp_gate.  With "grad path" = grad enabled and (h or a parameter of the decoder networks -- gated 2-D: or of
    double_mlp -- requires grad), and "native" = h and u float32 on the GPU:

                                         plain kinds ('1d', '2d')                          gated kinds ('gated', 'gated2d')
        no grad path                     the inference entry, no switch consulted;        native, _wide_fused("wide_dec"), sizes not refused:
                                         double_mlp: msmp_linear_swish_f32                the ONE gated launch; double_mlp: msmp_linear_f32
                                                                                          mode 1 into stride-384 rows read in place.
                                                                                          Else the formula
        grad path, native,               msmp_tune "dec_bwd" != 0, sizes not refused:     _wide_fused("dec_bwd"), sizes not refused:
        u does not require grad          DecoderFunction; double_mlp: mlp.swish_mlp       DecoderFunction; double_mlp: mlp.swish_mlp, for
                                         (model._mlp).  Else the formula                  'gated2d' at ld_out = row_stride(2 W).  Else the formula
        anything else                    the formula                                      the formula

    The formula is `_formula`: PyTorch ops, double_mlp through model._mlp.  RETURN_DIFF (MSSMP-PDE's sub-networks, '1d') gives the
    kernels no u and returns diff.  Sizes an entry refused by value are remembered on the model under the switch that led to the entry
    (`_dec_refused`), and not asked again: in 2-D each try costs a row GEMM."""
    gated = hasattr(model, 'output_mlp_gate')
    kind = ('gated2d' if model.TWO_D else 'gated') if gated else ('2d' if model.TWO_D else '1d')
    nets = (model.output_mlp_gate, model.output_mlp_diff) if gated else (model.output_mlp,)
    mods = nets + ((model.double_mlp,) if gated and model.TWO_D else ())
    grad_path = torch.is_grad_enabled() and (h.requires_grad or any(p.requires_grad for m in mods for p in m.parameters()))
    native = h.is_cuda and h.dtype == torch.float32 and u.is_cuda and u.dtype == torch.float32
    out = None
    if not (grad_path or gated):
        out = _infer_plain(model, kind, h, u, tw, nets)
    elif native and not (grad_path and u.requires_grad):
        switch = b'dec_bwd' if grad_path else b'wide_dec'
        asked = (switch, h.shape[1], tw)
        refused = model.__dict__.setdefault('_dec_refused', set())
        if asked not in refused and (_wide_fused(switch) if gated else lib().msmp_tune_query(switch)):
            out = (_train if grad_path else _infer_gated)(model, kind, h, u, tw, nets)
            if out is None:
                refused.add(asked)
    if out is None:
        out = _formula(model, kind, h, u, dt, tw)
    return out.to(u_in.dtype)
