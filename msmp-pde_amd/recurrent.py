"""The host side of the recurrent training kernel pairs (csrc/recurrent_train.h): what the LEM's and the LSTM's blobs and autograd Functions
(`lem._LEMTrainFunction`, `lstm._LSTMTrainFunction`) share.  Allocates through torch only and never synchronises (hipGraph capture).  No gradient
for the step inputs, nor for the initial states.  What differs between the cells is a `Cell` record."""
import collections

import torch

from ._lib import lib, check, ptr, current_stream, MSMP_ERR_UNSUPPORTED

# saved_floats, bwd_floats, pack_bwd, bwd: entry names;  n_states: how many of the initial states (h0, c0) the BPTT entry takes, counted from the end;
# gate_planes: for each gate of dG, the plane of `saved` whose rows its weight gradient multiplies (the state that entered the gate's product);
# grads(rows, weights, nhid): the gradients in the order of the Function's arguments, from rows(kind 0 weight / 1 bias, gates) = those rows of dW / db
Cell = collections.namedtuple('Cell', 'saved_floats bwd_floats pack_bwd bwd n_states gate_planes grads')


def packed_blob(cache, ps, size_entry, pack_entry, ninp, nhid):
    """A blob of the parameters `ps`, `size_entry(ninp, nhid)` floats written by `pack_entry`, cached in `cache` (a PackedCache) until one changes."""
    def build():
        L = lib()
        n_floats = getattr(L, size_entry)(ninp, nhid)
        if n_floats <= 0:
            check(MSMP_ERR_UNSUPPORTED, size_entry)
        blob = torch.empty(n_floats, dtype=torch.float32, device=ps[0].device)
        f = [p.detach().to(torch.float32).contiguous() for p in ps]
        check(getattr(L, pack_entry)(*[ptr(t) for t in f], ninp, nhid, ptr(blob), current_stream()), pack_entry)
        return blob
    return cache.get(ps, build)


def _padded_inputs(xin):
    """xin [N, T, ninp] -> float32, rows zero-padded to msmp_lem_input_stride(ninp), contiguous."""
    ninp = xin.shape[2]
    stride = lib().msmp_lem_input_stride(ninp)
    x = xin.detach().to(torch.float32)
    return (torch.nn.functional.pad(x, (0, stride - ninp)) if stride != ninp else x).contiguous()


def _state(t):
    return None if t is None else t.detach().to(torch.float32).contiguous()


def forward_launch(entry, x, ninp, nhid, scalars, blob, h0, c0, saved):
    """`entry`, a cell's forward entry, on the padded step inputs x [N, T, stride] from the states (h0, c0) (None = zeros) -> (h_T, c_T); `saved`: the
    planes the backward reads, or None when no backward follows; blob(): the forward blob, asked for once the outputs are allocated."""
    n, t_len = x.shape[0], x.shape[1]
    h = torch.empty(n, nhid, dtype=torch.float32, device=x.device)
    c = torch.empty_like(h)
    check(getattr(lib(), entry)(ptr(x), n, t_len, ninp, nhid, *scalars, ptr(blob()), ptr(h0), ptr(c0), ptr(saved), ptr(h), ptr(c), current_stream()), entry)
    return h, c


def train_forward(ctx, cell, launch, ninp, nhid, xin, weights, h0, c0, scalars=()):
    """The forward of a Function: launch(x, h0, c0, saved) -> (h_T, c_T) is the cell's forward entry on the padded inputs; `weights`: the parameters
    that hold the recurrent blocks, in the order of the cell's pack entry; `scalars`: the scalar arguments of its BPTT entry (the LEM's dt)."""
    x = _padded_inputs(xin)
    n, t_len, _ = xin.shape
    saved = torch.empty(getattr(lib(), cell.saved_floats)(n, t_len, nhid), dtype=torch.float32, device=x.device)
    h0, c0 = _state(h0), _state(c0)
    h, c = launch(x, h0, c0, saved)
    ctx.save_for_backward(x, saved, *weights, *((h0, c0)[-cell.n_states:] if c0 is not None else ()))
    ctx.cell, ctx.ninp, ctx.nhid, ctx.scalars, ctx.n_weights = cell, ninp, nhid, scalars, len(weights)
    ctx.mark_non_differentiable(c)          # the carried state: a constant for the next call (models_gnn.py:350-353)
    return h, c


def train_backward(ctx, grad_h, _grad_c=None):
    """The backward of a Function (c_T is not differentiable): the transposed blob packed, the cell's BPTT launch (dL/dh_T -> dG, the pre-activation gradients of the four gates per node and step) and ONE
    msmp_grad_weights_cat_f32 call whose jobs are the 128-column blocks of the four gates of dG (at most 8) against [saved state | x_t]."""
    L, cell = lib(), ctx.cell
    x, saved, *rest = ctx.saved_tensors
    weights, states = rest[:ctx.n_weights], rest[ctx.n_weights:] or [None] * cell.n_states
    n, t_len, stride = x.shape
    nh, ninp = ctx.nhid, ctx.ninp
    wp, ldg, nblk = 32 * ((nh + 31) // 32), 128 * ((nh + 127) // 128), (nh + 127) // 128
    blob = torch.empty(getattr(L, cell.bwd_floats)(ninp, nh), dtype=torch.float32, device=x.device)
    w = [p.detach().to(torch.float32).contiguous() for p in weights]
    check(getattr(L, cell.pack_bwd)(*[ptr(t) for t in w], ninp, nh, ptr(blob), current_stream()), cell.pack_bwd)
    dg = torch.empty(n * t_len, 4 * ldg, dtype=torch.float32, device=x.device)      # every element is written by the kernel
    g = grad_h.to(torch.float32).contiguous()
    check(getattr(L, cell.bwd)(ptr(g), ptr(saved), *[ptr(s) for s in states], n, t_len, nh, *ctx.scalars, ptr(blob), ptr(dg), current_stream()), cell.bwd)
    planes = saved.view(6, n * t_len, wp)       # node-major: each plane is directly the row matrix of a weight-gradient GEMM
    xs = x.view(n * t_len, stride)[:, :ninp]
    from .autograd import grad_weights          # weight / bias gradients: sums over the N*T rows; [state | x_t] is never materialised
    r = grad_weights([(dg[:, gate * ldg + 128 * j:gate * ldg + 128 * (j + 1)], planes[cell.gate_planes[gate]][:, :nh], xs)
                      for gate in range(4) for j in range(nblk)])

    def rows(kind, gates):          # without the rows >= width of a last block (zero columns of dG)
        blocks = [r[2 * (nblk * gate + j) + kind][:min(128, nh - 128 * j)] for gate in gates for j in range(nblk)]
        return blocks[0] if len(blocks) == 1 else torch.cat(blocks, 0)
    return cell.grads(rows, weights, nh)
