"""The LSTM encoder of the LSTM ablation classes on the HIP kernels of lstm_train_kernel.hip: torch.nn.LSTM(ninp, nhid) (one layer,
unidirectional, no projection) as ONE launch forward and, under autograd, one BPTT launch + one msmp_grad_weights_cat_f32 call backward.
`solvers.LSTM` holds the parameters (an nn.LSTM, so names and pickles are the reference's) and chooses the route; this module is the native
route."""
import torch

from ._lib import lib, check, ptr, current_stream, MSMP_ERR_UNSUPPORTED
from .lem import _padded_inputs, _state


def kernel_exists(ninp, nhid):
    """True at the sizes msmp_lstm_train_fwd_f32 / _bwd_f32 take."""
    return 1 <= ninp <= 8 and 1 <= nhid <= 256


def packed(cache, rnn):
    """The forward blob of msmp_lstm_train_fwd_f32 (bf16x3 fragments of weight_hh_l0, fp32 fragments of weight_ih_l0, b_ih + b_hh), cached in
    `cache` (a PackedCache) until a parameter changes."""
    ps = [rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0]

    def build():
        L = lib()
        n_floats = L.msmp_packed_lstm_train_floats(rnn.input_size, rnn.hidden_size)
        if n_floats <= 0:
            check(MSMP_ERR_UNSUPPORTED, 'msmp_packed_lstm_train_floats')
        blob = torch.empty(n_floats, dtype=torch.float32, device=ps[0].device)
        f = [p.detach().contiguous() for p in ps]
        check(L.msmp_pack_lstm_train_f32(*[ptr(t) for t in f], rnn.input_size, rnn.hidden_size, ptr(blob), current_stream()), 'msmp_pack_lstm_train_f32')
        return blob
    return cache.get(ps, build)


def train_forward(blob, ninp, nhid, x, h0, c0, saved=None):
    """msmp_lstm_train_fwd_f32 on the padded step inputs x [N, T, stride] from the states (h0, c0) (None = zeros) -> (h_T, c_T); `saved`: the
    planes the backward reads (msmp_lstm_saved_floats), or None when no backward follows."""
    n, t_len = x.shape[0], x.shape[1]
    h = torch.empty(n, nhid, dtype=torch.float32, device=x.device)
    c = torch.empty_like(h)
    check(lib().msmp_lstm_train_fwd_f32(ptr(x), n, t_len, ninp, nhid, ptr(blob), ptr(h0), ptr(c0), ptr(saved), ptr(h), ptr(c), current_stream()),
          'msmp_lstm_train_fwd_f32')
    return h, c


class _LSTMTrainFunction(torch.autograd.Function):
    """torch.nn.LSTM's output[-1] (and c_T) on the HIP training kernels at any hidden width 1..256: forward = msmp_lstm_train_fwd_f32 (saves the
    per-step activations), backward = msmp_lstm_train_bwd_f32 (BPTT, one launch) followed by ONE msmp_grad_weights_cat_f32 call whose jobs are
    the 128-column blocks of the four gates of dG (at most 8) against [h_{t-1} | x_t].  Allocates through torch only and never synchronises
    (hipGraph capture).  No gradient for the step inputs, nor for the initial states."""

    @staticmethod
    def forward(ctx, blob, xin, w_ih, w_hh, b_ih, b_hh, h0=None, c0=None):
        x = _padded_inputs(xin)
        n, t_len, ninp = xin.shape
        nh = w_hh.shape[1]
        saved = torch.empty(lib().msmp_lstm_saved_floats(n, t_len, nh), dtype=torch.float32, device=x.device)
        h0, c0 = _state(h0), _state(c0)
        h, c = train_forward(blob, ninp, nh, x, h0, c0, saved)
        ctx.save_for_backward(x, saved, w_hh, *([c0] if c0 is not None else []))
        ctx.ninp = ninp
        ctx.mark_non_differentiable(c)
        return h, c

    @staticmethod
    def backward(ctx, grad_h, _grad_c=None):
        L = lib()
        x, saved, w_hh, *state = ctx.saved_tensors
        c0 = state[0] if state else None
        n, t_len, stride = x.shape
        nh, ninp = w_hh.shape[1], ctx.ninp
        wp, ldg, nblk = 32 * ((nh + 31) // 32), 128 * ((nh + 127) // 128), (nh + 127) // 128
        blob = torch.empty(L.msmp_packed_lstm_bwd_floats(ninp, nh), dtype=torch.float32, device=x.device)
        check(L.msmp_pack_lstm_bwd_f32(ptr(w_hh.detach().contiguous()), ninp, nh, ptr(blob), current_stream()), 'msmp_pack_lstm_bwd_f32')
        dg = torch.empty(n * t_len, 4 * ldg, dtype=torch.float32, device=x.device)      # every element is written by the kernel
        g = grad_h.to(torch.float32).contiguous()
        check(L.msmp_lstm_train_bwd_f32(ptr(g), ptr(saved), ptr(c0), n, t_len, nh, ptr(blob), ptr(dg), current_stream()), 'msmp_lstm_train_bwd_f32')
        h_prev = saved.view(6, n * t_len, wp)[5][:, :nh]        # the forward saves h_{t-1} (h0 at t = 0): the rows of [h_{t-1} | x_t]
        xs = x.view(n * t_len, stride)[:, :ninp]
        from .autograd import grad_weights          # weight / bias gradients: sums over the N*T rows; [h_{t-1} | x_t] is never materialised
        r = grad_weights([(dg[:, gate * ldg + 128 * j:gate * ldg + 128 * (j + 1)], h_prev, xs) for gate in range(4) for j in range(nblk)])

        def rows(kind):          # kind 0: weight, 1: bias blocks of the four gates, without the rows >= width of a last block (zero columns of dG)
            return torch.cat([r[2 * (nblk * gate + j) + kind][:min(128, nh - 128 * j)] for gate in range(4) for j in range(nblk)], 0)
        dw, db = rows(0), rows(1)
        return None, None, dw[:, nh:].contiguous(), dw[:, :nh].contiguous(), db, db.clone(), None, None
