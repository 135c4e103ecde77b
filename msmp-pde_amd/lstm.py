"""The LSTM encoder of the LSTM ablation classes on the HIP kernels of lstm_train_kernel.hip: torch.nn.LSTM(ninp, nhid) (one layer,
unidirectional, no projection) as ONE launch forward and, under autograd, one BPTT launch + one msmp_grad_weights_cat_f32 call backward.
`solvers.LSTM` holds the parameters (an nn.LSTM, so names and pickles are the reference's) and chooses the route; this module is the native
route."""
import torch

from .recurrent import Cell, packed_blob, forward_launch, train_forward as _function_forward, train_backward, _padded_inputs, _state


def kernel_exists(ninp, nhid):
    """True at the sizes msmp_lstm_train_fwd_f32 / _bwd_f32 take."""
    return 1 <= ninp <= 8 and 1 <= nhid <= 256


def packed(cache, rnn):
    """The forward blob of msmp_lstm_train_fwd_f32 (bf16x3 fragments of weight_hh_l0, fp32 fragments of weight_ih_l0, b_ih + b_hh), cached in
    `cache` (a PackedCache) until a parameter changes."""
    return packed_blob(cache, [rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0], 'msmp_packed_lstm_train_floats',
                       'msmp_pack_lstm_train_f32', rnn.input_size, rnn.hidden_size)


def train_forward(blob, ninp, nhid, x, h0, c0, saved=None):
    """msmp_lstm_train_fwd_f32 with the forward blob `blob` (recurrent.forward_launch)."""
    return forward_launch('msmp_lstm_train_fwd_f32', x, ninp, nhid, (), lambda: blob, h0, c0, saved)


def _grads(rows, w, nh):
    dw, db = rows(0, range(4)), rows(1, range(4))
    return None, None, dw[:, nh:].contiguous(), dw[:, :nh].contiguous(), db, db.clone(), None, None


# saved planes i, f, g, o, c_t, h_{t-1}; dG gates i, f, g, o (torch's row order), all against [h_{t-1} | x_t]; both biases take the column sums
_CELL = Cell('msmp_lstm_saved_floats', 'msmp_packed_lstm_bwd_floats', 'msmp_pack_lstm_bwd_f32', 'msmp_lstm_train_bwd_f32', n_states=1,
             gate_planes=(5, 5, 5, 5), grads=_grads)


class _LSTMTrainFunction(torch.autograd.Function):
    """torch.nn.LSTM's output[-1] (and c_T) on the HIP training kernels at any hidden width 1..256: forward = msmp_lstm_train_fwd_f32 (saves the
    per-step activations), backward = msmp_lstm_train_bwd_f32 + the weight-gradient jobs (recurrent.py)."""

    @staticmethod
    def forward(ctx, blob, xin, w_ih, w_hh, b_ih, b_hh, h0=None, c0=None):
        ninp, nh = xin.shape[2], w_hh.shape[1]
        return _function_forward(ctx, _CELL, lambda x, h0, c0, saved: train_forward(blob, ninp, nh, x, h0, c0, saved), ninp, nh, xin, (w_hh,), h0, c0)

    backward = staticmethod(train_backward)
