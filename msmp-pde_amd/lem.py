"""LEM ("Long Expressive Memory") node encoder in PyTorch-ROCm.

The reference reaches an absent CUDA extension here (`import lem_cuda`, experiments/models_gnn.py:8,
285-342); BASELINE.json's north_star keeps the encoder in PyTorch, so this is a pure-torch
restatement of the recurrence with the reference's parameter names (`rnn.weights` [3H, ninp+H],
`rnn.weights_lin_z` [H, ninp+H], `rnn.bias` [3H], `rnn.bias_lin_z` [H]) and init
U(-1/sqrt(H), 1/sqrt(H)) (:318-321), dt = 1 (:334).  PARITY UNPINNED: the column order inside
lem_cuda cannot be confirmed offline; it follows the published LEM cell:
    X = [y, x_t]; g = X W^T + b -> (g1, g2, g3); dt_bar = dt s(g1); dt_ = dt s(g2)
    z <- (1-dt_) z + dt_ tanh(g3);  y <- (1-dt_bar) y + dt_bar tanh([z, x_t] Wz^T + bz)
"""
import math

import torch
from torch import nn

from ._lib import lib, check, ptr, current_stream, MSMP_ERR_UNSUPPORTED, PackedCache
from .recurrent import Cell, packed_blob, forward_launch, train_forward, train_backward, _padded_inputs, _state


class LEMcuda(nn.Module):
    """Parameter holder named like the reference's (experiments/models_gnn.py:305-330)."""

    def __init__(self, ninp, nhid, dt):
        super().__init__()
        self.ninp, self.nhid, self.dt = ninp, nhid, float(dt)
        self.weights = nn.Parameter(torch.empty(3 * nhid, ninp + nhid, dtype=torch.float32))
        self.weights_lin_z = nn.Parameter(torch.empty(nhid, ninp + nhid, dtype=torch.float32))
        self.bias = nn.Parameter(torch.empty(3 * nhid, dtype=torch.float32))
        self.bias_lin_z = nn.Parameter(torch.empty(nhid, dtype=torch.float32))
        self._wide_blob = PackedCache()
        self._wide_train_blob = PackedCache()
        self.reset_parameters()

    def _pack(self, cache, size_entry, pack_entry):
        """A blob of the four parameters, cached like LEM._pack (PackedCache)."""
        return packed_blob(cache, [self.weights, self.weights_lin_z, self.bias, self.bias_lin_z], size_entry, pack_entry, self.ninp, self.nhid)

    def _pack_wide(self):
        """The blob of msmp_lem_encoder_wide_f32 (fp16-split fragments)."""
        return self._pack(self._wide_blob, 'msmp_packed_lem_wide_floats', 'msmp_pack_lem_wide_f32')

    def _pack_wide_train(self):
        """The forward blob of msmp_lem_train_fwd_wide_f32 (bf16x3 fragments)."""
        return self._pack(self._wide_train_blob, 'msmp_packed_lem_wide_train_floats', 'msmp_pack_lem_wide_train_f32')

    def wide_kernel_exists(self):
        """True at the sizes msmp_lem_encoder_wide_f32 and the training pair take."""
        return 1 <= self.ninp <= 8 and 1 <= self.nhid <= 256

    def wide_kernel_selected(self):
        """True where a no-grad fp32 CUDA forward is ONE msmp_lem_encoder_wide_f32 launch: msmp_tune "lem_wide" and "split" both on
        (the exact-fp32 path, `_lib.exact_fp32()`, keeps the GEMM + pointwise loop: Solver.range_policy falls back to it)."""
        L = lib()
        return bool(L.msmp_tune_query(b'lem_wide')) and bool(L.msmp_tune_query(b'split')) and self.wide_kernel_exists()

    def forward_wide(self, xin, states=None):
        """xin [N, T, ninp] node-major fp32 CUDA, states (y0, z0) or None -> (y_T, z_T) on the width-generic HIP recurrence kernel."""
        x = _padded_inputs(xin)
        n, t_len = x.shape[0], x.shape[1]
        y0, z0 = (None, None) if states is None else (_state(states[0]), _state(states[1]))
        y = torch.empty(n, self.nhid, dtype=torch.float32, device=x.device)
        z = torch.empty_like(y)
        check(lib().msmp_lem_encoder_wide_f32(ptr(x), n, t_len, self.ninp, self.nhid, self.dt, ptr(self._pack_wide()), ptr(y0), ptr(z0),
                                              ptr(y), ptr(z), current_stream()), 'msmp_lem_encoder_wide_f32')
        return y, z

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.nhid)
        for w in self.parameters():
            w.data.uniform_(-stdv, +stdv)

    def forward(self, inputs, states=None, return_state=False):
        """inputs [T, N, ninp] -> final y [N, nhid] (and z with return_state); `states` = (y0, z0) as in the reference
        (models_gnn.py:325-332), default zeros."""
        t_len, n, _ = inputs.shape
        nh = self.nhid
        infer = inputs.is_cuda and inputs.dtype == torch.float32 and not torch.is_grad_enabled()
        if infer and n > 0 and self.wide_kernel_selected():      # inference at any width (the GLU classes): one launch for all T steps
            y, z = self.forward_wide(inputs.permute(1, 0, 2), states)
            return (y, z) if return_state else y
        y, z = (inputs.new_zeros(n, nh), inputs.new_zeros(n, nh)) if states is None else states
        wy, wx = self.weights[:, :nh].t().contiguous(), self.weights[:, nh:].t().contiguous()
        zy, zx = self.weights_lin_z[:, :nh].t().contiguous(), self.weights_lin_z[:, nh:].t().contiguous()
        # input projections for all steps at once (the recurrent part stays sequential)
        gx = torch.matmul(inputs, wx) + self.bias          # [T, N, 3H]
        lx = torch.matmul(inputs, zx) + self.bias_lin_z    # [T, N, H]
        if infer:
            # msmp_tune("lem_wide", 0) / the exact-fp32 path: the two recurrent GEMMs are library calls, the pointwise work between them is
            # one HIP launch each (msmp_wide_lem_z_f32 / _y_f32)
            L = lib()
            y, z = y.contiguous().clone(), z.contiguous().clone()
            dt_bar = torch.empty_like(y)
            for t in range(t_len):
                g = torch.addmm(gx[t], y, wy)
                check(L.msmp_wide_lem_z_f32(ptr(g), n, nh, float(self.dt), ptr(z), ptr(dt_bar), current_stream()), 'msmp_wide_lem_z_f32')
                lin = torch.addmm(lx[t], z, zy)
                check(L.msmp_wide_lem_y_f32(ptr(lin), ptr(dt_bar), n * nh, ptr(y), current_stream()), 'msmp_wide_lem_y_f32')
            return (y, z) if return_state else y
        for t in range(t_len):
            g = torch.addmm(gx[t], y, wy)
            dt_bar = self.dt * torch.sigmoid(g[:, :nh])
            dt_ = self.dt * torch.sigmoid(g[:, nh:2 * nh])
            z = (1.0 - dt_) * z + dt_ * torch.tanh(g[:, 2 * nh:])
            y = (1.0 - dt_bar) * y + dt_bar * torch.tanh(torch.addmm(lx[t], z, zy))
        return (y, z) if return_state else y


def _train_forward(rnn, x, y0, z0, saved=None):
    """msmp_lem_train_fwd_wide_f32: the fp32-exact recurrence at any width (recurrent.forward_launch)."""
    return forward_launch('msmp_lem_train_fwd_wide_f32', x, rnn.ninp, rnn.nhid, (rnn.dt,), rnn._pack_wide_train, y0, z0, saved)


# saved planes a2, c, a1, d, y_{t-1}, z'; dG gates g1, g2, g3 (rows of `weights` / `bias`, against [y_{t-1} ; x_t]) and lin (`weights_lin_z` /
# `bias_lin_z`, against [z' ; x_t])
_CELL = Cell('msmp_lem_wide_saved_floats', 'msmp_packed_lem_wide_bwd_floats', 'msmp_pack_lem_wide_bwd_f32', 'msmp_lem_train_bwd_wide_f32',
             n_states=2, gate_planes=(4, 4, 4, 5),
             grads=lambda rows, w, nh: (None, None, rows(0, (0, 1, 2)).to(w[0].dtype), rows(0, (3,)).to(w[1].dtype), rows(1, (0, 1, 2)),
                                        rows(1, (3,)), None, None))


class _LEMTrainFunction(torch.autograd.Function):
    """LEMFunction of the reference (experiments/models_gnn.py:285-302) on the HIP training kernels at any hidden width 1..256: forward =
    msmp_lem_train_fwd_wide_f32 (saves the per-step activations), backward = msmp_lem_train_bwd_wide_f32 + the weight-gradient jobs
    (recurrent.py).  Like the reference it returns no gradient for the step inputs, nor for the initial states."""

    @staticmethod
    def forward(ctx, rnn, xin, weights, weights_lin_z, bias, bias_lin_z, y0=None, z0=None):
        return train_forward(ctx, _CELL, lambda x, y0, z0, saved: _train_forward(rnn, x, y0, z0, saved), rnn.ninp, rnn.nhid, xin,
                             (weights, weights_lin_z), y0, z0, (rnn.dt,))

    backward = staticmethod(train_backward)


_LEMWideTrainFunction = _LEMTrainFunction       # its name while a 128-wide Function stood beside it: the test suite of that revision, run against this library, imports it

class LEM(nn.Module):
    """experiments/models_gnn.py:333-342: returns all_y[-1].

    `forward` / `forward_nodes` are the differentiable path; `_recurrence` is where they are routed (the table is in its docstring).  There
    is NO CPU path: host tensors raise.  TRAIN_KERNELS = False is a validation aid only (scripts/train_soak.py, scripts/train_step_time.py):
    under autograd it routes GPU tensors through the PyTorch-ROCm restatement `LEMcuda.forward`, which the tests also call directly in
    float64 as the reference of the kernels.  `encode` / `encode_nodes` are the product path for inference at width 128: the fused HIP
    kernel (recurrence + lemoutput_mlp in one launch, states in registers)."""
    TRAIN_KERNELS = True

    def __init__(self, ninp, nhid, dt=1.):
        super().__init__()
        self.ninp, self.nhid = ninp, nhid
        self.rnn = LEMcuda(ninp, nhid, dt)
        self._packed = PackedCache()

    def forward(self, inputs):
        """inputs [T, N, ninp] (the reference's layout) -> all_y[-1] [N, nhid]."""
        return self.forward_nodes(inputs.permute(1, 0, 2))

    def forward_nodes(self, xin):
        """Same with node-major step inputs xin [N, T, ninp] (the layout the kernels read)."""
        return self._recurrence(xin, None)[0]

    def _recurrence(self, xin, states):
        """xin [N, T, ninp], states = (y0, z0) or None (zeros) -> (y_T, z_T).  The one place where LEM and LEMS choose a path.  With
        "native" = module fp32 on the GPU, inputs fp32 (at width 128 any dtype: they are cast), N > 0, ninp <= 8, width <= 256, and
        "backward" = grad enabled and a parameter requires grad:

            native, backward, TRAIN_KERNELS, msmp_tune "lem_wide_train" != 0   _LEMTrainFunction (msmp_lem_train_fwd_wide_f32 with `saved`, then
                                                                               msmp_lem_train_bwd_wide_f32 + msmp_grad_weights_cat_f32)
            native, no backward, width 128                                     msmp_lem_train_fwd_wide_f32 with saved = NULL: fp32-exact and it takes
                                                                               initial states (the weight-stationary inference kernel does neither)
            other widths, no grad, fp32 module, N > 0, wide_kernel_selected()  LEMcuda.forward_wide: msmp_lem_encoder_wide_f32 on xin as it is
            everything else                                                    LEMcuda.forward: without grad the GEMM + pointwise loop; under
                                                                               autograd (switch 0, TRAIN_KERNELS = False, float64) the PyTorch-ROCm
                                                                               restatement of the cell
        """
        if not xin.is_cuda:
            raise RuntimeError(f'{type(self).__name__} needs CUDA tensors; there is no CPU fallback')
        r = self.rnn
        y0, z0 = states if states is not None else (None, None)
        fp32_module = all(p.dtype == torch.float32 and p.is_cuda for p in r.parameters())
        if (xin.dtype == torch.float32 or self.nhid == 128) and xin.shape[0] > 0 and r.wide_kernel_exists() and fp32_module:
            if torch.is_grad_enabled() and any(p.requires_grad for p in r.parameters()):
                if self.TRAIN_KERNELS and lib().msmp_tune_query(b'lem_wide_train') != 0:
                    return _LEMTrainFunction.apply(r, xin, r.weights, r.weights_lin_z, r.bias, r.bias_lin_z, y0, z0)
            elif self.nhid == 128:
                return _train_forward(r, _padded_inputs(xin), _state(y0), _state(z0))
        if self.nhid != 128 and not torch.is_grad_enabled() and xin.shape[0] > 0 and fp32_module and r.wide_kernel_selected():
            return r.forward_wide(xin, states)
        return r(xin.permute(1, 0, 2).contiguous().to(r.weights.dtype), states, return_state=True)

    def _pack(self, mlp):
        ps = [self.rnn.weights, self.rnn.weights_lin_z, self.rnn.bias, self.rnn.bias_lin_z]
        if mlp is not None:
            ps += [mlp[0].weight, mlp[0].bias, mlp[2].weight, mlp[2].bias]

        def build():
            L = lib()
            blob = torch.empty(L.msmp_packed_lem_floats(), dtype=torch.float32, device=ps[0].device)
            f = [p.detach().to(torch.float32).contiguous() for p in ps]
            args = [ptr(t) for t in f] + [None] * (8 - len(f))
            check(L.msmp_pack_lem_f32(*args, self.ninp, ptr(blob), current_stream()), 'msmp_pack_lem_f32')
            return blob
        return self._packed.get(ps, build)

    def encode_nodes(self, u, pos_x, pos_t, variables, dt_cum, two_d, mlp=None):
        """Same as `encode` with the step inputs assembled inside the kernel from the node arrays (models_gnn.py:1357-1360 /
        models_gnn2D.py:429-433).  Returns None on the exact-fp32 path (msmp_tune "split" 0), which has no such entry."""
        L = lib()
        n, nv = u.shape[0], variables.shape[1]
        tw = u.shape[1] // (2 if two_d else 1)
        assert self.nhid == 128 and self.ninp == (3 if two_d else 2) + nv
        t = [x.to(torch.float32).contiguous() for x in (u, pos_x, pos_t, variables, dt_cum)]
        out = torch.empty(n, self.nhid, dtype=torch.float32, device=u.device)
        rc = L.msmp_lem_encoder_nodes_f32(ptr(t[0]), ptr(t[1]), ptr(t[2]), ptr(t[3]), ptr(t[4]), n, tw, nv, int(two_d), self.rnn.dt,
                                          ptr(self._pack(mlp)), int(mlp is not None), ptr(out), current_stream())
        if rc == MSMP_ERR_UNSUPPORTED:
            return None
        check(rc, 'msmp_lem_encoder_nodes_f32')
        return out

    def encode(self, xin, mlp=None):
        """xin [N, T, ninp] float32 CUDA (node-major step inputs) -> [N, nhid]; `mlp` = lemoutput_mlp
        (nn.Sequential(Linear, Swish, Linear, Swish)) to fuse behind the recurrence."""
        assert self.nhid == 128 and xin.shape[2] == self.ninp
        L = lib()
        n, t_len, _ = xin.shape
        stride = L.msmp_lem_input_stride(self.ninp)
        if stride != self.ninp:
            xin = torch.nn.functional.pad(xin, (0, stride - self.ninp))
        xin = xin.to(torch.float32).contiguous()
        out = torch.empty(n, self.nhid, dtype=torch.float32, device=xin.device)
        check(L.msmp_lem_encoder_f32(ptr(xin), n, t_len, self.ninp, self.rnn.dt, ptr(self._pack(mlp)),
                                     int(mlp is not None), ptr(out), current_stream()), 'msmp_lem_encoder_f32')
        return out


class LEMS(LEM):
    """experiments/models_gnn.py:345-362: the LEM that keeps (all_y[-1], all_z[-1]) of a call as the initial states of the next
    (`reset_states()` starts a new unrolling sequence; train_helper.py:144-145, 199-200).  The carried states are constants for
    the next call.  Same routes as LEM (LEM._recurrence), all of which take initial states."""

    def __init__(self, ninp, nhid, dt=1.):
        super().__init__(ninp, nhid, dt)
        self.states = None

    def reset_states(self):
        self.states = None

    def forward_nodes(self, xin):
        y, z = self._recurrence(xin, self.states)
        self.states = (y.detach(), z.detach())
        return y

    def encode(self, *args, **kwargs):
        raise RuntimeError('LEMS is stateful: use forward / forward_nodes')

    encode_nodes = encode
