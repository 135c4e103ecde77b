// LSTM encoder of the LSTM ablation classes (experiments/models_gnn.py:758-767: torch.nn.LSTM(ninp, nhid), one layer, unidirectional, no
// projection; output[-1] = h_T) at any hidden width 1 <= W <= 256, for training AND inference: the T-step recurrence, with its per-step
// activations saved when a backward follows, and its back-propagation through time, one kernel each.
//   msmp_lstm_train_fwd_f32   the T-step recurrence from (h0, c0) to (h_T, c_T), saving per step i, f, g, o, c_t, h_{t-1} (saved = NULL: nothing)
//   msmp_lstm_train_bwd_f32   back-propagation through time: dL/dh_T -> dG = (di | df | dg | do) pre-activation gradients per node and step
//
// Forward (per step, per node; gate order i, f, g, o as in torch: rows [0, W), [W, 2W), [2W, 3W), [3W, 4W) of weight_ih / weight_hh):
//     G = W_hh h + W_ih x_t + (b_ih + b_hh);  i = s(G_i);  f = s(G_f);  g = tanh(G_g);  o = s(G_o);  c' = f c + i g;  h' = o tanh(c')
// Backward (t = T-1 .. 0, carrying dh = dL/dh_t and dc = dL/dc_t, dc = 0 at the start: only h_T is an output):
//     th = tanh(c_t);  do = dh th;  dc += dh o (1 - th^2);  di = dc g;  dg = dc i;  df = dc c_{t-1};  dc <- dc f
//     dG = (di i (1-i) | df f (1-f) | dg (1-g^2) | do o (1-o));  dh <- W_hh^T dG
// The parameter gradients are then plain GEMMs over the N*T rows (dW_hh = dG^T h_{t-1}, dW_ih = dG^T x_t) and column sums (the gradient of
// both biases): msmp_grad_weights_cat_f32 jobs of 128 columns of dG each, issued by the host layer.  The saved planes are node-major, so the
// h_{t-1} plane is directly the row matrix of those GEMMs.
//
// The workgroup shape, the weight stream, the publish and every memory layout are the recurrent scaffold's, described once at the head of
// recurrent_train.h; this file is the LSTM cell.  The four gates of a step depend on the SAME h (the LEM's two products are dependent), so the
// forward needs 2 barriers per step -- h is published once and read by four products; the backward accumulates dh over four published gate
// gradients: 8 barriers per step.  Pad channels W .. Wp - 1: i = f = o = 1/2 and g = 0 there, so their c and h stay exact zeros.
//
//   saved planes   i, f, g, o, c_t, h_{t-1}  (pad channels: 1/2 in i, f, o; 0 in g, c, h)
//   dG gate order  i, f, g, o: torch's, the cell's gate numbering below
//   stream positions   forward i, g, f, o (c' needs i g before f); backward o, i, g, f (the order their gradients are formed in)
#include "recurrent_train.h"

namespace msmp {

enum { LST_I = 0, LST_F = 1, LST_G = 2, LST_O = 3, LST_C = 4, LST_H = 5 };

struct LstmCell {
    struct Scalars {};
    // pack tensors: weight_ih [4 W, ninp], weight_hh [4 W, W], bias_ih [4 W], bias_hh [4 W]; the bias of the blob is b_ih + b_hh
    static __device__ __forceinline__ int fwd_gate(int pos) { return pos == 1 ? 2 : pos == 2 ? 1 : pos; }
    static __device__ __forceinline__ int bwd_gate(int pos) { return pos == 0 ? 3 : pos == 1 ? 0 : pos == 2 ? 2 : 1; }
    static __device__ __forceinline__ const float* rec(const RtPackArgs& a, int gate, int row, int col) {
        return a.p[1] + ((size_t)gate * a.width + row) * a.width + col;
    }
    static __device__ __forceinline__ const float* input(const RtPackArgs& a, int gate, int row, int f) {
        return a.p[0] + ((size_t)gate * a.width + row) * a.ninp + f;
    }
    static __device__ __forceinline__ float bias(const RtPackArgs& a, int gate, int row) { return a.p[2][gate * a.width + row] + a.p[3][gate * a.width + row]; }

    template <int KT, int NS>
    static __device__ __forceinline__ void forward(const RtFwdArgs<LstmCell>& a, u32x4* xf) {
        f32x16 h, cs, ig, acc;
        RtFwd<KT, NS> c;
        rt_fwd_begin(c, a, xf, h, cs);
        for (int t = 0; t < a.t_len; ++t) {
            RtStep<NS> in;
            rt_step_begin(c, t, in);
            rt_save(c, in, LST_H, h);                                    // h_{t-1}, the state ENTERING the step (published)
            rt_tile_init(c, 0, in, ig);                                  // i
            rt_gemm<0>(c, ig);
#pragma unroll
            for (int r = 0; r < 16; ++r) ig[r] = sigmoidf_(ig[r]);
            rt_save(c, in, LST_I, ig);
            rt_tile_init(c, 1, in, acc);                                 // g -> i g
            rt_gemm<1>(c, acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = tanhf_(acc[r]);
            rt_save(c, in, LST_G, acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) ig[r] *= acc[r];
            rt_tile_init(c, 2, in, acc);                                 // f -> c'
            rt_gemm<2>(c, acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[r] = sigmoidf_(acc[r]);
                cs[r] = acc[r] * cs[r] + ig[r];
            }
            rt_save(c, in, LST_F, acc);
            rt_save(c, in, LST_C, cs);
            rt_tile_init(c, 3, in, acc);                                 // o -> h'
            rt_gemm<3>(c, acc);
            __syncthreads();                                             // every wave has read the last fragment of h
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[r] = sigmoidf_(acc[r]);
                h[r] = acc[r] * tanhf_(cs[r]);
            }
            rt_save(c, in, LST_O, acc);
            rt_publish(c, h);
            __syncthreads();
        }
        rt_fwd_end(c, a, h, cs);
    }
};

template <int KT>
__global__ __launch_bounds__(64 * KT) void lstm_train_fwd_kernel(RtFwdArgs<LstmCell> a) {
    __shared__ u32x4 xf[KT * LWT_KTILE_U4];                          // 6 KT KB: h
    rt_forward<LstmCell, KT>(a, xf);
}

template <int KT>
__global__ __launch_bounds__(64 * KT) void lstm_bptt_kernel(RtBwdArgs<LstmCell> a) {
    __shared__ u32x4 xf[KT * LWT_KTILE_U4];
    f32x16 dh, dc, p, q;
    RtBwd<KT> c;
    rt_bwd_begin(c, a, xf, dh, dc);
    for (int t = a.t_len - 1; t >= 0; --t) {
        const float* st = c.srow + (size_t)t * c.WP;
        float* gt = c.grow + (size_t)t * (4 * c.ldg);
        {   // h' = o tanh(c'):  p = dG_o, dc += dh o (1 - th^2); dh is consumed here and rebuilt by the four products
            f32x16 o, cc;
            rt_saved(c, st, LST_O, o);
            rt_saved(c, st, LST_C, cc);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float th = tanhf_(cc[r]), gr = dh[r];
                p[r] = gr * th * o[r] * (1.0f - o[r]);
                dc[r] += gr * o[r] * (1.0f - th * th);
                dh[r] = 0.f;
            }
        }
        rt_dg_pad(c, gt);
        rt_gate_product<0>(c, gt + LST_O * c.ldg, p, dh);
        {   // c' = f c + i g:  p = dG_i, q = dG_g
            f32x16 gi, gg;
            rt_saved(c, st, LST_I, gi);
            rt_saved(c, st, LST_G, gg);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                p[r] = dc[r] * gg[r] * gi[r] * (1.0f - gi[r]);
                q[r] = dc[r] * gi[r] * (1.0f - gg[r] * gg[r]);
            }
        }
        rt_gate_product<1>(c, gt + LST_I * c.ldg, p, dh);
        rt_gate_product<2>(c, gt + LST_G * c.ldg, q, dh);
        {   // p = dG_f, dc <- dc f
            f32x16 f, cp;
            rt_saved(c, st, LST_F, f);
            rt_entering_c(c, st, t, LST_C, a.c0, cp);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                p[r] = dc[r] * cp[r] * f[r] * (1.0f - f[r]);
                dc[r] *= f[r];
            }
        }
        rt_gate_product<3>(c, gt + LST_F * c.ldg, p, dh);
    }
}

}  // namespace msmp

using namespace msmp;

extern "C" int64_t msmp_packed_lstm_train_floats(int ninp, int width) { return rt_packed_floats("msmp_packed_lstm_train_floats", ninp, width, false); }
extern "C" int64_t msmp_packed_lstm_bwd_floats(int ninp, int width) { return rt_packed_floats("msmp_packed_lstm_bwd_floats", ninp, width, true); }
extern "C" int64_t msmp_lstm_saved_floats(int64_t n_nodes, int t_len, int width) {
    return rt_rows_floats("msmp_lstm_saved_floats", n_nodes, t_len, width, false);
}
extern "C" int64_t msmp_lstm_dg_floats(int64_t n_nodes, int t_len, int width) { return rt_rows_floats("msmp_lstm_dg_floats", n_nodes, t_len, width, true); }

extern "C" int msmp_pack_lstm_train_f32(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int ninp, int width,
                                        float* packed_out, msmp_stream_t stream) {
    return rt_pack<LstmCell, false>("msmp_pack_lstm_train_f32", "pack_lstm_train_kernel", w_ih && w_hh && b_ih && b_hh,
                                    {{w_ih, w_hh, b_ih, b_hh}, ninp, width, (width + 31) / 32, packed_out}, stream);
}

extern "C" int msmp_pack_lstm_bwd_f32(const float* w_hh, int ninp, int width, float* packed_out, msmp_stream_t stream) {
    return rt_pack<LstmCell, true>("msmp_pack_lstm_bwd_f32", "pack_lstm_train_kernel", w_hh != nullptr,
                                   {{nullptr, w_hh, nullptr, nullptr}, ninp, width, (width + 31) / 32, packed_out}, stream);
}

extern "C" int msmp_lstm_train_fwd_f32(const float* xin, int64_t n_nodes, int t_len, int ninp, int width, const float* packed, const float* h0,
                                       const float* c0, float* saved, float* h_out, float* c_out, msmp_stream_t stream) {
    return rt_fwd_entry<LstmCell>("msmp_lstm_train_fwd_f32", "lstm_train_fwd_kernel", xin, n_nodes, t_len, ninp, width, {}, packed, h0, c0, saved,
                                  h_out, c_out, stream, [](auto K) { return lstm_train_fwd_kernel<decltype(K)::value>; });
}

extern "C" int msmp_lstm_train_bwd_f32(const float* grad_h, const float* saved, const float* c0, int64_t n_nodes, int t_len, int width,
                                       const float* packed_bwd, float* dg_out, msmp_stream_t stream) {
    const char* who = "msmp_lstm_train_bwd_f32";
    if (!wide_width_ok(who, width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(t_len >= 1, MSMP_ERR_ARG, "%s: t_len=%d < 1", who, t_len);
    return rt_bwd_entry<LstmCell>(who, "lstm_bptt_kernel", grad_h, saved, c0, true, n_nodes, t_len, width, {}, packed_bwd, dg_out, stream,
                                  [](auto K) { return lstm_bptt_kernel<decltype(K)::value>; });
}
