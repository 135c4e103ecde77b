// LEM encoder for TRAINING at any hidden width 1 <= W <= 256 (the 128-wide classes and the GLU classes' 164 alike):
// the T-step recurrence with its per-step activations saved, and its backward pass (back-propagation through time) as one kernel each,
// replacing `lem_cuda.forward` / `lem_cuda.backward` of the reference's absent extension (experiments/models_gnn.py:285-302:
// LEMFunction.forward saves all_X, all_X2, all_multi_scales, all_lin_new_z_state ...; LEMFunction.backward returns the gradients of weights,
// weights_lin_z, bias, bias_lin_z and drops the gradient of `inputs`, :296-302).
//   msmp_lem_train_fwd_wide_f32   the T-step recurrence from (y0, z0) to (y_T, z_T), saving per step a2, c, a1, d, y_{t-1}, z'
//   msmp_lem_train_bwd_wide_f32   back-propagation through time: dL/dy_T -> dG = (dg1 | dg2 | dg3 | dl) per node and step
//
// Forward (per step, per node; same cell as lem_kernel.hip):
//     g = W [y ; x_t] + b;  a1 = dt s(g1);  a2 = dt s(g2);  c = tanh(g3);  z' = (1-a2) z + a2 c
//     l = Wz [z' ; x_t] + bz;  d = tanh(l);  y' = (1-a1) y + a1 d
// Backward (t = T-1 .. 0, carrying dy = dL/dy_t and dz = dL/dz_t):
//     da1 = dy (d - y);  dd = dy a1;  dy <- dy (1-a1);  dl = dd (1-d^2);  dg1 = da1 a1 (1 - a1/dt)
//     dz += Wz[:, :W]^T dl;  da2 = dz (c - z);  dc = dz a2;  dz <- dz (1-a2);  dg2 = da2 a2 (1 - a2/dt);  dg3 = dc (1-c^2)
//     dy += W[:, :W]^T (dg1, dg2, dg3)
// The parameter gradients are then plain GEMMs over the N*T rows (dW = dG[:, :3]^T [y_prev ; x], dWz = dl^T [z' ; x]) and column sums:
// msmp_grad_weights_cat_f32 jobs of 128 columns of dG each, issued by the host layer.  The saved planes are node-major, so each is directly
// the row matrix of those GEMMs.
//
// The workgroup shape, the weight stream, the publish and every memory layout are the recurrent scaffold's, described once at the head of
// recurrent_train.h; this file is the LEM cell.  Barriers per step: 4 forward (y is read by three products, z' by one), 8 backward.  The backward
// writes the pad columns of dG before the gate gradients: at width 128 that order holds 168 registers (three workgroups per CU), the other 180
// (two), and both take the same time (profiles/r24a_recurrent_scaffold.md).  Pad channels W .. Wp - 1: a1 = a2 = dt / 2 and c = d = 0 there, so their z and y stay exact zeros.
//
//   saved planes   a2, c, a1, d, y_{t-1}, z'  (pad channels: dt / 2 in a1, a2; 0 elsewhere)
//   dG gate order  g1, g2, g3, lin: the cell's gate numbering below
//   stream positions   forward g2, g3, g1, lin; backward g1, lin, g2, g3 (consumption order)
#include "recurrent_train.h"

namespace msmp {

enum { LWT_A2 = 0, LWT_C = 1, LWT_A1 = 2, LWT_D = 3, LWT_Y = 4, LWT_Z = 5 };

struct LemCell {
    struct Scalars {
        float dt;
    };
    // pack tensors: weights [3 W, W + ninp] (gates g1, g2, g3), weights_lin_z [W, W + ninp] (lin), bias [3 W], bias_lin_z [W]
    static __device__ __forceinline__ int fwd_gate(int pos) { return pos == 0 ? 1 : pos == 1 ? 2 : pos == 2 ? 0 : 3; }
    static __device__ __forceinline__ int bwd_gate(int pos) { return pos == 0 ? 0 : pos == 1 ? 3 : pos == 2 ? 1 : 2; }
    static __device__ __forceinline__ const float* rec(const RtPackArgs& a, int gate, int row, int col) {
        const float* m = gate == 3 ? a.p[1] : a.p[0];
        return m + (size_t)((gate == 3 ? 0 : gate * a.width) + row) * (a.width + a.ninp) + col;
    }
    static __device__ __forceinline__ const float* input(const RtPackArgs& a, int gate, int row, int f) { return rec(a, gate, row, a.width + f); }
    static __device__ __forceinline__ float bias(const RtPackArgs& a, int gate, int row) {
        const float* m = gate == 3 ? a.p[3] : a.p[2];
        return m[(gate == 3 ? 0 : gate * a.width) + row];
    }

    template <int KT, int NS>
    static __device__ __forceinline__ void forward(const RtFwdArgs<LemCell>& a, u32x4* xf) {
        const float dt = a.k.dt;
        f32x16 y, z, g, acc;
        RtFwd<KT, NS> c;
        rt_fwd_begin(c, a, xf, y, z);
        for (int t = 0; t < a.t_len; ++t) {
            RtStep<NS> in;
            rt_step_begin(c, t, in);
            rt_save(c, in, LWT_Y, y);                                    // y_{t-1}, the state ENTERING the step
            rt_tile_init(c, 0, in, g);                                   // g2 -> a2            (published: y)
            rt_gemm<0>(c, g);
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = dt * sigmoidf_(g[r]);
            rt_save(c, in, LWT_A2, g);
            rt_tile_init(c, 1, in, acc);                                 // g3 -> c, z'
            rt_gemm<1>(c, acc);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[r] = tanhf_(acc[r]);
                z[r] = (1.0f - g[r]) * z[r] + g[r] * acc[r];
            }
            rt_save(c, in, LWT_C, acc);
            rt_save(c, in, LWT_Z, z);
            rt_tile_init(c, 2, in, g);                                   // g1 -> a1
            rt_gemm<2>(c, g);
            __syncthreads();                                             // every wave has read the last fragment of y
#pragma unroll
            for (int r = 0; r < 16; ++r) g[r] = dt * sigmoidf_(g[r]);
            rt_save(c, in, LWT_A1, g);
            rt_publish(c, z);
            rt_tile_init(c, 3, in, acc);                                 // lin -> d, y'        (published: z')
            __syncthreads();
            rt_gemm<3>(c, acc);
            __syncthreads();                                             // every wave has read the last fragment of z'
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                acc[r] = tanhf_(acc[r]);
                y[r] = (1.0f - g[r]) * y[r] + g[r] * acc[r];
            }
            rt_save(c, in, LWT_D, acc);
            rt_publish(c, y);
            __syncthreads();
        }
        rt_fwd_end(c, a, y, z);
    }
};

template <int KT>
__global__ __launch_bounds__(64 * KT) void lem_wide_train_fwd_kernel(RtFwdArgs<LemCell> a) {
    __shared__ u32x4 xf[KT * LWT_KTILE_U4];                          // 6 KT KB: y, then z', alternately
    rt_forward<LemCell, KT>(a, xf);
}

template <int KT>
__global__ __launch_bounds__(64 * KT) void lem_wide_bptt_kernel(RtBwdArgs<LemCell> a) {
    __shared__ u32x4 xf[KT * LWT_KTILE_U4];
    const float inv_dt = 1.0f / a.k.dt;
    f32x16 dy, dz, p, q;
    RtBwd<KT> c;
    rt_bwd_begin(c, a, xf, dy, dz);
    for (int t = a.t_len - 1; t >= 0; --t) {
        const float* st = c.srow + (size_t)t * c.WP;
        float* gt = c.grow + (size_t)t * (4 * c.ldg);
        {   // y' = (1-a1) y + a1 d:  p = dg1, q = dl
            f32x16 a1, d, yp;
            rt_saved(c, st, LWT_A1, a1);
            rt_saved(c, st, LWT_D, d);
            rt_saved(c, st, LWT_Y, yp);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float gr = dy[r];
                q[r] = gr * a1[r] * (1.0f - d[r] * d[r]);
                p[r] = gr * (d[r] - yp[r]) * a1[r] * (1.0f - a1[r] * inv_dt);
                dy[r] = gr * (1.0f - a1[r]);
            }
        }
        rt_dg_pad(c, gt);
        rt_dg_write(c, gt, p);
        rt_dg_write(c, gt + 3 * c.ldg, q);
        rt_product<0>(c, p, dy);                                     // dy += W_g1^T dg1
        rt_product<1>(c, q, dz);                                     // dz += Wz^T dl
        {   // z' = (1-a2) z + a2 c:  p = dg2, q = dg3
            f32x16 a2, cc, zp;
            rt_saved(c, st, LWT_A2, a2);
            rt_saved(c, st, LWT_C, cc);
            rt_entering_c(c, st, t, LWT_Z, a.c0, zp);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float gr = dz[r];
                q[r] = gr * a2[r] * (1.0f - cc[r] * cc[r]);
                p[r] = gr * (cc[r] - zp[r]) * a2[r] * (1.0f - a2[r] * inv_dt);
                dz[r] = gr * (1.0f - a2[r]);
            }
        }
        rt_dg_write(c, gt + c.ldg, p);
        rt_dg_write(c, gt + 2 * c.ldg, q);
        rt_product<2>(c, p, dy);                                     // dy += W_g2^T dg2
        rt_product<3>(c, q, dy);                                     // dy += W_g3^T dg3
    }
}

}  // namespace msmp

using namespace msmp;

extern "C" int64_t msmp_packed_lem_wide_train_floats(int ninp, int width) {
    return rt_packed_floats("msmp_packed_lem_wide_train_floats", ninp, width, false);
}
extern "C" int64_t msmp_packed_lem_wide_bwd_floats(int ninp, int width) { return rt_packed_floats("msmp_packed_lem_wide_bwd_floats", ninp, width, true); }
extern "C" int64_t msmp_lem_wide_saved_floats(int64_t n_nodes, int t_len, int width) {
    return rt_rows_floats("msmp_lem_wide_saved_floats", n_nodes, t_len, width, false);
}
extern "C" int64_t msmp_lem_wide_dg_floats(int64_t n_nodes, int t_len, int width) {
    return rt_rows_floats("msmp_lem_wide_dg_floats", n_nodes, t_len, width, true);
}

extern "C" int msmp_pack_lem_wide_train_f32(const float* weights, const float* weights_lin_z, const float* bias, const float* bias_lin_z,
                                            int ninp, int width, float* packed_out, msmp_stream_t stream) {
    return rt_pack<LemCell, false>("msmp_pack_lem_wide_train_f32", "pack_lem_wide_train_kernel", weights && weights_lin_z && bias && bias_lin_z,
                                   {{weights, weights_lin_z, bias, bias_lin_z}, ninp, width, (width + 31) / 32, packed_out}, stream);
}

extern "C" int msmp_pack_lem_wide_bwd_f32(const float* weights, const float* weights_lin_z, int ninp, int width, float* packed_out,
                                          msmp_stream_t stream) {
    return rt_pack<LemCell, true>("msmp_pack_lem_wide_bwd_f32", "pack_lem_wide_train_kernel", weights && weights_lin_z,
                                  {{weights, weights_lin_z, nullptr, nullptr}, ninp, width, (width + 31) / 32, packed_out}, stream);
}

extern "C" int msmp_lem_train_fwd_wide_f32(const float* xin, int64_t n_nodes, int t_len, int ninp, int width, float dt, const float* packed,
                                           const float* y0, const float* z0, float* saved, float* y_out, float* z_out, msmp_stream_t stream) {
    return rt_fwd_entry<LemCell>("msmp_lem_train_fwd_wide_f32", "lem_wide_train_fwd_kernel", xin, n_nodes, t_len, ninp, width, {dt}, packed, y0, z0,
                                 saved, y_out, z_out, stream, [](auto K) { return lem_wide_train_fwd_kernel<decltype(K)::value>; });
}

extern "C" int msmp_lem_train_bwd_wide_f32(const float* grad_y, const float* saved, const float* y0, const float* z0, int64_t n_nodes, int t_len,
                                           int width, float dt, const float* packed_bwd, float* dg_out, msmp_stream_t stream) {
    const char* who = "msmp_lem_train_bwd_wide_f32";
    if (!wide_width_ok(who, width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(t_len >= 1 && dt != 0.f, MSMP_ERR_ARG, "%s: t_len=%d < 1 or dt = 0", who, t_len);
    return rt_bwd_entry<LemCell>(who, "lem_wide_bptt_kernel", grad_y, saved, z0, (y0 == nullptr) == (z0 == nullptr), n_nodes, t_len, width, {dt},
                                 packed_bwd, dg_out, stream, [](auto K) { return lem_wide_bptt_kernel<decltype(K)::value>; });
}
