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
// The shape is that of lem_wide_train_kernel.hip (described at its head; the pieces are train_frags.h): one 32-node tile per workgroup, 64 KT
// threads, KT = ceil(W / 32); wave ct owns channels 32 ct .. of all four gates and of c and h (forward) / dh and dc (backward) in accumulator
// layout for all T steps, so the pointwise cell is wave-local.  The B operand of a product (h forward; one gate gradient after the other
// backward) is published in LDS as bf16 hi / mid / lo fragments in acc order, 6 KT KB, ONE area reused between barriers; the A operand is
// this wave's 32 rows of each gate's block of W_hh (forward) or of its transpose (backward), streamed from the L2-resident blob through
// buffer loads one k-tile ahead in consumption order; six v_mfma_f32_32x32x16_bf16 per K = 16 step, fp32-exact products.  No fp16 anywhere:
// there is no input range and the kernels neither read nor raise the range status.  The four gates of a step depend on the SAME h (the LEM's
// two products are dependent), so the forward needs 2 barriers per step -- h is published once and read by four products; the backward
// accumulates dh over four published gate gradients: 8 barriers per step.
// Channels W .. Wp - 1 carry zero weights and zero bias: i = f = o = 1/2 and g = 0 there, so their c and h stay exact zeros, their dG is an
// exact zero, and they are never written to h_out / c_out.  A node's arithmetic depends on nothing but its own row.
//
// Memory layouts (all fp32):
//   saved  [6][N][T][Wp]            planes i, f, g, o, c_t, h_{t-1}; every element is written (pad channels: 1/2 in i, f, o; 0 in g, c, h)
//   dG     [N][T][4][ldg]           ldg = 128 ceil(W / 128); gate order i, f, g, o; columns W .. ldg - 1 are written as 0
#include "lem_layout.h"       // LEM_MAX_INP, tanhf_
#include "train_frags.h"

namespace msmp {

enum { LST_I = 0, LST_F = 1, LST_G = 2, LST_O = 3, LST_C = 4, LST_H = 5, LST_PLANES = 6 };

// forward blob (floats), kt = ceil(W / 32), Wp = 32 kt; "position" p is the place of a gate in the wave's stream, i, g, f, o forward (c' needs
// i g before f) -- torch gate 0, 2, 1, 3:
//   rec  [wave ct kt][position 4][k-tile kc kt][s 2][plane 3: hi, mid, lo][lane 64][8 bf16]: rows 32 ct .. of the gate's block of W_hh, columns
//        32 kc .., as bf16x3 A fragments in acc order (split_k_acc); a wave's stream of one time step is contiguous |
//   wx   [position 4][ct kt][s 4][lane 64]: W_ih as v_mfma_f32_32x32x2_f32 A fragments, W_ih[gate W + 32 ct + (lane & 31)][2 s + (lane >> 5)] |
//   bias [position 4][Wp]: b_ih + b_hh
// zero outside the matrices.
struct LstmTrainLayout {
    int64_t rec, wx, bias, total;
};
__host__ __device__ inline LstmTrainLayout lstm_train_layout(int kt) {
    LstmTrainLayout L;
    L.rec = 0;
    L.wx = L.rec + (int64_t)4 * kt * kt * LWT_KTILE_FLOATS;
    L.bias = L.wx + (int64_t)4 * kt * 256;
    L.total = L.bias + (int64_t)4 * kt * 32;
    return L;
}
// backward blob (floats): rec_t [wave ct kt][position 4: o, i, g, f (the order their gradients are formed in)][k-tile kc kt][s 2][plane 3][lane 64]
//   [8 bf16]: fragment row 32 ct + m, column 32 kc + kk  =  W_hh[gate W + 32 kc + kk][32 ct + m]: the TRANSPOSED blocks
__host__ __device__ inline int64_t lstm_bwd_floats(int kt) { return (int64_t)4 * kt * kt * LWT_KTILE_FLOATS; }

__host__ __device__ inline int lstm_fwd_gate(int position) { return position == 1 ? 2 : position == 2 ? 1 : position; }      // i, g, f, o
__host__ __device__ inline int lstm_bwd_gate(int position) { return position == 0 ? 3 : position == 1 ? 0 : position == 2 ? 2 : 1; }      // o, i, g, f

struct LstmTrainPackArgs {
    const float *w_ih, *w_hh, *b_ih, *b_hh;
    int ninp, width, kt;
    float* out;
};

// TRANSPOSED = false: the forward blob; true: the backward blob (w_ih and the biases unused).  One thread per (ct, position, kc, s, lane).  The
// matrix element is selected by arithmetic on ONE pointer and read by one load (the note above lwt_weight of lem_wide_train_kernel.hip).
template <bool TRANSPOSED>
__global__ __launch_bounds__(256) void pack_lstm_train_kernel(LstmTrainPackArgs a) {
    const int kt = a.kt, W = a.width;
    const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t n_rec = (int64_t)4 * kt * kt * 2 * 64;
    for (int64_t p = tid0; p < n_rec; p += stride) {
        const int lane = (int)(p & 63), s = (int)(p >> 6) & 1;
        const int64_t q = p >> 7;
        const int kc = (int)(q % kt), pos = (int)((q / kt) & 3), ct = (int)(q / (4 * kt));
        const int row = 32 * ct + (lane & 31);
        const int gate = TRANSPOSED ? lstm_bwd_gate(pos) : lstm_fwd_gate(pos);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 32 * kc + split_k_acc(s, lane >> 5, j);
            const bool inside = row < W && k < W;
            const int r = inside ? (TRANSPOSED ? k : row) : 0, c = inside ? (TRANSPOSED ? row : k) : 0;
            const float w = a.w_hh[((size_t)gate * W + r) * W + c];
            v[j] = inside ? w : 0.f;
        }
        lwt_store_b3(a.out, p >> 6, lane, v);
    }
    if (TRANSPOSED) return;
    const LstmTrainLayout L = lstm_train_layout(kt);
    for (int64_t p = tid0; p < (int64_t)4 * kt * 256; p += stride) {
        const int lane = (int)(p & 63), s = (int)(p >> 6) & 3, ct = (int)((p >> 8) % kt), pos = (int)((p >> 8) / kt);
        const int row = 32 * ct + (lane & 31), f = 2 * s + (lane >> 5);
        const bool inside = row < W && f < a.ninp;
        const float w = a.w_ih[inside ? ((size_t)lstm_fwd_gate(pos) * W + row) * a.ninp + f : 0];
        a.out[L.wx + p] = inside ? w : 0.f;
    }
    for (int64_t p = tid0; p < (int64_t)4 * kt * 32; p += stride) {
        const int row = (int)(p % (32 * kt)), pos = (int)(p / (32 * kt));
        const int at = row < W ? lstm_fwd_gate(pos) * W + row : 0;
        const float b = a.b_ih[at] + a.b_hh[at];
        a.out[L.bias + p] = row < W ? b : 0.f;
    }
}

struct LstmTrainArgs {
    const float* xin;       // [N, T, stride]
    long n_nodes;
    int t_len, stride, width;
    const float *rec, *wx, *bias;
    float* saved;           // [6][N][T][Wp] or NULL
    const float *h0, *c0;   // [N, W] or NULL (zeros)
    float *h_out, *c_out;   // [N, W]; c_out may be NULL
};

// acc (tile ct) = bias + W_ih x_t of the gate at stream position `pos`: the input columns as ceil(ninp / 2) fp32 MFMA k-steps (the pad of an
// odd ninp is zero).  NS > 0: that many steps, x[s] = feature 2 s + hh of the lane's node.  NS = 0: `ns` steps, x[f] = feature f.
template <int KT, int NS>
__device__ __forceinline__ void lstm_tile_init(const LstmTrainArgs& a, int pos, int ct, int lane, int hh, int ns, const float (&x)[NS ? NS : 8], f32x16& acc) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + (pos * KT + ct) * 32 + 8 * q + 4 * hh);
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[4 * q + m] = bv[m];
    }
    const float* wf = a.wx + (size_t)(pos * KT + ct) * 256 + lane;
#pragma unroll
    for (int s = 0; s < (NS ? NS : 4); ++s) {
        if constexpr (NS != 0) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[s * 64], x[s], acc, 0, 0, 0);
        else if (s < ns) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[s * 64], hh ? x[2 * s + 1] : x[2 * s], acc, 0, 0, 0);
    }
}

// The forward.  NS = 0: the input stride is a.stride, read at run time.  NS > 0 (KT = 4, the only width the LSTM classes use): a compile-time
// constant of the whole body, the kernel below branches on it once (what this bought the LEM forward: lem_wide_train_kernel.hip).
template <int KT, int NS>
__device__ __forceinline__ void lstm_forward(const LstmTrainArgs& a, u32x4* xf) {
    constexpr int WP = 32 * KT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int ct = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5, W = a.width, stride = NS ? 2 * NS : a.stride, ns = stride >> 1;
    const size_t plane = (size_t)a.n_nodes * a.t_len * WP;
    const __amdgpu_buffer_rsrc_t stream = lwt_stream<KT>(a.rec, ct);
    const long n = (long)blockIdx.x * 32 + c;
    const bool live = n < a.n_nodes;
    const long nc = live ? n : a.n_nodes - 1;
    const bool save = live && a.saved != nullptr;
    const float* xrow = a.xin + (size_t)nc * a.t_len * stride + (NS ? hh : 0);
    float* srow = a.saved + (size_t)nc * a.t_len * WP + 4 * hh;

    f32x16 h, cs, ig, acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) { h[r] = 0.f; cs[r] = 0.f; }
    if (a.h0) lwt_dense_load(a.h0 + (size_t)nc * W, ct, hh, W, h);
    if (a.c0) lwt_dense_load(a.c0 + (size_t)nc * W, ct, hh, W, cs);
    lwt_publish(xf, ct, lane, h);
    LwtFrag wA, wB;
    unsigned loff = 16u * lane;
    asm volatile("" : "+v"(loff));
    lwt_frag_load(wA, stream, 0, loff);
    __syncthreads();

    for (int t = 0; t < a.t_len; ++t) {
        float x[NS ? NS : 8];
#pragma unroll
        for (int f = 0; f < (NS ? NS : 8); ++f) {
            if constexpr (NS != 0) x[f] = xrow[(size_t)t * stride + 2 * f];
            else x[f] = f < stride ? xrow[(size_t)t * stride + f] : 0.f;
        }
        float* st = srow + (size_t)t * WP;
        int wlane = lane;       // NS > 0: the input-column fragments are loaded where they are used, not held for the whole loop (as in the LEM forward)
        if constexpr (NS != 0) asm volatile("" : "+v"(wlane));

        if (save) lwt_tile_store(st + LST_H * plane, ct, h);         // h_{t-1}, the state ENTERING the step (published)
        lstm_tile_init<KT, NS>(a, 0, ct, wlane, hh, ns, x, ig);           // i
        lwt_gemm<KT, 0>(wA, wB, stream, xf, lane, loff, ig);
#pragma unroll
        for (int r = 0; r < 16; ++r) ig[r] = sigmoidf_(ig[r]);
        if (save) lwt_tile_store(st + LST_I * plane, ct, ig);
        lstm_tile_init<KT, NS>(a, 1, ct, wlane, hh, ns, x, acc);          // g -> i g
        lwt_gemm<KT, 1>(wA, wB, stream, xf, lane, loff, acc);
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = tanhf_(acc[r]);
        if (save) lwt_tile_store(st + LST_G * plane, ct, acc);
#pragma unroll
        for (int r = 0; r < 16; ++r) ig[r] *= acc[r];
        lstm_tile_init<KT, NS>(a, 2, ct, wlane, hh, ns, x, acc);          // f -> c'
        lwt_gemm<KT, 2>(wA, wB, stream, xf, lane, loff, acc);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[r] = sigmoidf_(acc[r]);
            cs[r] = acc[r] * cs[r] + ig[r];
        }
        if (save) {
            lwt_tile_store(st + LST_F * plane, ct, acc);
            lwt_tile_store(st + LST_C * plane, ct, cs);
        }
        lstm_tile_init<KT, NS>(a, 3, ct, wlane, hh, ns, x, acc);          // o -> h'
        lwt_gemm<KT, 3>(wA, wB, stream, xf, lane, loff, acc);
        __syncthreads();                                             // every wave has read the last fragment of h
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[r] = sigmoidf_(acc[r]);
            h[r] = acc[r] * tanhf_(cs[r]);
        }
        if (save) lwt_tile_store(st + LST_O * plane, ct, acc);
        lwt_publish(xf, ct, lane, h);
        __syncthreads();
    }
    if (live) {
        lwt_dense_store(a.h_out + (size_t)n * W, ct, hh, W, h);
        if (a.c_out) lwt_dense_store(a.c_out + (size_t)n * W, ct, hh, W, cs);
    }
}

template <int KT>
__global__ __launch_bounds__(64 * KT) void lstm_train_fwd_kernel(LstmTrainArgs a) {
    __shared__ u32x4 xf[KT * LWT_KTILE_U4];                          // 6 KT KB: h
    if constexpr (KT == 4) {
        switch (a.stride >> 1) {
            case 1: lstm_forward<KT, 1>(a, xf); break;
            case 2: lstm_forward<KT, 2>(a, xf); break;
            case 3: lstm_forward<KT, 3>(a, xf); break;
            default: lstm_forward<KT, 4>(a, xf); break;
        }
    } else {
        lstm_forward<KT, 0>(a, xf);
    }
}

struct LstmBwdArgs {
    const float* gout;      // [N, W] dL/dh_T
    const float* saved;     // [6][N][T][Wp]
    long n_nodes;
    int t_len, width, ldg;
    const float* rec_t;
    float* dg;              // [N][T][4][ldg]
    const float* c0;        // the forward's initial c [N, W] (NULL = zeros); h0 is in the saved h plane
};

// one gate gradient: written to dG, published, and dh += W_hh[gate]^T p (stream position POS)
template <int KT, int POS>
__device__ __forceinline__ void lstm_bwd_gate_product(LwtFrag& wA, LwtFrag& wB, __amdgpu_buffer_rsrc_t stream, u32x4* xf, int ct, int lane, unsigned loff, bool live,
                                                      float* gt_gate, const f32x16& p, f32x16& dh) {
    if (live) lwt_tile_store(gt_gate, ct, p);
    lwt_publish(xf, ct, lane, p);                // the area is free: the previous product ended with a barrier
    __syncthreads();
    lwt_gemm<KT, POS>(wA, wB, stream, xf, lane, loff, dh);
    __syncthreads();
}

template <int KT>
__global__ __launch_bounds__(64 * KT) void lstm_bptt_kernel(LstmBwdArgs a) {
    constexpr int WP = 32 * KT;
    __shared__ u32x4 xf[KT * LWT_KTILE_U4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int ct = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5, W = a.width, ldg = a.ldg;
    const size_t plane = (size_t)a.n_nodes * a.t_len * WP;
    const __amdgpu_buffer_rsrc_t stream = lwt_stream<KT>(a.rec_t, ct);
    const long n = (long)blockIdx.x * 32 + c;
    const bool live = n < a.n_nodes;
    const long nc = live ? n : a.n_nodes - 1;
    const float* srow = a.saved + (size_t)nc * a.t_len * WP + 4 * hh;
    float* grow = a.dg + (size_t)nc * a.t_len * (4 * ldg) + 4 * hh;
    f32x16 dh, dc, p, q;
    lwt_dense_load(a.gout + (size_t)nc * W, ct, hh, W, dh);
#pragma unroll
    for (int r = 0; r < 16; ++r) dc[r] = 0.f;
    LwtFrag wA, wB;
    unsigned loff = 16u * lane;
    asm volatile("" : "+v"(loff));
    lwt_frag_load(wA, stream, 0, loff);

    for (int t = a.t_len - 1; t >= 0; --t) {
        const float* st = srow + (size_t)t * WP;
        float* gt = grow + (size_t)t * (4 * ldg);
        {   // h' = o tanh(c'):  p = dG_o, dc += dh o (1 - th^2); dh is consumed here and rebuilt by the four products
            f32x16 o, cc;
            lwt_tile_load(st + LST_O * plane, ct, o);
            lwt_tile_load(st + LST_C * plane, ct, cc);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float th = tanhf_(cc[r]), gr = dh[r];
                p[r] = gr * th * o[r] * (1.0f - o[r]);
                dc[r] += gr * o[r] * (1.0f - th * th);
                dh[r] = 0.f;
            }
        }
        if (live) {
            // columns Wp .. ldg - 1 of all four gates: zeros (the weight-gradient jobs read whole 128-column blocks)
            f32x16 zero;
#pragma unroll
            for (int r = 0; r < 16; ++r) zero[r] = 0.f;
            for (int T2 = KT + ct; T2 < (ldg >> 5); T2 += KT)
#pragma unroll
                for (int gi = 0; gi < 4; ++gi) lwt_tile_store(gt + gi * ldg, T2, zero);
        }
        lstm_bwd_gate_product<KT, 0>(wA, wB, stream, xf, ct, lane, loff, live, gt + LST_O * ldg, p, dh);
        {   // c' = f c + i g:  p = dG_i, q = dG_g
            f32x16 gi, gg;
            lwt_tile_load(st + LST_I * plane, ct, gi);
            lwt_tile_load(st + LST_G * plane, ct, gg);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                p[r] = dc[r] * gg[r] * gi[r] * (1.0f - gi[r]);
                q[r] = dc[r] * gi[r] * (1.0f - gg[r] * gg[r]);
            }
        }
        lstm_bwd_gate_product<KT, 1>(wA, wB, stream, xf, ct, lane, loff, live, gt + LST_I * ldg, p, dh);
        lstm_bwd_gate_product<KT, 2>(wA, wB, stream, xf, ct, lane, loff, live, gt + LST_G * ldg, q, dh);
        {   // p = dG_f, dc <- dc f
            f32x16 f, cp;
            lwt_tile_load(st + LST_F * plane, ct, f);
            if (t > 0) lwt_tile_load(st - WP + LST_C * plane, ct, cp);
            else if (a.c0) lwt_dense_load(a.c0 + (size_t)nc * W, ct, hh, W, cp);
            else {
#pragma unroll
                for (int r = 0; r < 16; ++r) cp[r] = 0.f;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                p[r] = dc[r] * cp[r] * f[r] * (1.0f - f[r]);
                dc[r] *= f[r];
            }
        }
        lstm_bwd_gate_product<KT, 3>(wA, wB, stream, xf, ct, lane, loff, live, gt + LST_F * ldg, p, dh);
    }
}

}  // namespace msmp

using namespace msmp;

static bool lstm_train_shape_ok(const char* who, int ninp, int width) {
    if (!wide_width_ok(who, width)) return false;
    if (ninp < 1 || ninp > LEM_MAX_INP) {
        set_error("%s: ninp=%d outside 1..%d", who, ninp, LEM_MAX_INP);
        return false;
    }
    return true;
}
static bool lstm_sizes_ok(const char* who, int64_t n_nodes, int t_len, int width) {
    if (!wide_width_ok(who, width)) return false;
    if (n_nodes < 0 || n_nodes >= (1L << 31) || t_len < 1) {
        set_error("%s: bad sizes", who);
        return false;
    }
    return true;
}
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int64_t msmp_packed_lstm_train_floats(int ninp, int width) {
    if (!lstm_train_shape_ok("msmp_packed_lstm_train_floats", ninp, width)) return 0;
    return lstm_train_layout((width + 31) / 32).total;
}

extern "C" int64_t msmp_packed_lstm_bwd_floats(int ninp, int width) {
    if (!lstm_train_shape_ok("msmp_packed_lstm_bwd_floats", ninp, width)) return 0;
    return lstm_bwd_floats((width + 31) / 32);
}

extern "C" int64_t msmp_lstm_saved_floats(int64_t n_nodes, int t_len, int width) {
    if (!lstm_sizes_ok("msmp_lstm_saved_floats", n_nodes, t_len, width)) return 0;
    return (int64_t)LST_PLANES * n_nodes * t_len * (32 * ((width + 31) / 32));
}

extern "C" int64_t msmp_lstm_dg_floats(int64_t n_nodes, int t_len, int width) {
    if (!lstm_sizes_ok("msmp_lstm_dg_floats", n_nodes, t_len, width)) return 0;
    return (int64_t)4 * n_nodes * t_len * (128 * ((width + 127) / 128));
}

extern "C" int msmp_pack_lstm_train_f32(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int ninp, int width,
                                        float* packed_out, msmp_stream_t stream) {
    if (!lstm_train_shape_ok("msmp_pack_lstm_train_f32", ninp, width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(w_ih && w_hh && b_ih && b_hh && packed_out, MSMP_ERR_ARG, "msmp_pack_lstm_train_f32: null pointer");
    MSMP_REQUIRE(aligned16(packed_out), MSMP_ERR_ARG, "msmp_pack_lstm_train_f32: packed_out is not 16-byte aligned");
    LstmTrainPackArgs a{w_ih, w_hh, b_ih, b_hh, ninp, width, (width + 31) / 32, packed_out};
    hipLaunchKernelGGL(pack_lstm_train_kernel<false>, dim3(2 * a.kt * a.kt), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("pack_lstm_train_kernel");
}

extern "C" int msmp_pack_lstm_bwd_f32(const float* w_hh, int ninp, int width, float* packed_out, msmp_stream_t stream) {
    if (!lstm_train_shape_ok("msmp_pack_lstm_bwd_f32", ninp, width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(w_hh && packed_out, MSMP_ERR_ARG, "msmp_pack_lstm_bwd_f32: null pointer");
    MSMP_REQUIRE(aligned16(packed_out), MSMP_ERR_ARG, "msmp_pack_lstm_bwd_f32: packed_out is not 16-byte aligned");
    LstmTrainPackArgs a{nullptr, w_hh, nullptr, nullptr, ninp, width, (width + 31) / 32, packed_out};
    hipLaunchKernelGGL(pack_lstm_train_kernel<true>, dim3(2 * a.kt * a.kt), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("pack_lstm_train_kernel");
}

extern "C" int msmp_lstm_train_fwd_f32(const float* xin, int64_t n_nodes, int t_len, int ninp, int width, const float* packed, const float* h0,
                                       const float* c0, float* saved, float* h_out, float* c_out, msmp_stream_t stream) {
    if (!lstm_train_shape_ok("msmp_lstm_train_fwd_f32", ninp, width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(t_len >= 1, MSMP_ERR_ARG, "msmp_lstm_train_fwd_f32: t_len=%d < 1", t_len);
    MSMP_REQUIRE(n_nodes >= 0 && n_nodes < (1L << 31), MSMP_ERR_ARG, "msmp_lstm_train_fwd_f32: bad n_nodes");
    MSMP_REQUIRE(xin && packed && h_out, MSMP_ERR_ARG, "msmp_lstm_train_fwd_f32: null pointer");
    MSMP_REQUIRE((h0 == nullptr) == (c0 == nullptr), MSMP_ERR_ARG, "msmp_lstm_train_fwd_f32: give both initial states or none");
    MSMP_REQUIRE(aligned16(packed) && aligned16(saved), MSMP_ERR_ARG, "msmp_lstm_train_fwd_f32: packed / saved not 16-byte aligned");
    if (n_nodes == 0) return MSMP_OK;
    const int kt = (width + 31) / 32;
    const LstmTrainLayout L = lstm_train_layout(kt);
    LstmTrainArgs a{xin, (long)n_nodes, t_len, msmp_lem_input_stride(ninp), width, packed + L.rec, packed + L.wx, packed + L.bias,
                    saved, h0, c0, h_out, c_out};
    const unsigned grid = (unsigned)((n_nodes + 31) / 32);
    hipStream_t st = (hipStream_t)stream;
    dispatch_kt(kt, [&](auto K) {
        constexpr int KT = decltype(K)::value;
        hipLaunchKernelGGL((lstm_train_fwd_kernel<KT>), dim3(grid), dim3(64 * KT), 0, st, a);
    });
    return check_launch("lstm_train_fwd_kernel");
}

extern "C" int msmp_lstm_train_bwd_f32(const float* grad_h, const float* saved, const float* c0, int64_t n_nodes, int t_len, int width,
                                       const float* packed_bwd, float* dg_out, msmp_stream_t stream) {
    if (!wide_width_ok("msmp_lstm_train_bwd_f32", width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(t_len >= 1, MSMP_ERR_ARG, "msmp_lstm_train_bwd_f32: t_len=%d < 1", t_len);
    MSMP_REQUIRE(n_nodes >= 0 && n_nodes < (1L << 31), MSMP_ERR_ARG, "msmp_lstm_train_bwd_f32: bad n_nodes");
    MSMP_REQUIRE(grad_h && saved && packed_bwd && dg_out, MSMP_ERR_ARG, "msmp_lstm_train_bwd_f32: null pointer");
    MSMP_REQUIRE(aligned16(packed_bwd) && aligned16(saved) && aligned16(dg_out), MSMP_ERR_ARG,
                 "msmp_lstm_train_bwd_f32: packed_bwd / saved / dg_out not 16-byte aligned");
    if (n_nodes == 0) return MSMP_OK;
    const int kt = (width + 31) / 32;
    LstmBwdArgs a{grad_h, saved, (long)n_nodes, t_len, width, 128 * ((width + 127) / 128), packed_bwd, dg_out, c0};
    const unsigned grid = (unsigned)((n_nodes + 31) / 32);
    hipStream_t st = (hipStream_t)stream;
    dispatch_kt(kt, [&](auto K) {
        constexpr int KT = decltype(K)::value;
        hipLaunchKernelGGL((lstm_bptt_kernel<KT>), dim3(grid), dim3(64 * KT), 0, st, a);
    });
    return check_launch("lstm_bptt_kernel");
}
