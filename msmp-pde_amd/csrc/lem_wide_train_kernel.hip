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
// Workgroup shape: one 32-node tile per workgroup, 64 KT threads, KT = ceil(W / 32); wave ct owns channel tile ct (32 of the Wp = 32 KT
// channels) of every carried tensor, in accumulator layout (one node per lane), for all T steps.  A GEMM needs all Wp channels of its B
// operand (y, z' forward; dg1, dl, dg2, dg3 backward): the operand tensor is PUBLISHED in LDS as bf16 hi / mid / lo MFMA fragments in "acc
// order" (K step s of k-tile kt of a lane is registers 8 s .. 8 s + 7 of wave kt's accumulator tile, so a publish is a register split + three
// 16-byte stores, no transposition; 6 KB per k-tile, 6 KT KB per tensor; ONE area, reused between barriers), and every wave multiplies its own
// 32 rows of the weight block -- bf16x3 A fragments streamed from the L2-resident blob through buffer loads, one k-tile (6 KB per wave) ahead,
// nothing staged: a wave needs only ITS 32 rows -- with all published fragments: six v_mfma_f32_32x32x16_bf16 per K = 16 step, fp32-exact
// products (mfma_tiles.h).  No fp16 anywhere, so there is no input range and the kernels neither read nor raise the range status.  Barriers
// per step: 4 forward, 8 backward.  (The first edition, 128 wide only: v_mfma_f32_32x32x2_f32 with every 16-KB weight chunk staged through
// LDS, 19 barriers and 256 KB of staging per time step; this shape cut the matrix time per node 2.7x.)
// Node tiles per workgroup: two (64 nodes, 228 / 247 registers at width 128, two workgroups per CU) halve the weight-fragment traffic but
// measured the same as one (three workgroups per CU): 30.3 vs 30.0 ms per batch-512 training iteration.  At width 128 the backward holds 180
// registers (two workgroups per CU) and takes the time of a 163-register edition with three (profiles/r19a_one_lem_training_pair.md).
// Channels W .. Wp - 1 carry zero weights, zero bias and zero state: their z and y stay exact zeros, their dG is an exact zero, and they are
// never written to y_out / z_out.  A node's arithmetic depends on nothing but its own row.
//
// Memory layouts (all fp32):
//   saved  [6][N][T][Wp]            planes a2, c, a1, d, y_{t-1}, z'; every element is written (pad channels: dt / 2 in a1, a2; 0 elsewhere)
//   dG     [N][T][4][ldg]           ldg = 128 ceil(W / 128); gate order g1, g2, g3, lin; columns W .. ldg - 1 are written as 0
#include "lem_layout.h"
#include "train_frags.h"      // the tile, publish, fragment-stream and product pieces (shared with mlp_train_kernel.hip)

namespace msmp {

enum { LWT_A2 = 0, LWT_C = 1, LWT_A1 = 2, LWT_D = 3, LWT_Y = 4, LWT_Z = 5, LWT_PLANES = 6 };

// forward blob (floats), kt = ceil(W / 32), Wp = 32 kt:
//   rec  [wave ct kt][gate 4: g2, g3, g1, lin][k-tile kc kt][s 2][plane 3: hi, mid, lo][lane 64][8 bf16]: rows 32 ct .. of the gate's recurrent
//        block, columns 32 kc .., as bf16x3 A fragments in acc order (split_k_acc); a wave's stream of one time step is contiguous |
//   wx   [gate 4][ct kt][s 4][lane 64]: the input columns as v_mfma_f32_32x32x2_f32 A fragments, W_gate[32 ct + (lane & 31)][W + 2 s + (lane >> 5)] |
//   bias [gate 4][Wp]
// zero outside the matrices.
struct LemWideTrainLayout {
    int64_t rec, wx, bias, total;
};
__host__ __device__ inline LemWideTrainLayout lem_wide_train_layout(int kt) {
    LemWideTrainLayout L;
    L.rec = 0;
    L.wx = L.rec + (int64_t)4 * kt * kt * LWT_KTILE_FLOATS;
    L.bias = L.wx + (int64_t)4 * kt * 256;
    L.total = L.bias + (int64_t)4 * kt * 32;
    return L;
}
// backward blob (floats): rec_t [wave ct kt][gate 4: g1, lin, g2, g3 (consumption order)][k-tile kc kt][s 2][plane 3][lane 64][8 bf16]:
//   fragment row 32 ct + m, column 32 kc + kk  =  M_gate[32 kc + kk][32 ct + m], M the gate's recurrent block: the TRANSPOSED blocks
__host__ __device__ inline int64_t lem_wide_bwd_floats(int kt) { return (int64_t)4 * kt * kt * LWT_KTILE_FLOATS; }

struct LemWideTrainPackArgs {
    const float *w, *wz, *b, *bz;
    int ninp, width, kt;
    float* out;
};

// recurrent / input weight of `row` (< W) of forward gate g (0 g2, 1 g3, 2 g1, 3 lin), column col.  ONE load from a selected matrix and
// first row: as a chain of four conditional loads the wx loop below was compiled into divergent blocks in which the lanes of gate 3 reached
// the load with neither the matrix nor the row assigned (read in the gfx950 assembly: a wild address, the kernel faulted on first use).
__device__ __forceinline__ float lwt_weight(const LemWideTrainPackArgs& a, int g, int row, int col) {
    const int kin = a.width + a.ninp;
    const float* m = g == 3 ? a.wz : a.w;
    const int first = g == 0 ? a.width : g == 1 ? 2 * a.width : 0;
    return m[(size_t)(first + row) * kin + col];
}
__device__ __forceinline__ float lwt_bias(const LemWideTrainPackArgs& a, int g, int row) {
    const float* m = g == 3 ? a.bz : a.b;
    const int first = g == 0 ? a.width : g == 1 ? 2 * a.width : 0;
    return m[first + row];
}


// TRANSPOSED = false: the forward blob; true: the backward blob (a.b / a.bz unused).  One thread per (ct, gate, kc, s, lane).
template <bool TRANSPOSED>
__global__ __launch_bounds__(256) void pack_lem_wide_train_kernel(LemWideTrainPackArgs a) {
    const int kt = a.kt, W = a.width;
    const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t n_rec = (int64_t)4 * kt * kt * 2 * 64;
    for (int64_t p = tid0; p < n_rec; p += stride) {
        const int lane = (int)(p & 63), s = (int)(p >> 6) & 1;
        const int64_t q = p >> 7;
        const int kc = (int)(q % kt), g = (int)((q / kt) & 3), ct = (int)(q / (4 * kt));
        const int row = 32 * ct + (lane & 31);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 32 * kc + split_k_acc(s, lane >> 5, j);
            if (row >= W || k >= W) v[j] = 0.f;
            else if (!TRANSPOSED) v[j] = lwt_weight(a, g, row, k);
            else v[j] = lwt_weight(a, g == 0 ? 2 : g == 1 ? 3 : g == 2 ? 0 : 1, k, row);      // g1, lin, g2, g3 in forward numbering
        }
        lwt_store_b3(a.out, p >> 6, lane, v);
    }
    if (TRANSPOSED) return;
    const LemWideTrainLayout L = lem_wide_train_layout(kt);
    for (int64_t p = tid0; p < (int64_t)4 * kt * 256; p += stride) {
        const int lane = (int)(p & 63), s = (int)(p >> 6) & 3, ct = (int)((p >> 8) % kt), g = (int)((p >> 8) / kt);
        const int row = 32 * ct + (lane & 31), f = 2 * s + (lane >> 5);
        a.out[L.wx + p] = row < W && f < a.ninp ? lwt_weight(a, g, row, W + f) : 0.f;
    }
    for (int64_t p = tid0; p < (int64_t)4 * kt * 32; p += stride) {
        const int row = (int)(p % (32 * kt)), g = (int)(p / (32 * kt));
        a.out[L.bias + p] = row < W ? lwt_bias(a, g, row) : 0.f;
    }
}

struct LemWideTrainArgs {
    const float* xin;       // [N, T, stride]
    long n_nodes;
    int t_len, stride, width;
    float dt;
    const float *rec, *wx, *bias;
    float* saved;           // [6][N][T][Wp] or NULL
    const float *y0, *z0;   // [N, W] or NULL (zeros)
    float *y_out, *z_out;   // [N, W]; z_out may be NULL
};

// acc (tile ct) = bias + W[:, W : W + ninp] x_t: the input columns as ceil(ninp / 2) fp32 MFMA k-steps (the pad of an odd ninp is zero).
// NS > 0: that many steps, x[s] = feature 2 s + hh of the lane's node.  NS = 0: `ns` steps, x[f] = feature f (zero past the stride).
template <int KT, int NS>
__device__ __forceinline__ void lwt_tile_init(const LemWideTrainArgs& a, int g, int ct, int lane, int hh, int ns, const float (&x)[NS ? NS : 8], f32x16& acc) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(a.bias + (g * KT + ct) * 32 + 8 * q + 4 * hh);
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[4 * q + m] = bv[m];
    }
    const float* wf = a.wx + (size_t)(g * KT + ct) * 256 + lane;
#pragma unroll
    for (int s = 0; s < (NS ? NS : 4); ++s) {
        if constexpr (NS != 0) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[s * 64], x[s], acc, 0, 0, 0);
        else if (s < ns) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[s * 64], hh ? x[2 * s + 1] : x[2 * s], acc, 0, 0, 0);
    }
}

// The forward.  NS = 0: the input stride is a.stride, read at run time.  NS > 0 (KT = 4, the flagship width, only): it is a compile-time
// constant of the whole body and the kernel below branches on it once.  At run time the step-input loads and the input-column MFMAs of every
// step sit behind branches, which at width 128 cost the forward 5 % (51 200 nodes) to 13 % (1 600 nodes) against the retired 128-wide kernel,
// whose NS was a template argument too (profiles/r19a_one_lem_training_pair.md).  The other KT keep the run-time body: with four bodies per
// kernel they would hold 167 - 176 registers instead of 149 - 160 and lose a workgroup per CU.
template <int KT, int NS>
__device__ __forceinline__ void lwt_forward(const LemWideTrainArgs& a, u32x4* xf) {
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

    f32x16 y, z, g, acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) { y[r] = 0.f; z[r] = 0.f; }
    if (a.y0) lwt_dense_load(a.y0 + (size_t)nc * W, ct, hh, W, y);
    if (a.z0) lwt_dense_load(a.z0 + (size_t)nc * W, ct, hh, W, z);
    lwt_publish(xf, ct, lane, y);
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
        // NS > 0: the input-column fragments are the same in every step; read through an offset the compiler cannot see through, they are
        // loaded where they are used (L1 hits) instead of being held in 4 NS registers for the whole loop: a body alone needs at most 164
        // registers, not 176, and the kernel of the four bodies 168, which is three workgroups per CU instead of two (with two, the forward
        // with saving of 51 200 nodes took 1.74 ms, not 1.63)
        int wlane = lane;
        if constexpr (NS != 0) asm volatile("" : "+v"(wlane));

        if (save) lwt_tile_store(st + LWT_Y * plane, ct, y);        // y_{t-1}, the state ENTERING the step
        lwt_tile_init<KT, NS>(a, 0, ct, wlane, hh, ns, x, g);             // g2 -> a2            (published: y)
        lwt_gemm<KT, 0>(wA, wB, stream, xf, lane, loff, g);
#pragma unroll
        for (int r = 0; r < 16; ++r) g[r] = a.dt * sigmoidf_(g[r]);
        if (save) lwt_tile_store(st + LWT_A2 * plane, ct, g);
        lwt_tile_init<KT, NS>(a, 1, ct, wlane, hh, ns, x, acc);           // g3 -> c, z'
        lwt_gemm<KT, 1>(wA, wB, stream, xf, lane, loff, acc);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[r] = tanhf_(acc[r]);
            z[r] = (1.0f - g[r]) * z[r] + g[r] * acc[r];
        }
        if (save) {
            lwt_tile_store(st + LWT_C * plane, ct, acc);
            lwt_tile_store(st + LWT_Z * plane, ct, z);
        }
        lwt_tile_init<KT, NS>(a, 2, ct, wlane, hh, ns, x, g);             // g1 -> a1
        lwt_gemm<KT, 2>(wA, wB, stream, xf, lane, loff, g);
        __syncthreads();                                             // every wave has read the last fragment of y
#pragma unroll
        for (int r = 0; r < 16; ++r) g[r] = a.dt * sigmoidf_(g[r]);
        if (save) lwt_tile_store(st + LWT_A1 * plane, ct, g);
        lwt_publish(xf, ct, lane, z);
        lwt_tile_init<KT, NS>(a, 3, ct, wlane, hh, ns, x, acc);           // lin -> d, y'        (published: z')
        __syncthreads();
        lwt_gemm<KT, 3>(wA, wB, stream, xf, lane, loff, acc);
        __syncthreads();                                             // every wave has read the last fragment of z'
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            acc[r] = tanhf_(acc[r]);
            y[r] = (1.0f - g[r]) * y[r] + g[r] * acc[r];
        }
        if (save) lwt_tile_store(st + LWT_D * plane, ct, acc);
        lwt_publish(xf, ct, lane, y);
        __syncthreads();
    }
    if (live) {
        lwt_dense_store(a.y_out + (size_t)n * W, ct, hh, W, y);
        if (a.z_out) lwt_dense_store(a.z_out + (size_t)n * W, ct, hh, W, z);
    }
}

template <int KT>
__global__ __launch_bounds__(64 * KT) void lem_wide_train_fwd_kernel(LemWideTrainArgs a) {
    __shared__ u32x4 xf[KT * LWT_KTILE_U4];                          // 6 KT KB: y, then z', alternately
    if constexpr (KT == 4) {
        switch (a.stride >> 1) {
            case 1: lwt_forward<KT, 1>(a, xf); break;
            case 2: lwt_forward<KT, 2>(a, xf); break;
            case 3: lwt_forward<KT, 3>(a, xf); break;
            default: lwt_forward<KT, 4>(a, xf); break;
        }
    } else {
        lwt_forward<KT, 0>(a, xf);
    }
}

struct LemWideBwdArgs {
    const float* gout;      // [N, W] dL/dy_T
    const float* saved;     // [6][N][T][Wp]
    long n_nodes;
    int t_len, width, ldg;
    float dt;
    const float* rec_t;
    float* dg;              // [N][T][4][ldg]
    const float* z0;        // the forward's initial z [N, W] (NULL = zeros); y0 is in the saved y plane
};

template <int KT>
__global__ __launch_bounds__(64 * KT) void lem_wide_bptt_kernel(LemWideBwdArgs a) {
    constexpr int WP = 32 * KT;
    __shared__ u32x4 xf[KT * LWT_KTILE_U4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int ct = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5, W = a.width, ldg = a.ldg;
    const size_t plane = (size_t)a.n_nodes * a.t_len * WP;
    const __amdgpu_buffer_rsrc_t stream = lwt_stream<KT>(a.rec_t, ct);
    const float inv_dt = 1.0f / a.dt;
    const long n = (long)blockIdx.x * 32 + c;
    const bool live = n < a.n_nodes;
    const long nc = live ? n : a.n_nodes - 1;
    const float* srow = a.saved + (size_t)nc * a.t_len * WP + 4 * hh;
    float* grow = a.dg + (size_t)nc * a.t_len * (4 * ldg) + 4 * hh;
    f32x16 dy, dz, p, q;
    lwt_dense_load(a.gout + (size_t)nc * W, ct, hh, W, dy);
#pragma unroll
    for (int r = 0; r < 16; ++r) dz[r] = 0.f;
    LwtFrag wA, wB;
    unsigned loff = 16u * lane;
    asm volatile("" : "+v"(loff));
    lwt_frag_load(wA, stream, 0, loff);

    for (int t = a.t_len - 1; t >= 0; --t) {
        const float* st = srow + (size_t)t * WP;
        float* gt = grow + (size_t)t * (4 * ldg);
        {   // y' = (1-a1) y + a1 d:  p = dg1, q = dl
            f32x16 a1, d, yp;
            lwt_tile_load(st + LWT_A1 * plane, ct, a1);
            lwt_tile_load(st + LWT_D * plane, ct, d);
            lwt_tile_load(st + LWT_Y * plane, ct, yp);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float gr = dy[r];
                q[r] = gr * a1[r] * (1.0f - d[r] * d[r]);
                p[r] = gr * (d[r] - yp[r]) * a1[r] * (1.0f - a1[r] * inv_dt);
                dy[r] = gr * (1.0f - a1[r]);
            }
        }
        if (live) {
            lwt_tile_store(gt, ct, p);
            lwt_tile_store(gt + 3 * ldg, ct, q);
            // columns Wp .. ldg - 1 of all four gates: zeros (the weight-gradient jobs read whole 128-column blocks)
            f32x16 zero;
#pragma unroll
            for (int r = 0; r < 16; ++r) zero[r] = 0.f;
            for (int T2 = KT + ct; T2 < (ldg >> 5); T2 += KT)
#pragma unroll
                for (int gi = 0; gi < 4; ++gi) lwt_tile_store(gt + gi * ldg, T2, zero);
        }
        lwt_publish(xf, ct, lane, p);            // the area is free: the previous GEMM ended with a barrier
        __syncthreads();
        lwt_gemm<KT, 0>(wA, wB, stream, xf, lane, loff, dy);         // dy += W_g1^T dg1
        __syncthreads();
        lwt_publish(xf, ct, lane, q);
        __syncthreads();
        lwt_gemm<KT, 1>(wA, wB, stream, xf, lane, loff, dz);         // dz += Wz^T dl
        __syncthreads();
        {   // z' = (1-a2) z + a2 c:  p = dg2, q = dg3
            f32x16 a2, cc, zp;
            lwt_tile_load(st + LWT_A2 * plane, ct, a2);
            lwt_tile_load(st + LWT_C * plane, ct, cc);
            if (t > 0) lwt_tile_load(st - WP + LWT_Z * plane, ct, zp);
            else if (a.z0) lwt_dense_load(a.z0 + (size_t)nc * W, ct, hh, W, zp);
            else {
#pragma unroll
                for (int r = 0; r < 16; ++r) zp[r] = 0.f;
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float gr = dz[r];
                q[r] = gr * a2[r] * (1.0f - cc[r] * cc[r]);
                p[r] = gr * (cc[r] - zp[r]) * a2[r] * (1.0f - a2[r] * inv_dt);
                dz[r] = gr * (1.0f - a2[r]);
            }
        }
        if (live) {
            lwt_tile_store(gt + ldg, ct, p);
            lwt_tile_store(gt + 2 * ldg, ct, q);
        }
        lwt_publish(xf, ct, lane, p);
        __syncthreads();
        lwt_gemm<KT, 2>(wA, wB, stream, xf, lane, loff, dy);         // dy += W_g2^T dg2
        __syncthreads();
        lwt_publish(xf, ct, lane, q);
        __syncthreads();
        lwt_gemm<KT, 3>(wA, wB, stream, xf, lane, loff, dy);         // dy += W_g3^T dg3
        __syncthreads();
    }
}

}  // namespace msmp

using namespace msmp;

static bool lem_wide_train_shape_ok(const char* who, int ninp, int width) {
    if (!wide_width_ok(who, width)) return false;
    if (ninp < 1 || ninp > LEM_MAX_INP) {
        set_error("%s: ninp=%d outside 1..%d", who, ninp, LEM_MAX_INP);
        return false;
    }
    return true;
}
static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

extern "C" int64_t msmp_packed_lem_wide_train_floats(int ninp, int width) {
    if (!lem_wide_train_shape_ok("msmp_packed_lem_wide_train_floats", ninp, width)) return 0;
    return lem_wide_train_layout((width + 31) / 32).total;
}

extern "C" int64_t msmp_packed_lem_wide_bwd_floats(int ninp, int width) {
    if (!lem_wide_train_shape_ok("msmp_packed_lem_wide_bwd_floats", ninp, width)) return 0;
    return lem_wide_bwd_floats((width + 31) / 32);
}

extern "C" int64_t msmp_lem_wide_saved_floats(int64_t n_nodes, int t_len, int width) {
    if (!wide_width_ok("msmp_lem_wide_saved_floats", width)) return 0;
    if (n_nodes < 0 || n_nodes >= (1L << 31) || t_len < 1) {
        set_error("msmp_lem_wide_saved_floats: bad sizes");
        return 0;
    }
    return (int64_t)LWT_PLANES * n_nodes * t_len * (32 * ((width + 31) / 32));
}

extern "C" int64_t msmp_lem_wide_dg_floats(int64_t n_nodes, int t_len, int width) {
    if (!wide_width_ok("msmp_lem_wide_dg_floats", width)) return 0;
    if (n_nodes < 0 || n_nodes >= (1L << 31) || t_len < 1) {
        set_error("msmp_lem_wide_dg_floats: bad sizes");
        return 0;
    }
    return (int64_t)4 * n_nodes * t_len * (128 * ((width + 127) / 128));
}

extern "C" int msmp_pack_lem_wide_train_f32(const float* weights, const float* weights_lin_z, const float* bias, const float* bias_lin_z,
                                            int ninp, int width, float* packed_out, msmp_stream_t stream) {
    if (!lem_wide_train_shape_ok("msmp_pack_lem_wide_train_f32", ninp, width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(weights && weights_lin_z && bias && bias_lin_z && packed_out, MSMP_ERR_ARG, "msmp_pack_lem_wide_train_f32: null pointer");
    MSMP_REQUIRE(aligned16(packed_out), MSMP_ERR_ARG, "msmp_pack_lem_wide_train_f32: packed_out is not 16-byte aligned");
    LemWideTrainPackArgs a{weights, weights_lin_z, bias, bias_lin_z, ninp, width, (width + 31) / 32, packed_out};
    hipLaunchKernelGGL(pack_lem_wide_train_kernel<false>, dim3(2 * a.kt * a.kt), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("pack_lem_wide_train_kernel");
}

extern "C" int msmp_pack_lem_wide_bwd_f32(const float* weights, const float* weights_lin_z, int ninp, int width, float* packed_out,
                                          msmp_stream_t stream) {
    if (!lem_wide_train_shape_ok("msmp_pack_lem_wide_bwd_f32", ninp, width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(weights && weights_lin_z && packed_out, MSMP_ERR_ARG, "msmp_pack_lem_wide_bwd_f32: null pointer");
    MSMP_REQUIRE(aligned16(packed_out), MSMP_ERR_ARG, "msmp_pack_lem_wide_bwd_f32: packed_out is not 16-byte aligned");
    LemWideTrainPackArgs a{weights, weights_lin_z, nullptr, nullptr, ninp, width, (width + 31) / 32, packed_out};
    hipLaunchKernelGGL(pack_lem_wide_train_kernel<true>, dim3(2 * a.kt * a.kt), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("pack_lem_wide_train_kernel");
}

extern "C" int msmp_lem_train_fwd_wide_f32(const float* xin, int64_t n_nodes, int t_len, int ninp, int width, float dt, const float* packed,
                                           const float* y0, const float* z0, float* saved, float* y_out, float* z_out, msmp_stream_t stream) {
    if (!lem_wide_train_shape_ok("msmp_lem_train_fwd_wide_f32", ninp, width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(t_len >= 1, MSMP_ERR_ARG, "msmp_lem_train_fwd_wide_f32: t_len=%d < 1", t_len);
    MSMP_REQUIRE(n_nodes >= 0 && n_nodes < (1L << 31), MSMP_ERR_ARG, "msmp_lem_train_fwd_wide_f32: bad n_nodes");
    MSMP_REQUIRE(xin && packed && y_out, MSMP_ERR_ARG, "msmp_lem_train_fwd_wide_f32: null pointer");
    MSMP_REQUIRE((y0 == nullptr) == (z0 == nullptr), MSMP_ERR_ARG, "msmp_lem_train_fwd_wide_f32: give both initial states or none");
    MSMP_REQUIRE(aligned16(packed) && aligned16(saved), MSMP_ERR_ARG, "msmp_lem_train_fwd_wide_f32: packed / saved not 16-byte aligned");
    if (n_nodes == 0) return MSMP_OK;
    const int kt = (width + 31) / 32;
    const LemWideTrainLayout L = lem_wide_train_layout(kt);
    LemWideTrainArgs a{xin, (long)n_nodes, t_len, msmp_lem_input_stride(ninp), width, dt, packed + L.rec, packed + L.wx, packed + L.bias,
                       saved, y0, z0, y_out, z_out};
    const unsigned grid = (unsigned)((n_nodes + 31) / 32);
    hipStream_t st = (hipStream_t)stream;
    dispatch_kt(kt, [&](auto K) {
        constexpr int KT = decltype(K)::value;
        hipLaunchKernelGGL((lem_wide_train_fwd_kernel<KT>), dim3(grid), dim3(64 * KT), 0, st, a);
    });
    return check_launch("lem_wide_train_fwd_kernel");
}

extern "C" int msmp_lem_train_bwd_wide_f32(const float* grad_y, const float* saved, const float* y0, const float* z0, int64_t n_nodes, int t_len,
                                           int width, float dt, const float* packed_bwd, float* dg_out, msmp_stream_t stream) {
    if (!wide_width_ok("msmp_lem_train_bwd_wide_f32", width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(t_len >= 1 && dt != 0.f, MSMP_ERR_ARG, "msmp_lem_train_bwd_wide_f32: t_len=%d < 1 or dt = 0", t_len);
    MSMP_REQUIRE(n_nodes >= 0 && n_nodes < (1L << 31), MSMP_ERR_ARG, "msmp_lem_train_bwd_wide_f32: bad n_nodes");
    MSMP_REQUIRE(grad_y && saved && packed_bwd && dg_out, MSMP_ERR_ARG, "msmp_lem_train_bwd_wide_f32: null pointer");
    MSMP_REQUIRE((y0 == nullptr) == (z0 == nullptr), MSMP_ERR_ARG, "msmp_lem_train_bwd_wide_f32: give both initial states or none");
    MSMP_REQUIRE(aligned16(packed_bwd) && aligned16(saved) && aligned16(dg_out), MSMP_ERR_ARG,
                 "msmp_lem_train_bwd_wide_f32: packed_bwd / saved / dg_out not 16-byte aligned");
    if (n_nodes == 0) return MSMP_OK;
    const int kt = (width + 31) / 32;
    LemWideBwdArgs a{grad_y, saved, (long)n_nodes, t_len, width, 128 * ((width + 127) / 128), dt, packed_bwd, dg_out, z0};
    const unsigned grid = (unsigned)((n_nodes + 31) / 32);
    hipStream_t st = (hipStream_t)stream;
    dispatch_kt(kt, [&](auto K) {
        constexpr int KT = decltype(K)::value;
        hipLaunchKernelGGL((lem_wide_bptt_kernel<KT>), dim3(grid), dim3(64 * KT), 0, st, a);
    });
    return check_launch("lem_wide_bptt_kernel");
}
