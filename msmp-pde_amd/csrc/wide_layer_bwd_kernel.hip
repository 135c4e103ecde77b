// msmp_wide_layer_bwd_f32: the backward of one GNN_LayerLin / one gated pair of them at any hidden width up to 256 (the GLU classes:
// 164; experiments/models_gnn.py:88-149, 1486-1489) behind one C-ABI call -- the `_wide` counterpart of msmp_mp_layer_bwd_f32, in its
// factorised form only.
//
// The layer is evaluated in PADDED coordinates: every [rows, width] tensor has the row stride ld = 128 ceil(width / 128) with zero
// padding columns, and every weight matrix is copied once per call into a zero-padded [ld, .] matrix (wide_bwd_pad_weights_kernel).  A
// width-164 layer is then exactly a width-256 layer whose extra channels are dead: their pre-activations, activations and gradients
// are 0, so nothing below needs a column bound, every access is a 16-byte piece of a 512- or 1024-byte row, and the gradients of the real
// parameters are the leading [width, .] blocks of the padded ones (wide_bwd_assemble_kernel).
//
//   recompute   F = [h | u pos vars | 0] [N, ldf];  P = F Wp^T + b1, Q = F Wq^T (row GEMMs, 128-column output groups);
//               a1 = P[tgt] + Q[src], m1 = Swish(a1);  a2 = m1 W2^T + b2;  agg = CSR mean of Swish(a2);
//               cat_n = [h | agg | vars | 0];  a3 = cat_n W3^T + b3, u1 = Swish(a3);  upd = u1 W4^T + b4
//   gradients   blend / InstanceNorm backward per graph -> d upd;  d a3 = (d upd W4) Swish'(a3);  dh (+)= d a3 W3[:, h],
//               dagg = d a3 W3[:, agg];  d a2 = dagg[tgt] / deg Swish'(a2) (over a2);  x1 = d a2 W2;
//               S_t / S_s = x1 Swish'(a1) summed over each node's in- / out-edges in a fixed order;  dh += S_t Wp[:, h] + S_s Wq[:, h]
//   parameters  S_t^T F, S_s^T F, d a2^T m1, d a3^T cat_n, d upd^T u1 through the weight-gradient kernel of grad_weights_kernel.hip (A in
//               128-column groups, B in column slices of at most 319), reassembled by ONE launch for all sixteen gradients.
// Row GEMMs and the weight split are those of rows_gemm_kernel.hip (rows_gemm.h), the weight-gradient launcher that of
// grad_weights_kernel.hip (grad_weights.h); the kernels of this file are everything between them.  No atomics, no memset, fixed summation orders: two calls on the same inputs give the same bits.
#include <vector>

#include "grad_weights.h"
#include "graph_norm.h"
#include "rows_gemm.h"
#include "wide_frags.h"

namespace msmp {

constexpr int WB_MAX_SLICE = 319;          // columns of B one weight-gradient job takes
constexpr int WB_JOBS_PER_CALL = 8;

// ---- zero-padded copies of one head's parameters ------------------------------------------------------------------------------------
//   wp [ld, ldf] = [W1[:, 0:W] | 0 | W1[:, 2W : 2W + T] | 0],   wq [ld, ldf] = [W1[:, W:2W] | 0 | -W1[:, 2W : 2W + tw + 1] | 0]   (T = tw + 1 + nv)
//   w2, w4 [ld, ld];   w3 [ld, ld_n] = [W3[:, 0:W] | 0 | W3[:, W:2W] | 0 | W3[:, 2W : 2W + nv] | 0];   bias [4, ld] = b1 .. b4
struct WbPrepArgs {
    const float* p[2][8];
    float *wp[2], *wq[2], *w2[2], *w3[2], *w4[2], *bias[2];
    int W, ld, ldf, ld_n, tw, nv;
};
__global__ __launch_bounds__(256) void wide_bwd_pad_weights_kernel(WbPrepArgs a) {
    const int hd = blockIdx.y, W = a.W, ld = a.ld, ldf = a.ldf, ld_n = a.ld_n;
    const int T = a.tw + 1 + a.nv, kmsg = 2 * W + T, kupd = 2 * W + a.nv;
    const long n_pq = (long)ld * ldf, n_sq = (long)ld * ld, n_w3 = (long)ld * ld_n, total = n_pq + 2 * n_sq + n_w3 + 4 * ld;
    const float* const* p = a.p[hd];
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        long r = i;
        if (r < n_pq) {
            const int o = (int)(r / ldf), k = (int)(r - (long)o * ldf);
            float vp = 0.f, vq = 0.f;
            if (o < W) {
                const float* row = p[0] + (size_t)o * kmsg;
                if (k < ld) {
                    if (k < W) { vp = row[k]; vq = row[W + k]; }
                } else if (k - ld < T) {
                    vp = row[2 * W + (k - ld)];
                    if (k - ld < a.tw + 1) vq = -vp;
                }
            }
            a.wp[hd][r] = vp;
            a.wq[hd][r] = vq;
            continue;
        }
        r -= n_pq;
        if (r < 2 * n_sq) {
            const bool second = r >= n_sq;
            if (second) r -= n_sq;
            const int o = (int)(r / ld), k = (int)(r - (long)o * ld);
            const float v = (o < W && k < W) ? p[second ? 6 : 2][(size_t)o * W + k] : 0.f;
            (second ? a.w4[hd] : a.w2[hd])[r] = v;
            continue;
        }
        r -= 2 * n_sq;
        if (r < n_w3) {
            const int o = (int)(r / ld_n), k = (int)(r - (long)o * ld_n);
            float v = 0.f;
            if (o < W) {
                const float* row = p[4] + (size_t)o * kupd;
                if (k < ld) { if (k < W) v = row[k]; }
                else if (k < 2 * ld) { if (k - ld < W) v = row[W + (k - ld)]; }
                else if (k - 2 * ld < a.nv) v = row[2 * W + (k - 2 * ld)];
            }
            a.w3[hd][r] = v;
            continue;
        }
        r -= n_w3;
        const int b = (int)(r / ld), o = (int)(r - (long)b * ld);
        a.bias[hd][r] = o < W ? p[1 + 2 * b][o] : 0.f;
    }
}

// ---- glue on [rows, ld] tensors: thread = (row, 16-byte channel group), g4 = ld / 4 = 1 << sh groups per row -------------------------

// F[n] = [h[n] (ld columns) | u[n] | pos[n] | vars[n] | 0]   (row stride ldf)
__global__ __launch_bounds__(256) void wide_bwd_node_feat_kernel(const float* __restrict__ h, const float* __restrict__ u, const float* __restrict__ pos,
                                                                 const float* __restrict__ vars, long n_nodes, int tw, int nv, int ld, int ldf,
                                                                 float* __restrict__ out) {
    const int f4 = ldf / 4, g4 = ld / 4;
    const long total = n_nodes * f4;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
        const long n = p / f4;
        const int g = (int)(p - n * f4);
        f32x4 v;
        if (g < g4) v = reinterpret_cast<const f32x4*>(h)[(size_t)n * g4 + g];
        else {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int k = 4 * (g - g4) + m;
                v[m] = k < tw ? u[(size_t)n * tw + k] : (k == tw ? pos[n] : (k <= tw + nv ? vars[(size_t)n * nv + (k - tw - 1)] : 0.f));
            }
        }
        reinterpret_cast<f32x4*>(out)[p] = v;
    }
}

// a1[e] = P[tgt[e]] + Q[src[e]],  m1[e] = Swish(a1[e])
__global__ __launch_bounds__(256) void wide_bwd_gather_swish_kernel(const float* __restrict__ P, const float* __restrict__ Q, const int* __restrict__ tgt,
                                                                    const int* __restrict__ src, long n_edges, int sh, float* __restrict__ a1,
                                                                    float* __restrict__ m1) {
    const long total = n_edges << sh;
    const int mask = (1 << sh) - 1;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
        const long e = p >> sh;
        const int cg = (int)(p & mask);
        const f32x4 v = reinterpret_cast<const f32x4*>(P)[((size_t)tgt[e] << sh) + cg] + reinterpret_cast<const f32x4*>(Q)[((size_t)src[e] << sh) + cg];
        f32x4 s;
#pragma unroll
        for (int m = 0; m < 4; ++m) s[m] = swishf(v[m]);
        reinterpret_cast<f32x4*>(a1)[p] = v;
        reinterpret_cast<f32x4*>(m1)[p] = s;
    }
}

// agg[n] = mean over the CSR row of n of Swish(a2[e])   (fixed order; a node without in-edges gets 0)
__global__ __launch_bounds__(256) void wide_bwd_swish_mean_kernel(const float* __restrict__ a2, const int* __restrict__ rowptr, long n_nodes, int sh,
                                                                  float* __restrict__ agg) {
    const long total = n_nodes << sh;
    const int mask = (1 << sh) - 1;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
        const long n = p >> sh;
        const int cg = (int)(p & mask);
        const int r0 = rowptr[n], r1 = rowptr[n + 1];
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int e = r0; e < r1; ++e) {
            const f32x4 v = reinterpret_cast<const f32x4*>(a2)[((size_t)e << sh) + cg];
#pragma unroll
            for (int m = 0; m < 4; ++m) s[m] += swishf(v[m]);
        }
        reinterpret_cast<f32x4*>(agg)[p] = s * (1.0f / (float)max(r1 - r0, 1));
    }
}

// cat_n[n] = [h[n] (ld) | agg[n] (ld) | vars[n] | 0]   (row stride ld_n = 2 ld + 8)
__global__ __launch_bounds__(256) void wide_bwd_cat_node_kernel(const float* __restrict__ h, const float* __restrict__ agg, const float* __restrict__ vars,
                                                                long n_nodes, int nv, int ld, float* __restrict__ out) {
    const int g4 = ld / 4, c4 = 2 * g4 + 2;
    const long total = n_nodes * c4;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
        const long n = p / c4;
        const int g = (int)(p - n * c4);
        f32x4 v;
        if (g < g4) v = reinterpret_cast<const f32x4*>(h)[(size_t)n * g4 + g];
        else if (g < 2 * g4) v = reinterpret_cast<const f32x4*>(agg)[(size_t)n * g4 + (g - g4)];
        else {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int k = 4 * (g - 2 * g4) + m;
                v[m] = k < nv ? vars[(size_t)n * nv + k] : 0.f;
            }
        }
        reinterpret_cast<f32x4*>(out)[p] = v;
    }
}

// out = Swish(x)
__global__ __launch_bounds__(256) void wide_bwd_swish_kernel(const float* __restrict__ x, long n4, float* __restrict__ out) {
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < n4; p += (long)gridDim.x * 256) {
        const f32x4 v = reinterpret_cast<const f32x4*>(x)[p];
        f32x4 r;
#pragma unroll
        for (int m = 0; m < 4; ++m) r[m] = swishf(v[m]);
        reinterpret_cast<f32x4*>(out)[p] = r;
    }
}

// g *= Swish'(a)   (in place)
__global__ __launch_bounds__(256) void wide_bwd_dswish_mul_kernel(float* __restrict__ g, const float* __restrict__ a, long n4) {
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < n4; p += (long)gridDim.x * 256) {
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[p], av = reinterpret_cast<const f32x4*>(a)[p];
        f32x4 r;
#pragma unroll
        for (int m = 0; m < 4; ++m) r[m] = gv[m] * dswish(av[m]);
        reinterpret_cast<f32x4*>(g)[p] = r;
    }
}

// a2[e] <- dagg[tgt[e]] / max(deg, 1) * Swish'(a2[e])   (the gradient takes the place of the pre-activation it is the gradient of)
__global__ __launch_bounds__(256) void wide_bwd_mean_bwd_dswish_kernel(const float* __restrict__ dagg, const int* __restrict__ rowptr,
                                                                       const int* __restrict__ tgt, long n_edges, int sh, float* __restrict__ a2) {
    const long total = n_edges << sh;
    const int mask = (1 << sh) - 1;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
        const long e = p >> sh;
        const int cg = (int)(p & mask), i = tgt[e];
        const float inv = 1.0f / (float)max(rowptr[i + 1] - rowptr[i], 1);
        const f32x4 g = reinterpret_cast<const f32x4*>(dagg)[((size_t)i << sh) + cg];
        const f32x4 a = reinterpret_cast<const f32x4*>(a2)[p];
        f32x4 r;
#pragma unroll
        for (int m = 0; m < 4; ++m) r[m] = g[m] * inv * dswish(a[m]);
        reinterpret_cast<f32x4*>(a2)[p] = r;
    }
}

// The two segmented sums of d a1 = x1 Swish'(a1):  blockIdx.y = 0: S_t[n] over the in-edges of n (its CSR row, ascending),
// blockIdx.y = 1: S_s[n] over its out-edges (src_rowptr / src_perm: CSR edge ids, ascending inside a source).  d a1 itself is never stored.
__global__ __launch_bounds__(256) void wide_bwd_segsum_kernel(const float* __restrict__ x1, const float* __restrict__ a1, const int* __restrict__ rowptr,
                                                              const int* __restrict__ src_rowptr, const int* __restrict__ src_perm, long n_nodes,
                                                              int sh, float* __restrict__ s_t, float* __restrict__ s_s) {
    const long total = n_nodes << sh;
    const int mask = (1 << sh) - 1;
    const bool by_src = blockIdx.y != 0;
    const int* __restrict__ rp = by_src ? src_rowptr : rowptr;
    float* __restrict__ out = by_src ? s_s : s_t;
    for (long p = (long)blockIdx.x * 256 + threadIdx.x; p < total; p += (long)gridDim.x * 256) {
        const long n = p >> sh;
        const int cg = (int)(p & mask);
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int k = rp[n]; k < rp[n + 1]; ++k) {
            const size_t o = ((size_t)(by_src ? src_perm[k] : k) << sh) + cg;
            const f32x4 g = reinterpret_cast<const f32x4*>(x1)[o], a = reinterpret_cast<const f32x4*>(a1)[o];
#pragma unroll
            for (int m = 0; m < 4; ++m) s[m] += g[m] * dswish(a[m]);
        }
        reinterpret_cast<f32x4*>(out)[p] = s;
    }
}

// ---- per graph: InstanceNorm backward, alone or under the gated blend; grid = (graphs, ld / 128), thread = (channel group, row slice)
__device__ __forceinline__ void wide_bwd_stats(const f32x4* __restrict__ x, int n0, int n1, int g4, int col, int cg, int rs, f32x4* red, float eps,
                                               f32x4& mean, f32x4& rstd) {
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    for (int r = n0 + rs; r < n1; r += 8) s += x[(size_t)r * g4 + col];
    const float inv = 1.0f / (float)max(n1 - n0, 1);
    mean = block_colsum(s, red, cg, rs) * inv;
    f32x4 q = {0.f, 0.f, 0.f, 0.f};
    for (int r = n0 + rs; r < n1; r += 8) {
        const f32x4 d = x[(size_t)r * g4 + col] - mean;
        q += d * d;
    }
    const f32x4 var = block_colsum(q, red, cg, rs) * inv;
#pragma unroll
    for (int m = 0; m < 4; ++m) rstd[m] = 1.0f / sqrtf(var[m] + eps);
}

// y = (x - mean) rstd per graph and channel:  dx = rstd (g - mean_graph(g) - y mean_graph(g y))
__global__ __launch_bounds__(256) void wide_bwd_norm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g, const int* __restrict__ graph_ptr,
                                                                int g4, float eps, float* __restrict__ dx) {
    __shared__ f32x4 red[256];
    const int cg = threadIdx.x & 31, rs = threadIdx.x >> 5, col = blockIdx.y * 32 + cg;
    const int n0 = graph_ptr[blockIdx.x], n1 = graph_ptr[blockIdx.x + 1];
    const f32x4* xp = reinterpret_cast<const f32x4*>(x);
    const f32x4* gp = reinterpret_cast<const f32x4*>(g);
    f32x4 mean, rstd;
    wide_bwd_stats(xp, n0, n1, g4, col, cg, rs, red, eps, mean, rstd);
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
    for (int r = n0 + rs; r < n1; r += 8) {
        const size_t o = (size_t)r * g4 + col;
        s += gp[o];
        q += gp[o] * ((xp[o] - mean) * rstd);
    }
    const float inv = 1.0f / (float)max(n1 - n0, 1);
    s = block_colsum(s, red, cg, rs) * inv;
    q = block_colsum(q, red, cg, rs) * inv;
    for (int r = n0 + rs; r < n1; r += 8) {
        const size_t o = (size_t)r * g4 + col;
        const f32x4 y = (xp[o] - mean) * rstd;
        reinterpret_cast<f32x4*>(dx)[o] = rstd * (gp[o] - s - y * q);
    }
}

// out = (1 - tau) h + tau s,  tau = sigmoid(IN(gate_pre)),  s = Swish(IN(main_pre)):
//   d IN(gate) = g (s - h) tau (1 - tau);  d IN(main) = g tau Swish'(IN(main));  dh = g (1 - tau);  then both InstanceNorm backwards
__device__ __forceinline__ void wide_bwd_blend_grads(f32x4 g, f32x4 hv, f32x4 yg, f32x4 ym, f32x4& dyg, f32x4& dym, f32x4& dh) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const float tau = sigmoidf_(yg[m]);
        dyg[m] = g[m] * (swishf(ym[m]) - hv[m]) * tau * (1.0f - tau);
        dym[m] = g[m] * tau * dswish(ym[m]);
        dh[m] = g[m] * (1.0f - tau);
    }
}
__global__ __launch_bounds__(256) void wide_bwd_blend_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ h, const float* __restrict__ gate,
                                                                 const float* __restrict__ mainp, const int* __restrict__ graph_ptr, int g4, float eps,
                                                                 float* __restrict__ d_gate, float* __restrict__ d_main, float* __restrict__ dh_out) {
    __shared__ f32x4 red[256];
    const int cg = threadIdx.x & 31, rs = threadIdx.x >> 5, col = blockIdx.y * 32 + cg;
    const int n0 = graph_ptr[blockIdx.x], n1 = graph_ptr[blockIdx.x + 1];
    const f32x4* gp = reinterpret_cast<const f32x4*>(gout);
    const f32x4* hp = reinterpret_cast<const f32x4*>(h);
    const f32x4* tp = reinterpret_cast<const f32x4*>(gate);
    const f32x4* mp = reinterpret_cast<const f32x4*>(mainp);
    f32x4 gm, gr, mm, mr;
    wide_bwd_stats(tp, n0, n1, g4, col, cg, rs, red, eps, gm, gr);
    wide_bwd_stats(mp, n0, n1, g4, col, cg, rs, red, eps, mm, mr);
    f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sgy = sg, sm = sg, smy = sg;
    for (int r = n0 + rs; r < n1; r += 8) {
        const size_t o = (size_t)r * g4 + col;
        const f32x4 yg = (tp[o] - gm) * gr, ym = (mp[o] - mm) * mr;
        f32x4 dyg, dym, dh;
        wide_bwd_blend_grads(gp[o], hp[o], yg, ym, dyg, dym, dh);
        sg += dyg; sgy += dyg * yg; sm += dym; smy += dym * ym;
    }
    const float inv = 1.0f / (float)max(n1 - n0, 1);
    sg = block_colsum(sg, red, cg, rs) * inv;
    sgy = block_colsum(sgy, red, cg, rs) * inv;
    sm = block_colsum(sm, red, cg, rs) * inv;
    smy = block_colsum(smy, red, cg, rs) * inv;
    for (int r = n0 + rs; r < n1; r += 8) {
        const size_t o = (size_t)r * g4 + col;
        const f32x4 yg = (tp[o] - gm) * gr, ym = (mp[o] - mm) * mr;
        f32x4 dyg, dym, dh;
        wide_bwd_blend_grads(gp[o], hp[o], yg, ym, dyg, dym, dh);
        reinterpret_cast<f32x4*>(d_gate)[o] = gr * (dyg - sg - yg * sgy);
        reinterpret_cast<f32x4*>(d_main)[o] = mr * (dym - sm - ym * smy);
        reinterpret_cast<f32x4*>(dh_out)[o] = dh;
    }
}

// ---- the sixteen (eight) parameter gradients from the weight-gradient kernel's blocks ---------------------------------------------------
// A product A^T B (A [rows, ld], B [rows, k]) is computed as blocks (g, s): rows 128 g .. + 127 of the result, columns s ws .. of it, each a
// dense [128, k2_s] matrix (k2_s = min(ws, k - s ws)) at blk + (g n_s + s) 128 ws, its column sums of A at bias + (g n_s + s) 128.
struct WbProd {
    float *blk, *bias;
    int k, ws, n_s;
};
__device__ __forceinline__ float wb_at(const WbProd& m, int o, int c) {
    const int g = o >> 7, s = c / m.ws, k2 = min(m.ws, m.k - s * m.ws);
    return m.blk[((size_t)(g * m.n_s + s) * 128 + (o & 127)) * m.ws - (size_t)(o & 127) * (m.ws - k2) + (c - s * m.ws)];
}
struct WbAsmArgs {
    WbProd prod[2][5];       // per head: S_t^T F, S_s^T F, d a2^T m1, d a3^T cat_n, d upd^T u1
    float* grad[2][8];
    int W, ld, tw, nv, has_edges;
};
// grid = (blocks, 8 gradients, heads)
__global__ __launch_bounds__(256) void wide_bwd_assemble_kernel(WbAsmArgs a) {
    const int hd = blockIdx.z, which = blockIdx.y, W = a.W, ld = a.ld;
    const int T = a.tw + 1 + a.nv, kmsg = 2 * W + T, kupd = 2 * W + a.nv;
    const WbProd* m = a.prod[hd];
    float* __restrict__ out = a.grad[hd][which];
    const int cols = which == 0 ? kmsg : which == 4 ? kupd : (which & 1) ? 1 : W;
    const int total = W * cols;
    for (int p = blockIdx.x * 256 + threadIdx.x; p < total; p += gridDim.x * 256) {
        const int o = p / cols, k = p - o * cols;
        float v = 0.f;
        if (which < 4 && !a.has_edges) v = 0.f;          // no edges: the message layers get zero gradients
        else if (which == 0) {                            // dW1[:, h_i | h_j | tail] from S_t^T F and S_s^T F (Q's u, pos columns are negated)
            if (k < W) v = wb_at(m[0], o, k);
            else if (k < 2 * W) v = wb_at(m[1], o, k - W);
            else {
                const int j = k - 2 * W;
                v = wb_at(m[0], o, ld + j);
                if (j < a.tw + 1) v -= wb_at(m[1], o, ld + j);
            }
        } else if (which == 4) v = wb_at(m[3], o, k < W ? k : k < 2 * W ? ld + (k - W) : 2 * ld + (k - 2 * W));
        else if (which == 2) v = wb_at(m[2], o, k);
        else if (which == 6) v = wb_at(m[4], o, k);
        else {                                            // biases: column sums of S_t, d a2, d a3, d upd
            const WbProd& b = m[which == 1 ? 0 : which == 3 ? 2 : which == 5 ? 3 : 4];
            v = b.bias[(size_t)((o >> 7) * b.n_s) * 128 + (o & 127)];
        }
        out[p] = v;
    }
}

// ---- host: sizes, workspace plan, orchestration -------------------------------------------------------------------------------------
struct WbDims {
    long n, e;
    int W, G, ld, sh, tw, nv, T, ldf, ld_n, Kw, heads;
};
static WbDims wb_dims(long n, long e, int tw, int nv, int width, int gated) {
    WbDims d;
    d.n = n; d.e = e; d.W = width; d.G = (width + 127) / 128; d.ld = 128 * d.G; d.sh = d.G == 1 ? 5 : 6;
    d.tw = tw; d.nv = nv; d.T = tw + 1 + nv; d.ldf = d.ld + 32 * ((d.T + 31) / 32); d.ld_n = 2 * d.ld + 8;
    d.Kw = 32 * ((width + 31) / 32);       // reduction length of the W-wide operands: the padding beyond it is zero on both sides
    d.heads = gated ? 2 : 1;
    return d;
}

struct WbHead {
    float *wp, *wq, *w2, *w3, *w4, *bias;                                  // zero-padded parameters
    u32x4 *f_wp[2], *f_wq[2], *f_w2[2], *f_w3[2], *f_w4[2];                // forward forms, one per 128-channel output group
    u32x4 *f_w4t[2], *f_w3t[4], *f_w2t[2], *f_w1ti[2], *f_w1tj[2];         // data-gradient forms
    float *a1, *m1, *a2;                                                   // [E, ld]
    float *cat_n, *a3, *u1, *upd, *dupd, *da3, *st, *ss;                   // [N, ld_n], 7 x [N, ld]
    WbProd prod[5];
};
struct WbPlan {
    WbHead hd[2];
    float *feat, *P, *Q, *agg, *dagg, *x1, *gw;      // shared by the heads: [N, ldf], 4 x [N, ld], [E, ld], the weight-gradient partials
    int64_t gw_floats;
    size_t bytes;
};
struct WbJob {
    const float *a, *b;
    int64_t rows;
    int ldb, k2;
    float *w, *bias;
};

struct WbCarver {
    uintptr_t base;
    size_t off = 0;
    template <class T>
    T* take(size_t count) {
        T* r = reinterpret_cast<T*>(base + off);
        off += (count * sizeof(T) + 255) & ~(size_t)255;
        return r;
    }
};

static void wb_jobs(const WbDims& d, const WbPlan& pl, std::vector<WbJob>& jobs) {
    for (int h = 0; h < d.heads; ++h) {
        const WbHead& b = pl.hd[h];
        const float* A[5] = {b.st, b.ss, b.a2, b.da3, b.dupd};
        const float* B[5] = {pl.feat, pl.feat, b.m1, b.cat_n, b.u1};
        const int ldb[5] = {d.ldf, d.ldf, d.ld, d.ld_n, d.ld};
        for (int i = d.e ? 0 : 3; i < 5; ++i) {
            const WbProd& m = b.prod[i];
            for (int g = 0; g < d.G; ++g)
                for (int s = 0; s < m.n_s; ++s) {
                    const int k2 = m.ws < m.k - s * m.ws ? m.ws : m.k - s * m.ws;
                    const size_t blk = (size_t)(g * m.n_s + s) * 128;
                    jobs.push_back({A[i] + 128 * g, B[i] + s * m.ws, i == 2 ? d.e : d.n, ldb[i], k2, m.blk + blk * m.ws, m.bias + blk});
                }
        }
    }
}

// every buffer of the call at its offset from `base` (0 for the size query); false where the weight-gradient kernel refuses a job
static bool wb_plan(const WbDims& d, uintptr_t base, WbPlan& pl) {
    WbCarver c{base};
    const size_t n = d.n, e = d.e, ld = d.ld;
    const int cw = d.Kw / 32, cf = d.ldf / 32, c3 = (d.ld_n + 31) / 32;
    pl.feat = c.take<float>(n * d.ldf);
    pl.P = c.take<float>(n * ld); pl.Q = c.take<float>(n * ld); pl.agg = c.take<float>(n * ld); pl.dagg = c.take<float>(n * ld);
    pl.x1 = c.take<float>(e * ld);
    for (int h = 0; h < d.heads; ++h) {
        WbHead& b = pl.hd[h];
        b.wp = c.take<float>(ld * d.ldf); b.wq = c.take<float>(ld * d.ldf); b.w2 = c.take<float>(ld * ld); b.w3 = c.take<float>(ld * d.ld_n);
        b.w4 = c.take<float>(ld * ld); b.bias = c.take<float>(4 * ld);
        auto frag = [&](int chunks) { return c.take<u32x4>((size_t)chunks * RG_CHUNK_U4); };
        for (int g = 0; g < d.G; ++g) {
            b.f_wp[g] = frag(cf); b.f_wq[g] = frag(cf); b.f_w2[g] = frag(cw); b.f_w3[g] = frag(c3); b.f_w4[g] = frag(cw);
            b.f_w4t[g] = frag(cw); b.f_w3t[g] = frag(cw); b.f_w3t[d.G + g] = frag(cw); b.f_w2t[g] = frag(cw); b.f_w1ti[g] = frag(cw); b.f_w1tj[g] = frag(cw);
        }
        b.a1 = c.take<float>(e * ld); b.m1 = c.take<float>(e * ld); b.a2 = c.take<float>(e * ld);
        b.cat_n = c.take<float>(n * d.ld_n);
        b.a3 = c.take<float>(n * ld); b.u1 = c.take<float>(n * ld); b.upd = c.take<float>(n * ld); b.dupd = c.take<float>(n * ld);
        b.da3 = c.take<float>(n * ld); b.st = c.take<float>(n * ld); b.ss = c.take<float>(n * ld);
        const int k[5] = {d.ld + d.T, d.ld + d.tw + 1, d.W, 2 * d.ld + d.nv, d.W};
        for (int i = 0; i < 5; ++i) {
            WbProd& m = b.prod[i];
            m.k = k[i];
            m.n_s = (k[i] + WB_MAX_SLICE - 1) / WB_MAX_SLICE;
            m.ws = (k[i] + m.n_s - 1) / m.n_s;
            m.blk = c.take<float>((size_t)d.G * m.n_s * 128 * m.ws);
            m.bias = c.take<float>((size_t)d.G * m.n_s * 128);
        }
    }
    std::vector<WbJob> jobs;
    wb_jobs(d, pl, jobs);
    pl.gw_floats = 0;
    for (size_t j0 = 0; j0 < jobs.size(); j0 += WB_JOBS_PER_CALL) {
        int64_t rows[WB_JOBS_PER_CALL];
        int k2[WB_JOBS_PER_CALL], cnt = 0;
        for (size_t j = j0; j < jobs.size() && cnt < WB_JOBS_PER_CALL; ++j, ++cnt) { rows[cnt] = jobs[j].rows; k2[cnt] = jobs[j].k2; }
        const int64_t need = msmp_grad_weights_workspace_floats(cnt, rows, k2);
        if (need < 0) return false;
        pl.gw_floats = need > pl.gw_floats ? need : pl.gw_floats;
    }
    pl.gw = c.take<float>((size_t)pl.gw_floats);
    pl.bytes = c.off + 256;        // the base is aligned up to 256 bytes
    return true;
}

static bool wb_sizes_ok(int64_t n_nodes, int64_t n_edges, int tw, int nv, int width) {
    return n_nodes > 0 && n_edges >= 0 && n_nodes < (1L << 31) && n_edges < (1L << 31) && tw >= 1 && nv >= 1 && width >= 1 && width <= WIDE_MAX_W &&
           nv <= MSMP_MAX_VARS && tw + 1 + nv <= 128;
}

#define WB_RC(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

// rows_gemm for every 128-channel output group g of a [rows, ld] result
static int wb_gemm(const WbDims& d, int epi, const float* x, int ldx, long rows, int K, u32x4* const* frag, const float* bias, float* out, hipStream_t st) {
    for (int g = 0; g < d.G; ++g) WB_RC(rows_gemm(epi, x, ldx, rows, K, frag[g], bias ? bias + 128 * g : nullptr, nullptr, out + 128 * g, d.ld, nullptr, st));
    return MSMP_OK;
}

struct WbCtx {
    const float *h, *vars;
    const int32_t *rowptr, *col, *tgt, *src_rowptr, *src_perm;
    hipStream_t st;
};

// upd = W4 Swish(W3 [h, mean_j Swish(W2 Swish(P_i + Q_j) + b2), vars] + b3) + b4, keeping the pre-activations
static int wb_recompute(const WbDims& d, const WbCtx& c, const WbPlan& pl, const WbHead& b) {
    const long n = d.n, e = d.e;
    const dim3 blk(256);
    if (e) {
        WB_RC(wb_gemm(d, 1, pl.feat, d.ldf, n, d.ldf, b.f_wp, b.bias, pl.P, c.st));
        WB_RC(wb_gemm(d, 3, pl.feat, d.ldf, n, d.ldf, b.f_wq, nullptr, pl.Q, c.st));
        hipLaunchKernelGGL(wide_bwd_gather_swish_kernel, dim3(grid_for(e << d.sh)), blk, 0, c.st, pl.P, pl.Q, c.tgt, c.col, e, d.sh, b.a1, b.m1);
        WB_RC(wb_gemm(d, 1, b.m1, d.ld, e, d.Kw, b.f_w2, b.bias + d.ld, b.a2, c.st));
    }
    hipLaunchKernelGGL(wide_bwd_swish_mean_kernel, dim3(grid_for(n << d.sh)), blk, 0, c.st, b.a2, c.rowptr, n, d.sh, pl.agg);
    hipLaunchKernelGGL(wide_bwd_cat_node_kernel, dim3(grid_for(n * (d.ld_n / 4))), blk, 0, c.st, c.h, pl.agg, c.vars, n, d.nv, d.ld, b.cat_n);
    WB_RC(wb_gemm(d, 1, b.cat_n, d.ld_n, n, d.ld_n, b.f_w3, b.bias + 2 * d.ld, b.a3, c.st));
    hipLaunchKernelGGL(wide_bwd_swish_kernel, dim3(grid_for(n << d.sh)), blk, 0, c.st, b.a3, n << d.sh, b.u1);
    WB_RC(wb_gemm(d, 1, b.u1, d.ld, n, d.Kw, b.f_w4, b.bias + 3 * d.ld, b.upd, c.st));
    return check_launch("wide layer backward: recompute");
}

// b.dupd = dL/d upd -> dL/dh through this head: written to dh (first) or added to it
static int wb_backward(const WbDims& d, const WbCtx& c, const WbPlan& pl, const WbHead& b, float* dh, bool first) {
    const long n = d.n, e = d.e;
    const dim3 blk(256);
    WB_RC(wb_gemm(d, 3, b.dupd, d.ld, n, d.Kw, b.f_w4t, nullptr, b.da3, c.st));
    hipLaunchKernelGGL(wide_bwd_dswish_mul_kernel, dim3(grid_for(n << d.sh)), blk, 0, c.st, b.da3, b.a3, n << d.sh);                     // d a3
    WB_RC(wb_gemm(d, first ? 3 : 5, b.da3, d.ld, n, d.Kw, b.f_w3t, nullptr, dh, c.st));                                                  // dh (+)= d a3 W3[:, h]
    if (e) {
        WB_RC(wb_gemm(d, 3, b.da3, d.ld, n, d.Kw, b.f_w3t + d.G, nullptr, pl.dagg, c.st));                                               // dagg
        hipLaunchKernelGGL(wide_bwd_mean_bwd_dswish_kernel, dim3(grid_for(e << d.sh)), blk, 0, c.st, pl.dagg, c.rowptr, c.tgt, e, d.sh, b.a2);   // d a2
        WB_RC(wb_gemm(d, 3, b.a2, d.ld, e, d.Kw, b.f_w2t, nullptr, pl.x1, c.st));                                                        // d a2 W2
        hipLaunchKernelGGL(wide_bwd_segsum_kernel, dim3(grid_for(n << d.sh), 2), blk, 0, c.st, pl.x1, b.a1, c.rowptr, c.src_rowptr, c.src_perm, n, d.sh,
                           b.st, b.ss);
        WB_RC(wb_gemm(d, 5, b.st, d.ld, n, d.Kw, b.f_w1ti, nullptr, dh, c.st));                                                          // dh += S_t W1[:, h_i]
        WB_RC(wb_gemm(d, 5, b.ss, d.ld, n, d.Kw, b.f_w1tj, nullptr, dh, c.st));                                                          // dh += S_s W1[:, h_j]
    }
    return check_launch("wide layer backward: data gradients");
}

}  // namespace msmp

using namespace msmp;

extern "C" size_t msmp_wide_layer_bwd_workspace_bytes(int64_t n_nodes, int64_t n_edges, int tw, int nv, int width, int gated) {
    if (!wb_sizes_ok(n_nodes, n_edges, tw, nv, width)) return 0;
    WbPlan pl;
    return wb_plan(wb_dims((long)n_nodes, (long)n_edges, tw, nv, width, gated), 0, pl) ? pl.bytes : 0;
}

extern "C" int msmp_wide_layer_bwd_f32(const float* grad_out, const float* h, const float* u, const float* pos, const float* vars,
                                       const int32_t* rowptr, const int32_t* col, const int32_t* tgt, const int32_t* src_rowptr,
                                       const int32_t* src_perm, const int32_t* graph_ptr, int64_t n_nodes, int64_t n_edges, int64_t n_graphs,
                                       int tw, int nv, int width, int ld, const float* const* params_main, const float* const* params_gate,
                                       float eps, float* dh_out, float* const* grads_main, float* const* grads_gate, void* workspace,
                                       size_t workspace_bytes, msmp_stream_t stream) {
    const char* who = "msmp_wide_layer_bwd_f32";
    MSMP_REQUIRE(grad_out && h && u && pos && vars && rowptr && col && tgt && graph_ptr && params_main && dh_out && grads_main && workspace,
                 MSMP_ERR_ARG, "%s: null pointer", who);
    MSMP_REQUIRE((params_gate != nullptr) == (grads_gate != nullptr), MSMP_ERR_ARG, "%s: give both gate arguments or none", who);
    const bool gated = params_gate != nullptr;
    for (int i = 0; i < 8; ++i) {
        MSMP_REQUIRE(params_main[i] && grads_main[i], MSMP_ERR_ARG, "%s: null parameter / gradient pointer %d", who, i);
        MSMP_REQUIRE(!gated || (params_gate[i] && grads_gate[i]), MSMP_ERR_ARG, "%s: null gate parameter / gradient pointer %d", who, i);
    }
    MSMP_REQUIRE(n_nodes > 0 && n_edges >= 0 && n_graphs > 0 && n_nodes < (1L << 31) && n_edges < (1L << 31) && n_graphs < (1L << 31) && tw >= 1 &&
                 nv >= 1, MSMP_ERR_ARG, "%s: bad sizes", who);
    if (!wide_width_ok(who, width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(nv <= MSMP_MAX_VARS && tw + 1 + nv <= 128, MSMP_ERR_UNSUPPORTED, "%s: nv = %d (up to %d), tw + 1 + nv = %d (up to 128)", who, nv,
                 MSMP_MAX_VARS, tw + 1 + nv);
    MSMP_REQUIRE(n_edges == 0 || (src_rowptr && src_perm), MSMP_ERR_ARG, "%s: src_rowptr / src_perm are required (the by-source sums run in a fixed order)", who);
    const WbDims d = wb_dims((long)n_nodes, (long)n_edges, tw, nv, width, gated);
    MSMP_REQUIRE(ld == d.ld, MSMP_ERR_ARG, "%s: ld = %d, need %d = 128 ceil(width / 128)", who, ld, d.ld);
    MSMP_REQUIRE((((uintptr_t)grad_out | (uintptr_t)h | (uintptr_t)dh_out) & 15) == 0, MSMP_ERR_ARG, "%s: grad_out, h and dh_out must be 16-byte aligned", who);
    WbPlan pl;
    const uintptr_t base = ((uintptr_t)workspace + 255) & ~(uintptr_t)255;
    MSMP_REQUIRE(wb_plan(d, base, pl), MSMP_ERR_UNSUPPORTED, "%s: sizes outside the weight-gradient kernel", who);
    MSMP_REQUIRE(workspace_bytes >= pl.bytes, MSMP_ERR_WORKSPACE, "%s: workspace %zu < %zu", who, workspace_bytes, pl.bytes);
    hipStream_t st = (hipStream_t)stream;
    const dim3 blk(256);

    // the parameters: zero-padded copies, then their bf16x3 fragments (one split launch per head)
    WbPrepArgs pa;
    WbAsmArgs as;
    for (int hd = 0; hd < 2; ++hd) {
        const int s = hd < d.heads ? hd : 0;
        const WbHead& b = pl.hd[s];
        for (int i = 0; i < 8; ++i) {
            pa.p[hd][i] = (s ? params_gate : params_main)[i];
            as.grad[hd][i] = (s ? grads_gate : grads_main)[i];
        }
        pa.wp[hd] = b.wp; pa.wq[hd] = b.wq; pa.w2[hd] = b.w2; pa.w3[hd] = b.w3; pa.w4[hd] = b.w4; pa.bias[hd] = b.bias;
        for (int i = 0; i < 5; ++i) as.prod[hd][i] = b.prod[i];
    }
    pa.W = d.W; pa.ld = d.ld; pa.ldf = d.ldf; pa.ld_n = d.ld_n; pa.tw = tw; pa.nv = nv;
    as.W = d.W; as.ld = d.ld; as.tw = tw; as.nv = nv; as.has_edges = d.e > 0;
    const long n_pad = (long)d.ld * (2 * d.ldf + 2 * d.ld + d.ld_n + 4);
    hipLaunchKernelGGL(wide_bwd_pad_weights_kernel, dim3(grid_for(n_pad), d.heads), blk, 0, st, pa);
    for (int hd = 0; hd < d.heads; ++hd) {
        const WbHead& b = pl.hd[hd];
        RgPackArgs pk;
        pk.n_jobs = 0;
        int blocks = 0;
        for (int g = 0; g < d.G; ++g) {
            const int c0 = 128 * g;
            add_pack(pk, blocks, b.wp, d.ldf, d.ldf, c0, 0, b.f_wp[g]);
            add_pack(pk, blocks, b.wq, d.ldf, d.ldf, c0, 0, b.f_wq[g]);
            add_pack(pk, blocks, b.w2, d.ld, d.Kw, c0, 0, b.f_w2[g]);
            add_pack(pk, blocks, b.w3, d.ld_n, d.ld_n, c0, 0, b.f_w3[g]);
            add_pack(pk, blocks, b.w4, d.ld, d.Kw, c0, 0, b.f_w4[g]);
            add_pack(pk, blocks, b.w4, d.ld, d.Kw, c0, 1, b.f_w4t[g]);
            add_pack(pk, blocks, b.w3, d.ld_n, d.Kw, c0, 1, b.f_w3t[g]);
            add_pack(pk, blocks, b.w3, d.ld_n, d.Kw, d.ld + c0, 1, b.f_w3t[d.G + g]);
            add_pack(pk, blocks, b.w2, d.ld, d.Kw, c0, 1, b.f_w2t[g]);
            add_pack(pk, blocks, b.wp, d.ldf, d.Kw, c0, 1, b.f_w1ti[g]);
            add_pack(pk, blocks, b.wq, d.ldf, d.Kw, c0, 1, b.f_w1tj[g]);
        }
        WB_RC(launch_rg_pack(pk, blocks, st));
    }

    const WbCtx c{h, vars, rowptr, col, tgt, src_rowptr, src_perm, st};
    if (d.e)
        hipLaunchKernelGGL(wide_bwd_node_feat_kernel, dim3(grid_for(d.n * (d.ldf / 4))), blk, 0, st, h, u, pos, vars, d.n, tw, nv, d.ld, d.ldf, pl.feat);
    WB_RC(wb_recompute(d, c, pl, pl.hd[0]));
    const dim3 per_graph((unsigned)n_graphs, (unsigned)d.G);
    if (gated) {
        WB_RC(wb_recompute(d, c, pl, pl.hd[1]));
        hipLaunchKernelGGL(wide_bwd_blend_bwd_kernel, per_graph, blk, 0, st, grad_out, h, pl.hd[1].upd, pl.hd[0].upd, graph_ptr, d.ld / 4, eps,
                           pl.hd[1].dupd, pl.hd[0].dupd, dh_out);
        WB_RC(wb_backward(d, c, pl, pl.hd[0], dh_out, false));
        WB_RC(wb_backward(d, c, pl, pl.hd[1], dh_out, false));
    } else {                                      // out = IN(upd): no direct path to h
        hipLaunchKernelGGL(wide_bwd_norm_bwd_kernel, per_graph, blk, 0, st, pl.hd[0].upd, grad_out, graph_ptr, d.ld / 4, eps, pl.hd[0].dupd);
        WB_RC(wb_backward(d, c, pl, pl.hd[0], dh_out, true));
    }

    std::vector<WbJob> jobs;
    wb_jobs(d, pl, jobs);
    for (size_t j0 = 0; j0 < jobs.size(); j0 += WB_JOBS_PER_CALL) {
        const float *ja[WB_JOBS_PER_CALL], *jb[WB_JOBS_PER_CALL];
        float *jw[WB_JOBS_PER_CALL], *jbias[WB_JOBS_PER_CALL];
        int64_t rows[WB_JOBS_PER_CALL];
        int lda[WB_JOBS_PER_CALL], ldb[WB_JOBS_PER_CALL], k2[WB_JOBS_PER_CALL], cnt = 0;
        for (size_t j = j0; j < jobs.size() && cnt < WB_JOBS_PER_CALL; ++j, ++cnt) {
            ja[cnt] = jobs[j].a; jb[cnt] = jobs[j].b; jw[cnt] = jobs[j].w; jbias[cnt] = jobs[j].bias;
            rows[cnt] = jobs[j].rows; lda[cnt] = d.ld; ldb[cnt] = jobs[j].ldb; k2[cnt] = jobs[j].k2;
        }
        WB_RC(launch_grad_weights(cnt, ja, jb, rows, lda, ldb, k2, jw, jbias, pl.gw, pl.gw_floats, st));
    }
    int max_cols = 2 * d.W + d.T;
    if (2 * d.W + nv > max_cols) max_cols = 2 * d.W + nv;
    hipLaunchKernelGGL(wide_bwd_assemble_kernel, dim3(grid_for((long)d.W * max_cols), 8, (unsigned)d.heads), blk, 0, st, as);
    return check_launch("wide_bwd_assemble_kernel");
}
