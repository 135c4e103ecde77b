// msmp_mp_layer_bwd_f32: the training backward of one width-128 message-passing layer or gated pair behind the C-ABI (the `_bwd` variant of
// msmp_mp_layer_f32); the counterpart of wide_layer_bwd_kernel.hip at the other widths.  One call
// re-evaluates the layer in materialised form, runs the gated-blend / InstanceNorm backward and the data-gradient chain and leaves the
// eight (sixteen) parameter gradients: ~60 launches issued from native code (at the reference's batch of 16 graphs the host was the bound).
//   GEMMs with edge- or node-sized outputs   the own fp32-exact bf16x3 row GEMM (rows_gemm.h) by default; with src_rowptr / src_perm
//                                            message_net_1 is factorised into per-node projections (no [E, kmsg] input, no GEMM on it);
//                                            rocblas_sgemm only under msmp_tune("bwd_gemm") = 0 (kept for A/B runs), looked up at run
//                                            time in the librocblas the process already has: the library is never loaded otherwise
//   weight gradients                         one batched launch pair for all of them (grad_weights.h)
//   everything between the GEMMs             the kernels of this file.  Four of them are C entries of their own, which autograd.py's
//                                            explicit path calls:
//     msmp_edge_concat_f32          the per-edge input of message_net_1 (models_gnn.py:69-75: cat(x_i, x_j, u_i - u_j, pos_i - pos_j, variables_i))
//     msmp_mean_bwd_dswish_f32      backward of aggr='mean' (:42,107) fused with the Swish' of message_net_2
//     msmp_instance_norm_bwd_f32    backward of PyG InstanceNorm (:59,66; affine=False, biased variance)
//     msmp_gate_blend_bwd_f32       backward of the gated blend (:1204-1207) through both InstanceNorms in one launch
// All fp32, HBM-bound, one pass per tensor where the per-graph statistics allow it.
#include <dlfcn.h>
#include <rocblas/rocblas.h>

#include "grad_weights.h"
#include "graph_norm.h"
#include "rows_gemm.h"

namespace msmp {

// one wave per edge: lanes 0..31 copy h[tgt] (16 B each), lanes 32..63 copy h[src]; then the tw + 1 + nv tail columns
__global__ __launch_bounds__(256) void edge_concat_kernel(const float* __restrict__ h, const float* __restrict__ u,
                                                          const float* __restrict__ pos, const float* __restrict__ vars,
                                                          const int* __restrict__ tgt, const int* __restrict__ col, long n_edges,
                                                          int tw, int nv, int ld, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (long)gridDim.x * 4;
    for (long e = wave; e < n_edges; e += n_waves) {
        const int i = tgt[e], j = col[e];
        float* row = out + (size_t)e * ld;
        const int node = lane < 32 ? i : j;
        *reinterpret_cast<f32x4*>(row + 4 * lane) = *reinterpret_cast<const f32x4*>(h + (size_t)node * H + 4 * (lane & 31));
        for (int k = lane; k < tw + 1 + nv; k += 64) {          // tail column k (one pass up to 64 columns, two up to 128)
            if (k < tw) row[2 * H + k] = u[(size_t)i * tw + k] - u[(size_t)j * tw + k];
            else if (k == tw) row[2 * H + tw] = pos[i] - pos[j];
            else row[2 * H + k] = vars[(size_t)i * nv + (k - tw - 1)];
        }
    }
}

// da2[e] = dagg[tgt[e]] / max(deg, 1) * Swish'(a2[e]);  thread = (edge, 16-B channel group)
__global__ __launch_bounds__(256) void mean_bwd_dswish_kernel(const float* __restrict__ dagg, int ld, const int* __restrict__ rowptr,
                                                              const int* __restrict__ tgt, const float* __restrict__ a2,
                                                              long n_edges, float* __restrict__ out) {
    const long total = n_edges * (H / 4);
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        const long e = p >> 5;
        const int cg = (int)(p & 31), i = tgt[e];
        const float inv = 1.0f / (float)max(rowptr[i + 1] - rowptr[i], 1);
        const f32x4 g = *reinterpret_cast<const f32x4*>(dagg + (size_t)i * ld + 4 * cg);
        const f32x4 a = reinterpret_cast<const f32x4*>(a2)[p];
        f32x4 r;
#pragma unroll
        for (int m = 0; m < 4; ++m) r[m] = g[m] * inv * dswish(a[m]);
        reinterpret_cast<f32x4*>(out)[p] = r;
    }
}

// y = (x - mean) rstd per graph and channel:  dx = rstd (g - mean_graph(g) - y mean_graph(g y))
__device__ __forceinline__ void norm_bwd_sums(const float* __restrict__ x, const float* __restrict__ g, int n0, int n1, int cg, int rs,
                                              f32x4* red, f32x4 mean, f32x4 rstd, f32x4& g_mean, f32x4& gy_mean) {
    f32x4 s = {0.f, 0.f, 0.f, 0.f}, q = {0.f, 0.f, 0.f, 0.f};
    for (int r = n0 + rs; r < n1; r += 8) {
        const size_t o = (size_t)r * (H / 4) + cg;
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[o];
        s += gv;
        q += gv * ((reinterpret_cast<const f32x4*>(x)[o] - mean) * rstd);
    }
    const float inv = 1.0f / (float)max(n1 - n0, 1);
    g_mean = block_colsum(s, red, cg, rs) * inv;
    gy_mean = block_colsum(q, red, cg, rs) * inv;
}

__global__ __launch_bounds__(256) void instance_norm_bwd_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                const int* __restrict__ graph_ptr, float eps, float* __restrict__ dx) {
    __shared__ f32x4 red[256];
    const int cg = threadIdx.x & 31, rs = threadIdx.x >> 5;
    const int n0 = graph_ptr[blockIdx.x], n1 = graph_ptr[blockIdx.x + 1];
    f32x4 mean, rstd, gm, gym;
    graph_stats(x, n0, n1, cg, rs, red, eps, mean, rstd);
    norm_bwd_sums(x, g, n0, n1, cg, rs, red, mean, rstd, gm, gym);
    for (int r = n0 + rs; r < n1; r += 8) {
        const size_t o = (size_t)r * (H / 4) + cg;
        const f32x4 y = (reinterpret_cast<const f32x4*>(x)[o] - mean) * rstd;
        reinterpret_cast<f32x4*>(dx)[o] = rstd * (reinterpret_cast<const f32x4*>(g)[o] - gm - y * gym);
    }
}

// out = (1 - tau) h + tau s,  tau = sigmoid(IN(gate_pre)),  s = Swish(IN(main_pre)):
//   d IN(gate) = g (s - h) tau (1 - tau);  d IN(main) = g tau Swish'(IN(main));  dh = g (1 - tau);  then both InstanceNorm backwards.
// The two upstream gradients are formed on the fly in each pass (never stored): 3 passes over g, h, gate_pre, main_pre.
__device__ __forceinline__ void blend_grads(f32x4 g, f32x4 hv, f32x4 yg, f32x4 ym, f32x4& dyg, f32x4& dym, f32x4& dh) {
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const float tau = sigmoidf_(yg[m]);
        dyg[m] = g[m] * (swishf(ym[m]) - hv[m]) * tau * (1.0f - tau);
        dym[m] = g[m] * tau * dswish(ym[m]);
        dh[m] = g[m] * (1.0f - tau);
    }
}

__global__ __launch_bounds__(256) void gate_blend_bwd_kernel(const float* __restrict__ gout, const float* __restrict__ h,
                                                             const float* __restrict__ gate, const float* __restrict__ mainp,
                                                             const int* __restrict__ graph_ptr, float eps, float* __restrict__ d_gate,
                                                             float* __restrict__ d_main, float* __restrict__ dh_out) {
    __shared__ f32x4 red[256];
    const int cg = threadIdx.x & 31, rs = threadIdx.x >> 5;
    const int n0 = graph_ptr[blockIdx.x], n1 = graph_ptr[blockIdx.x + 1];
    f32x4 gm, gr, mm, mr;
    graph_stats(gate, n0, n1, cg, rs, red, eps, gm, gr);
    graph_stats(mainp, n0, n1, cg, rs, red, eps, mm, mr);
    const f32x4* gp = reinterpret_cast<const f32x4*>(gout);
    const f32x4* hp = reinterpret_cast<const f32x4*>(h);
    const f32x4* tp = reinterpret_cast<const f32x4*>(gate);
    const f32x4* mp = reinterpret_cast<const f32x4*>(mainp);
    f32x4 sg = {0.f, 0.f, 0.f, 0.f}, sgy = sg, sm = sg, smy = sg;
    for (int r = n0 + rs; r < n1; r += 8) {
        const size_t o = (size_t)r * (H / 4) + cg;
        const f32x4 yg = (tp[o] - gm) * gr, ym = (mp[o] - mm) * mr;
        f32x4 dyg, dym, dh;
        blend_grads(gp[o], hp[o], yg, ym, dyg, dym, dh);
        sg += dyg; sgy += dyg * yg; sm += dym; smy += dym * ym;
    }
    const float inv = 1.0f / (float)max(n1 - n0, 1);
    sg = block_colsum(sg, red, cg, rs) * inv;
    sgy = block_colsum(sgy, red, cg, rs) * inv;
    sm = block_colsum(sm, red, cg, rs) * inv;
    smy = block_colsum(smy, red, cg, rs) * inv;
    for (int r = n0 + rs; r < n1; r += 8) {
        const size_t o = (size_t)r * (H / 4) + cg;
        const f32x4 yg = (tp[o] - gm) * gr, ym = (mp[o] - mm) * mr;
        f32x4 dyg, dym, dh;
        blend_grads(gp[o], hp[o], yg, ym, dyg, dym, dh);
        reinterpret_cast<f32x4*>(d_gate)[o] = gr * (dyg - sg - yg * sgy);
        reinterpret_cast<f32x4*>(d_main)[o] = mr * (dym - sm - ym * smy);
        reinterpret_cast<f32x4*>(dh_out)[o] = dh;
    }
}

}  // namespace msmp

using namespace msmp;

extern "C" int msmp_edge_concat_f32(const float* h, const float* u, const float* pos, const float* vars, const int32_t* tgt,
                                    const int32_t* col, int64_t n_edges, int tw, int nv, int ld, float* out, msmp_stream_t stream) {
    MSMP_REQUIRE(h && u && pos && vars && tgt && col && out, MSMP_ERR_ARG, "msmp_edge_concat_f32: null pointer");
    MSMP_REQUIRE(n_edges >= 0 && n_edges < (1L << 31) && tw >= 1 && nv >= 1 && nv <= MSMP_MAX_VARS, MSMP_ERR_ARG, "msmp_edge_concat_f32: bad sizes");
    MSMP_REQUIRE(tw + 1 + nv <= 128, MSMP_ERR_UNSUPPORTED, "msmp_edge_concat_f32: tw + 1 + nv = %d > 128", tw + 1 + nv);
    MSMP_REQUIRE(ld >= 2 * H + tw + 1 + nv && ld % 4 == 0, MSMP_ERR_ARG, "msmp_edge_concat_f32: row stride %d (need a multiple of 4 >= %d)", ld,
                 2 * H + tw + 1 + nv);
    if (n_edges == 0) return MSMP_OK;
    const unsigned grid = (unsigned)((n_edges + 3) / 4 < 16384 ? (n_edges + 3) / 4 : 16384);
    hipLaunchKernelGGL(edge_concat_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, h, u, pos, vars, tgt, col, (long)n_edges, tw, nv,
                       ld, out);
    return check_launch("edge_concat_kernel");
}

extern "C" int msmp_mean_bwd_dswish_f32(const float* dagg, const int32_t* rowptr, const int32_t* tgt, const float* a2, int64_t n_edges,
                                        float* out, msmp_stream_t stream) {
    MSMP_REQUIRE(dagg && rowptr && tgt && a2 && out, MSMP_ERR_ARG, "msmp_mean_bwd_dswish_f32: null pointer");
    MSMP_REQUIRE(n_edges >= 0 && n_edges < (1L << 31), MSMP_ERR_ARG, "msmp_mean_bwd_dswish_f32: bad sizes");
    if (n_edges == 0) return MSMP_OK;
    const long blocks = (n_edges * (H / 4) + 255) / 256;
    hipLaunchKernelGGL(mean_bwd_dswish_kernel, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, (hipStream_t)stream, dagg,
                       H, rowptr, tgt, a2, (long)n_edges, out);
    return check_launch("mean_bwd_dswish_kernel");
}

extern "C" int msmp_instance_norm_bwd_f32(const float* x, const float* grad_y, const int32_t* graph_ptr, int64_t n_graphs, float eps,
                                          float* dx_out, msmp_stream_t stream) {
    MSMP_REQUIRE(x && grad_y && graph_ptr && dx_out, MSMP_ERR_ARG, "msmp_instance_norm_bwd_f32: null pointer");
    MSMP_REQUIRE(n_graphs > 0 && n_graphs < (1L << 31), MSMP_ERR_ARG, "msmp_instance_norm_bwd_f32: bad n_graphs");
    hipLaunchKernelGGL(instance_norm_bwd_kernel, dim3((unsigned)n_graphs), dim3(256), 0, (hipStream_t)stream, x, grad_y, graph_ptr, eps,
                       dx_out);
    return check_launch("instance_norm_bwd_kernel");
}

extern "C" int msmp_gate_blend_bwd_f32(const float* grad_out, const float* h, const float* gate_pre, const float* main_pre,
                                       const int32_t* graph_ptr, int64_t n_graphs, float eps, float* d_gate_pre, float* d_main_pre,
                                       float* dh_out, msmp_stream_t stream) {
    MSMP_REQUIRE(grad_out && h && gate_pre && main_pre && graph_ptr && d_gate_pre && d_main_pre && dh_out, MSMP_ERR_ARG,
                 "msmp_gate_blend_bwd_f32: null pointer");
    MSMP_REQUIRE(n_graphs > 0 && n_graphs < (1L << 31), MSMP_ERR_ARG, "msmp_gate_blend_bwd_f32: bad n_graphs");
    hipLaunchKernelGGL(gate_blend_bwd_kernel, dim3((unsigned)n_graphs), dim3(256), 0, (hipStream_t)stream, grad_out, h, gate_pre,
                       main_pre, graph_ptr, eps, d_gate_pre, d_main_pre, dh_out);
    return check_launch("gate_blend_bwd_kernel");
}

namespace msmp {

// ---- rocBLAS for bwd_gemm = 0: resolved with dlopen on first use, so inference and the default backward never load it -----------------
struct Blas {
    rocblas_handle handle = nullptr;
    rocblas_status (*sgemm)(rocblas_handle, rocblas_operation, rocblas_operation, rocblas_int, rocblas_int, rocblas_int, const float*,
                            const float*, rocblas_int, const float*, rocblas_int, const float*, float*, rocblas_int) = nullptr;
    rocblas_status (*set_stream)(rocblas_handle, hipStream_t) = nullptr;
    bool tried = false;
};

static Blas& blas() {
    static thread_local Blas b;          // one handle per calling thread (the autograd engine calls from its own)
    if (!b.tried) {
        b.tried = true;
        void* lib = dlopen("librocblas.so.5", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librocblas.so", RTLD_NOW | RTLD_GLOBAL);
        if (lib) {
            auto create = reinterpret_cast<rocblas_status (*)(rocblas_handle*)>(dlsym(lib, "rocblas_create_handle"));
            b.sgemm = reinterpret_cast<decltype(b.sgemm)>(dlsym(lib, "rocblas_sgemm"));
            b.set_stream = reinterpret_cast<decltype(b.set_stream)>(dlsym(lib, "rocblas_set_stream"));
            if (!create || !b.sgemm || !b.set_stream || create(&b.handle) != rocblas_status_success) b.handle = nullptr;
        }
    }
    return b;
}

// row-major helpers on the column-major library (a row-major [R,C] matrix with stride ld is the column-major [C,R] one)
//   C[M,N] = A[M,K] W[N,K]^T      (a linear layer's forward)
static rocblas_status gemm_nt(Blas& b, int M, int N, int K, const float* A, int lda, const float* W, int ldw, float* C, int ldc) {
    const float one = 1.f, zero = 0.f;
    return b.sgemm(b.handle, rocblas_operation_transpose, rocblas_operation_none, N, M, K, &one, W, ldw, A, lda, &zero, C, ldc);
}
//   C[M,K2] = G[M,N] W[N, :K2]    (its data gradient; W's row stride ldw >= K2)
static rocblas_status gemm_nn(Blas& b, int M, int K2, int N, const float* G, int ldg, const float* W, int ldw, float* C, int ldc) {
    const float one = 1.f, zero = 0.f;
    return b.sgemm(b.handle, rocblas_operation_none, rocblas_operation_none, K2, M, N, &one, W, ldw, G, ldg, &zero, C, ldc);
}

// ---- elementwise glue on [rows, 128] tensors (thread = 16-byte channel group) ----------------------------------------
__global__ __launch_bounds__(256) void bias_silu_kernel(float* __restrict__ a, const float* __restrict__ bias, float* __restrict__ m, long n4) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n4; p += (long)gridDim.x * blockDim.x) {
        const f32x4 v = reinterpret_cast<f32x4*>(a)[p] + reinterpret_cast<const f32x4*>(bias)[p & 31];
        reinterpret_cast<f32x4*>(a)[p] = v;
        if (m) {
            f32x4 r;
#pragma unroll
            for (int i = 0; i < 4; ++i) r[i] = swishf(v[i]);
            reinterpret_cast<f32x4*>(m)[p] = r;
        }
    }
}

// out = g * Swish'(a)   (out may alias g)
__global__ __launch_bounds__(256) void dsilu_mul_kernel(const float* g, const float* __restrict__ a, float* out, long n4) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n4; p += (long)gridDim.x * blockDim.x) {
        const f32x4 gv = reinterpret_cast<const f32x4*>(g)[p], av = reinterpret_cast<const f32x4*>(a)[p];
        f32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = gv[i] * dswish(av[i]);
        reinterpret_cast<f32x4*>(out)[p] = r;
    }
}

__global__ __launch_bounds__(256) void fill_kernel(float* __restrict__ x, float v, long n) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n; p += (long)gridDim.x * blockDim.x) x[p] = v;
}

// out = h + Swish(upd)   (GNN_Layer's pre-norm tensor)
__global__ __launch_bounds__(256) void residual_silu_kernel(const float* __restrict__ h, const float* __restrict__ upd, float* __restrict__ out, long n4) {
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < n4; p += (long)gridDim.x * blockDim.x) {
        const f32x4 hv = reinterpret_cast<const f32x4*>(h)[p], uv = reinterpret_cast<const f32x4*>(upd)[p];
        f32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = hv[i] + swishf(uv[i]);
        reinterpret_cast<f32x4*>(out)[p] = r;
    }
}

// the input of update_net_1: out[n] = [h[n] | agg[n] | vars[n]]  (row stride ld, a multiple of 4)
__global__ __launch_bounds__(256) void cat_node_kernel(const float* __restrict__ h, const float* __restrict__ agg, const float* __restrict__ vars,
                                                       long n_nodes, int nv, int ld, float* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    const long wave = (long)blockIdx.x * 4 + (threadIdx.x >> 6), n_waves = (long)gridDim.x * 4;
    for (long n = wave; n < n_nodes; n += n_waves) {
        float* row = out + (size_t)n * ld;
        const float* src = lane < 32 ? h : agg;
        *reinterpret_cast<f32x4*>(row + 4 * lane) = *reinterpret_cast<const f32x4*>(src + (size_t)n * H + 4 * (lane & 31));
        if (lane < nv) row[2 * H + lane] = vars[(size_t)n * nv + lane];
    }
}

// dh[n] += x[n][0..127]   (x row stride ld)
__global__ __launch_bounds__(256) void add_cols_kernel(float* __restrict__ dh, const float* __restrict__ x, int ld, long n_nodes) {
    const long total = n_nodes * (H / 4);
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        const long n = p >> 5;
        const int cg = (int)(p & 31);
        reinterpret_cast<f32x4*>(dh)[p] += *reinterpret_cast<const f32x4*>(x + (size_t)n * ld + 4 * cg);
    }
}

// dh[i] += sum over the in-edges e of i of d[e][0..127]   (CSR order: deterministic), thread = (node, channel group)
__global__ __launch_bounds__(256) void scatter_target_kernel(float* __restrict__ dh, const float* __restrict__ d, int ld,
                                                             const int* __restrict__ rowptr, long n_nodes, int overwrite = 0) {
    const long total = n_nodes * (H / 4);
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        const long n = p >> 5;
        const int cg = (int)(p & 31);
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int e = rowptr[n]; e < rowptr[n + 1]; ++e) s += *reinterpret_cast<const f32x4*>(d + (size_t)e * ld + 4 * cg);
        if (overwrite) reinterpret_cast<f32x4*>(dh)[p] = s;
        else reinterpret_cast<f32x4*>(dh)[p] += s;
    }
}

// dh[col[e]] += d[e][128..255]   (the source side: atomics, order not fixed)
__global__ __launch_bounds__(256) void scatter_source_kernel(float* __restrict__ dh, const float* __restrict__ d, int ld,
                                                             const int* __restrict__ col, long n_edges) {
    const long total = n_edges * H;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        const long e = p >> 7;
        const int c = (int)(p & 127);
        atomicAdd(dh + (size_t)col[e] * H + c, d[(size_t)e * ld + H + c]);
    }
}

// the same in a FIXED order: the edges regrouped by source (src_rowptr [N+1], src_perm [E] = CSR edge ids, ascending inside a
// source), thread = (node, channel group): run-to-run bitwise reproducible gradients
__global__ __launch_bounds__(256) void scatter_source_sorted_kernel(float* __restrict__ dh, const float* __restrict__ d, int ld,
                                                                    const int* __restrict__ src_rowptr, const int* __restrict__ src_perm,
                                                                    long n_nodes, int col_off = H, int overwrite = 0) {
    const long total = n_nodes * (H / 4);
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        const long n = p >> 5;
        const int cg = (int)(p & 31);
        f32x4 s = {0.f, 0.f, 0.f, 0.f};
        for (int k = src_rowptr[n]; k < src_rowptr[n + 1]; ++k)
            s += *reinterpret_cast<const f32x4*>(d + (size_t)src_perm[k] * ld + col_off + 4 * cg);
        if (overwrite) reinterpret_cast<f32x4*>(dh)[p] = s;
        else reinterpret_cast<f32x4*>(dh)[p] += s;
    }
}

// ----------------------------------------------------------------------------------------------------------------------
// message_net_1 WITHOUT edge-sized GEMMs in the backward (round 2).  Its input row is [h_i, h_j, u_i - u_j, p_i - p_j, v_i]:
//   forward    a1_e = P[tgt_e] + Q[src_e],   P = W1[:, h_i | u | p | v] F_i + b1,   Q = W1[:, h_j | -u | -p] F_j,   F = [h | u | p | v] per NODE
//   backward   with S_t[i] = sum over in-edges of d a1, S_s[j] = sum over out-edges of d a1 (both in a fixed order):
//              dh += S_t W1[:, h_i] + S_s W1[:, h_j];   dW1[:, h_i | u,p | v] = S_t^T F,   dW1[:, h_j] and the negative u, p part = S_s^T F;   db1 = sum S_t
// i.e. the [E,284] input, its two 284- / 256-wide GEMMs and the largest weight-gradient reduction become node-sized (E = 5.9 N).
// ----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void node_feat_kernel(const float* __restrict__ h, const float* __restrict__ u, const float* __restrict__ pos,
                                                        const float* __restrict__ vars, long n_nodes, int tw, int nv, int ldf, float* __restrict__ out) {
    const int g4 = ldf / 4;
    const long total = n_nodes * g4;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        const long n = p / g4;
        const int g = (int)(p - n * g4);
        f32x4 v;
        if (g < 32) v = *reinterpret_cast<const f32x4*>(h + (size_t)n * H + 4 * g);
        else {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const int k = 4 * (g - 32) + m;
                v[m] = k < tw ? u[(size_t)n * tw + k] : (k == tw ? pos[n] : (k <= tw + nv ? vars[(size_t)n * nv + (k - tw - 1)] : 0.f));
            }
        }
        *reinterpret_cast<f32x4*>(out + (size_t)n * ldf + 4 * g) = v;
    }
}
// WP[o][:] = [W1[o][0:128] | W1[o][256:256+tw+1+nv] | 0],  WQ[o][:] = [W1[o][128:256] | -W1[o][256:256+tw+1] | 0]
__global__ __launch_bounds__(256) void pq_weights_kernel(const float* __restrict__ w1, int kmsg, int tw, int nv, int ldf, float* __restrict__ wp,
                                                         float* __restrict__ wq) {
    const int total = H * ldf;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += gridDim.x * blockDim.x) {
        const int o = p / ldf, k = p - o * ldf;
        float vp = 0.f, vq = 0.f;
        if (k < H) { vp = w1[(size_t)o * kmsg + k]; vq = w1[(size_t)o * kmsg + H + k]; }
        else if (k - H < tw + 1 + nv) {
            vp = w1[(size_t)o * kmsg + H + k];           // column 256 + (k - 128)
            if (k - H < tw + 1) vq = -vp;
        }
        wp[p] = vp;
        wq[p] = vq;
    }
}
// a1[e] = P[tgt[e]] + Q[src[e]],  m1[e] = Swish(a1[e])   (thread = edge x 16-byte channel group)
__global__ __launch_bounds__(256) void edge_gather_add_kernel(const float* __restrict__ P, const float* __restrict__ Q, const int* __restrict__ tgt,
                                                              const int* __restrict__ src, long n_edges, float* __restrict__ a1, float* __restrict__ m1) {
    const long total = n_edges * 32;
    for (long p = (long)blockIdx.x * blockDim.x + threadIdx.x; p < total; p += (long)gridDim.x * blockDim.x) {
        const long e = p >> 5;
        const int cg = (int)(p & 31);
        const f32x4 v = *reinterpret_cast<const f32x4*>(P + (size_t)tgt[e] * H + 4 * cg) + *reinterpret_cast<const f32x4*>(Q + (size_t)src[e] * H + 4 * cg);
        f32x4 s;
#pragma unroll
        for (int m = 0; m < 4; ++m) s[m] = swishf(v[m]);
        reinterpret_cast<f32x4*>(a1)[p] = v;
        reinterpret_cast<f32x4*>(m1)[p] = s;
    }
}
// dW1 [128, kmsg] from  t1 = S_t^T F [128, kf]  and  t2 = S_s^T F [128, kq]   (kf = 128 + tw + 1 + nv, kq = 128 + tw + 1)
__global__ __launch_bounds__(256) void combine_w1_kernel(const float* __restrict__ t1, const float* __restrict__ t2, int kf, int kq, int kmsg, int tw,
                                                         float* __restrict__ dw1) {
    const int total = H * kmsg;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += gridDim.x * blockDim.x) {
        const int o = p / kmsg, k = p - o * kmsg;
        float v;
        if (k < H) v = t1[(size_t)o * kf + k];
        else if (k < 2 * H) v = t2[(size_t)o * kq + (k - H)];
        else {
            const int j = k - 2 * H;                     // tail column
            v = t1[(size_t)o * kf + H + j];
            if (j < tw + 1) v -= t2[(size_t)o * kq + H + j];
        }
        dw1[p] = v;
    }
}

struct BwdCtx {
    const float *h, *u, *pos, *vars;
    const int32_t *rowptr, *col, *tgt, *graph_ptr, *src_rowptr, *src_perm;
    long n, e, g;
    int tw, nv, kmsg, kupd, ld_e, ld_n;
    hipStream_t st;
};

struct HeadBuf {      // per head: recompute intermediates and gradient scratch
    float *cat_e, *a1, *m1, *a2, *x2, *x1, *dcat_e;             // edge-sized: [E, ld_e], 5 x [E,128], [E,256]
    float *agg, *cat_n, *a3, *u1, *upd, *dupd, *x3, *dcat_n;    // node-sized: [N,128], [N, ld_n], 5 x [N,128], [N,256]
    // factorised message_net_1: node features F [N, ldf] (shared by the heads), P, Q, S_t, S_s [N,128], WP, WQ [128, ldf],
    // weight-gradient pieces t1 [128, kf], t2 [128, kq], an unused bias row [128]
    float *feat, *P, *Q, *st, *ss, *wp, *wq, *t1, *t2, *tb;
};
static int fact_ldf(int tw, int nv) { return H + 32 * ((tw + 1 + nv + 31) / 32); }
// row stride the workspace reserves for F, WP, WQ, t1, t2: H + 64 (every tw + 1 + nv <= 64, the sizes of before), H + 128 above
static int ws_ldf(int tw, int nv) { return tw + 1 + nv <= 64 ? H + 64 : fact_ldf(tw, nv); }

static size_t head_floats(long n, long e, int ld_e, int ld_n, int ldf) {
    return (size_t)e * (ld_e + 5 * H + 2 * H) + (size_t)n * (H + ld_n + 5 * H + 2 * H) + (size_t)n * (ldf + 4 * H) + 4 * (size_t)H * ldf + H + 10 * 64;
}

static void carve(float*& p, long n, long e, int ld_e, int ld_n, int ldf, HeadBuf& b) {
    auto take = [&](size_t k) { float* r = p; p += (k + 63) / 64 * 64; return r; };
    b.cat_e = take((size_t)e * ld_e); b.a1 = take((size_t)e * H); b.m1 = take((size_t)e * H); b.a2 = take((size_t)e * H);
    b.x2 = take((size_t)e * H); b.x1 = take((size_t)e * H); b.dcat_e = take((size_t)e * 2 * H);
    b.agg = take((size_t)n * H); b.cat_n = take((size_t)n * ld_n); b.a3 = take((size_t)n * H); b.u1 = take((size_t)n * H);
    b.upd = take((size_t)n * H); b.dupd = take((size_t)n * H); b.x3 = take((size_t)n * H); b.dcat_n = take((size_t)n * 2 * H);
    b.feat = take((size_t)n * ldf); b.P = take((size_t)n * H); b.Q = take((size_t)n * H); b.st = take((size_t)n * H); b.ss = take((size_t)n * H);
    b.wp = take((size_t)H * ldf); b.wq = take((size_t)H * ldf); b.t1 = take((size_t)H * ldf); b.t2 = take((size_t)H * ldf); b.tb = take(H);
}

// the ten weight operands of one head, packed once per backward call
struct HeadFrags {
    u32x4 *w1, *w2, *w3, *w4;            // forward forms (K = kmsg, 128, kupd, 128)
    u32x4 *w4t, *w3t[2], *w2t, *w1t[2];  // data-gradient forms (reduction over the 128 output channels; 128-column groups of the input)
    u32x4 *wp, *wq;                      // factorised message_net_1: the per-node projections (K = fact_ldf)
};
static size_t head_frag_u4(int kmsg, int kupd, int ldf) {
    return (size_t)RG_CHUNK_U4 * ((kmsg + 31) / 32 + 4 + (kupd + 31) / 32 + 4 + 6 * 4 + 2 * (ldf / 32));
}
static void carve_frags(u32x4*& p, int kmsg, int kupd, int ldf, HeadFrags& f) {
    auto take = [&](int chunks) { u32x4* r = p; p += (size_t)chunks * RG_CHUNK_U4; return r; };
    f.w1 = take((kmsg + 31) / 32); f.w2 = take(4); f.w3 = take((kupd + 31) / 32); f.w4 = take(4);
    f.w4t = take(4); f.w3t[0] = take(4); f.w3t[1] = take(4); f.w2t = take(4); f.w1t[0] = take(4); f.w1t[1] = take(4);
    f.wp = take(ldf / 32); f.wq = take(ldf / 32);
}
static int pack_head_frags(const float* const* p, int kmsg, int kupd, const HeadFrags& f, RgPackArgs& a, int& blocks, const float* wp, const float* wq,
                           int ldf) {
    if (wp) {        // factorised message_net_1: the projection weights replace the [128, kmsg] forward form
        add_pack(a, blocks, wp, ldf, ldf, 0, 0, f.wp);
        add_pack(a, blocks, wq, ldf, ldf, 0, 0, f.wq);
    } else
        add_pack(a, blocks, p[0], kmsg, kmsg, 0, 0, f.w1);
    add_pack(a, blocks, p[2], H, H, 0, 0, f.w2);
    add_pack(a, blocks, p[4], kupd, kupd, 0, 0, f.w3);
    add_pack(a, blocks, p[6], H, H, 0, 0, f.w4);
    add_pack(a, blocks, p[6], H, H, 0, 1, f.w4t);
    add_pack(a, blocks, p[4], kupd, H, 0, 1, f.w3t[0]);
    add_pack(a, blocks, p[4], kupd, H, H, 1, f.w3t[1]);
    add_pack(a, blocks, p[2], H, H, 0, 1, f.w2t);
    add_pack(a, blocks, p[0], kmsg, H, 0, 1, f.w1t[0]);
    add_pack(a, blocks, p[0], kmsg, H, H, 1, f.w1t[1]);
    return MSMP_OK;
}

#define BLAS_OK(call, what) do { if ((call) != rocblas_status_success) { set_error("msmp_mp_layer_bwd_f32: rocblas_sgemm failed (%s)", what); return MSMP_ERR_HIP; } } while (0)

// upd = W4 Swish(W3 [h, mean_j Swish(W2 Swish(W1 cat_e + b1) + b2), vars] + b3) + b4, keeping the pre-activations
static int head_recompute(const BwdCtx& c, Blas& bl, const HeadFrags* fr, const float* const* p, HeadBuf& b, bool build_cat_e) {
    const long n = c.n, e = c.e;
    if (e) {
        const bool fact = fr && c.src_rowptr;       // message_net_1 through the per-node projections (no [E, kmsg] input, no edge-sized GEMM)
        if (fact) {
            const int ldf = fact_ldf(c.tw, c.nv);
            if (build_cat_e)
                hipLaunchKernelGGL(node_feat_kernel, dim3(grid_for(n * (ldf / 4))), dim3(256), 0, c.st, c.h, c.u, c.pos, c.vars, n, c.tw, c.nv, ldf, b.feat);
            RC(rows_gemm(1, b.feat, ldf, n, ldf, fr->wp, p[1], nullptr, b.P, H, nullptr, c.st));
            RC(rows_gemm(3, b.feat, ldf, n, ldf, fr->wq, nullptr, nullptr, b.Q, H, nullptr, c.st));
            hipLaunchKernelGGL(edge_gather_add_kernel, dim3(grid_for(e * 32)), dim3(256), 0, c.st, b.P, b.Q, c.tgt, c.col, e, b.a1, b.m1);
            RC(rows_gemm(0, b.m1, H, e, H, fr->w2, p[3], nullptr, b.a2, H, b.x2, c.st));
        } else if (fr) {
            if (build_cat_e) RC(msmp_edge_concat_f32(c.h, c.u, c.pos, c.vars, c.tgt, c.col, e, c.tw, c.nv, c.ld_e, b.cat_e, c.st));
            RC(rows_gemm(0, b.cat_e, c.ld_e, e, c.kmsg, fr->w1, p[1], nullptr, b.a1, H, b.m1, c.st));
            RC(rows_gemm(0, b.m1, H, e, H, fr->w2, p[3], nullptr, b.a2, H, b.x2, c.st));
        } else {
            if (build_cat_e) RC(msmp_edge_concat_f32(c.h, c.u, c.pos, c.vars, c.tgt, c.col, e, c.tw, c.nv, c.ld_e, b.cat_e, c.st));
            BLAS_OK(gemm_nt(bl, (int)e, H, c.kmsg, b.cat_e, c.ld_e, p[0], c.kmsg, b.a1, H), "message_net_1");
            hipLaunchKernelGGL(bias_silu_kernel, dim3(grid_for(e * 32)), dim3(256), 0, c.st, b.a1, p[1], b.m1, e * 32);
            BLAS_OK(gemm_nt(bl, (int)e, H, H, b.m1, H, p[2], H, b.a2, H), "message_net_2");
            hipLaunchKernelGGL(bias_silu_kernel, dim3(grid_for(e * 32)), dim3(256), 0, c.st, b.a2, p[3], b.x2, e * 32);
        }
        RC(msmp_scatter_mean_f32(b.x2, c.rowptr, n, b.agg, c.st));
    } else
        hipLaunchKernelGGL(fill_kernel, dim3(grid_for(n * H)), dim3(256), 0, c.st, b.agg, 0.f, n * H);
    hipLaunchKernelGGL(cat_node_kernel, dim3(grid_for(n * 64)), dim3(256), 0, c.st, c.h, b.agg, c.vars, n, c.nv, c.ld_n, b.cat_n);
    if (fr) {
        RC(rows_gemm(0, b.cat_n, c.ld_n, n, c.kupd, fr->w3, p[5], nullptr, b.a3, H, b.u1, c.st));
        RC(rows_gemm(1, b.u1, H, n, H, fr->w4, p[7], nullptr, b.upd, H, nullptr, c.st));
    } else {
        BLAS_OK(gemm_nt(bl, (int)n, H, c.kupd, b.cat_n, c.ld_n, p[4], c.kupd, b.a3, H), "update_net_1");
        hipLaunchKernelGGL(bias_silu_kernel, dim3(grid_for(n * 32)), dim3(256), 0, c.st, b.a3, p[5], b.u1, n * 32);
        BLAS_OK(gemm_nt(bl, (int)n, H, H, b.u1, H, p[6], H, b.upd, H), "update_net_2");
        hipLaunchKernelGGL(bias_silu_kernel, dim3(grid_for(n * 32)), dim3(256), 0, c.st, b.upd, p[7], (float*)nullptr, n * 32);
    }
    return check_launch("layer backward: recompute");
}

struct GwJobs {
    const float *a[GW_MAX_JOBS], *b[GW_MAX_JOBS];
    int64_t rows[GW_MAX_JOBS];
    int lda[GW_MAX_JOBS], ldb[GW_MAX_JOBS], k2[GW_MAX_JOBS];
    float *out_w[GW_MAX_JOBS], *out_b[GW_MAX_JOBS];
    int n = 0;
    void add(const float* a_, const float* b_, int64_t rows_, int ldb_, int k2_, float* w, float* bias) {
        a[n] = a_; b[n] = b_; rows[n] = rows_; lda[n] = H; ldb[n] = ldb_; k2[n] = k2_; out_w[n] = w; out_b[n] = bias; ++n;
    }
};

// b.dupd = dL/d upd  ->  dh += dL/dh through this head; the four (gradient, input) pairs are queued for the weight-gradient kernel
static int head_backward(const BwdCtx& c, Blas& bl, const HeadFrags* fr, const float* const* p, HeadBuf& b, float* dh, float* const* grads, GwJobs& jobs) {
    const long n = c.n, e = c.e;
    if (fr) {
        RC(rows_gemm(2, b.dupd, H, n, H, fr->w4t, nullptr, b.a3, b.x3, H, nullptr, c.st));                                       // d a3
        RC(rows_gemm(3, b.x3, H, n, H, fr->w3t[0], nullptr, nullptr, b.dcat_n, 2 * H, nullptr, c.st));                           // [dh |
        RC(rows_gemm(3, b.x3, H, n, H, fr->w3t[1], nullptr, nullptr, b.dcat_n + H, 2 * H, nullptr, c.st));                       //  dagg]
    } else {
        BLAS_OK(gemm_nn(bl, (int)n, H, H, b.dupd, H, p[6], H, b.x3, H), "d update_net_2");
        hipLaunchKernelGGL(dsilu_mul_kernel, dim3(grid_for(n * 32)), dim3(256), 0, c.st, b.x3, b.a3, b.x3, n * 32);             // d a3
        BLAS_OK(gemm_nn(bl, (int)n, 2 * H, H, b.x3, H, p[4], c.kupd, b.dcat_n, 2 * H), "d update_net_1");                        // [dh | dagg]
    }
    hipLaunchKernelGGL(add_cols_kernel, dim3(grid_for(n * 32)), dim3(256), 0, c.st, dh, b.dcat_n, 2 * H, n);
    if (e) {
        hipLaunchKernelGGL(mean_bwd_dswish_kernel, dim3(grid_for(e * 32)), dim3(256), 0, c.st, b.dcat_n + H, 2 * H, c.rowptr, c.tgt, b.a2, e, b.x2);   // d a2
        const bool fact = fr && c.src_rowptr;
        if (fact) {
            const int ldf = fact_ldf(c.tw, c.nv), kf = H + c.tw + 1 + c.nv, kq = H + c.tw + 1;
            RC(rows_gemm(2, b.x2, H, e, H, fr->w2t, nullptr, b.a1, b.x1, H, nullptr, c.st));                                     // d a1
            // S_t / S_s: d a1 summed over each node's in- / out-edges, fixed order (CSR by target; the by-source regrouping)
            hipLaunchKernelGGL(scatter_target_kernel, dim3(grid_for(n * 32)), dim3(256), 0, c.st, b.st, b.x1, H, c.rowptr, n, 1);
            hipLaunchKernelGGL(scatter_source_sorted_kernel, dim3(grid_for(n * 32)), dim3(256), 0, c.st, b.ss, b.x1, H, c.src_rowptr, c.src_perm, n, 0, 1);
            RC(rows_gemm(5, b.st, H, n, H, fr->w1t[0], nullptr, nullptr, dh, H, nullptr, c.st));                                 // dh += S_t W1[:, h_i]
            RC(rows_gemm(5, b.ss, H, n, H, fr->w1t[1], nullptr, nullptr, dh, H, nullptr, c.st));                                 // dh += S_s W1[:, h_j]
            jobs.add(b.st, b.feat, n, ldf, kf, b.t1, grads[1]);          // S_t^T F and db1 = column sums of S_t
            jobs.add(b.ss, b.feat, n, ldf, kq, b.t2, b.tb);
            jobs.add(b.x2, b.m1, e, H, H, grads[2], grads[3]);
        } else if (fr) {
            RC(rows_gemm(2, b.x2, H, e, H, fr->w2t, nullptr, b.a1, b.x1, H, nullptr, c.st));                                     // d a1
            RC(rows_gemm(3, b.x1, H, e, H, fr->w1t[0], nullptr, nullptr, b.dcat_e, 2 * H, nullptr, c.st));                       // [d x_i |
            RC(rows_gemm(3, b.x1, H, e, H, fr->w1t[1], nullptr, nullptr, b.dcat_e + H, 2 * H, nullptr, c.st));                   //  d x_j]
        } else {
            BLAS_OK(gemm_nn(bl, (int)e, H, H, b.x2, H, p[2], H, b.x1, H), "d message_net_2");
            hipLaunchKernelGGL(dsilu_mul_kernel, dim3(grid_for(e * 32)), dim3(256), 0, c.st, b.x1, b.a1, b.x1, e * 32);         // d a1
            BLAS_OK(gemm_nn(bl, (int)e, 2 * H, H, b.x1, H, p[0], c.kmsg, b.dcat_e, 2 * H), "d message_net_1");                  // [d x_i | d x_j]
        }
        if (!fact) {
            hipLaunchKernelGGL(scatter_target_kernel, dim3(grid_for(n * 32)), dim3(256), 0, c.st, dh, b.dcat_e, 2 * H, c.rowptr, n, 0);
            if (c.src_rowptr)
                hipLaunchKernelGGL(scatter_source_sorted_kernel, dim3(grid_for(n * 32)), dim3(256), 0, c.st, dh, b.dcat_e, 2 * H, c.src_rowptr,
                                   c.src_perm, n, H, 0);
            else
                hipLaunchKernelGGL(scatter_source_kernel, dim3(grid_for(e * H)), dim3(256), 0, c.st, dh, b.dcat_e, 2 * H, c.col, e);
            jobs.add(b.x1, b.cat_e, e, c.ld_e, c.kmsg, grads[0], grads[1]);
            jobs.add(b.x2, b.m1, e, H, H, grads[2], grads[3]);
        }
    } else {          // no edges: the message layers get zero gradients
        hipLaunchKernelGGL(fill_kernel, dim3(grid_for((long)H * c.kmsg)), dim3(256), 0, c.st, grads[0], 0.f, (long)H * c.kmsg);
        hipLaunchKernelGGL(fill_kernel, dim3(1), dim3(256), 0, c.st, grads[1], 0.f, (long)H);
        hipLaunchKernelGGL(fill_kernel, dim3(grid_for((long)H * H)), dim3(256), 0, c.st, grads[2], 0.f, (long)H * H);
        hipLaunchKernelGGL(fill_kernel, dim3(1), dim3(256), 0, c.st, grads[3], 0.f, (long)H);
    }
    jobs.add(b.x3, b.cat_n, n, c.ld_n, c.kupd, grads[4], grads[5]);
    jobs.add(b.dupd, b.u1, n, H, H, grads[6], grads[7]);
    return check_launch("layer backward: data gradients");
}

static int64_t bwd_gw_floats(long n, long e, int kmsg, int kupd, int heads) {
    int64_t rows[GW_MAX_JOBS];
    int k2[GW_MAX_JOBS], j = 0;
    for (int hd = 0; hd < heads; ++hd) {
        if (e) { rows[j] = e; k2[j++] = kmsg; rows[j] = e; k2[j++] = H; }
        rows[j] = n; k2[j++] = kupd; rows[j] = n; k2[j++] = H;
    }
    // (tw + 1 + nv > 64: kmsg > 319 is past the weight-gradient kernel; such layers take the factorised form only)
    const int64_t plain = kmsg - 2 * H <= 64 ? msmp_grad_weights_workspace_floats(j, rows, k2) : 0;
    j = 0;                                  // factorised message_net_1: two node-sized jobs instead of the [E, kmsg] one
    for (int hd = 0; hd < heads; ++hd) {
        if (e) { rows[j] = n; k2[j++] = kmsg - H; rows[j] = n; k2[j++] = kmsg - H; rows[j] = e; k2[j++] = H; }
        rows[j] = n; k2[j++] = kupd; rows[j] = n; k2[j++] = H;
    }
    const int64_t fact = msmp_grad_weights_workspace_floats(j, rows, k2);
    return plain < 0 || fact < 0 ? -1 : (plain > fact ? plain : fact);
}

}  // namespace msmp

extern "C" size_t msmp_mp_layer_bwd_workspace_bytes(int64_t n_nodes, int64_t n_edges, int tw, int nv, int gated) {
    if (n_nodes <= 0 || n_edges < 0 || tw < 1 || nv < 1 || nv > MSMP_MAX_VARS) return 0;
    const int kmsg = 2 * H + tw + 1 + nv, kupd = 2 * H + nv, ld_e = (kmsg + 3) / 4 * 4, ld_n = (kupd + 3) / 4 * 4;
    const int heads = gated ? 2 : 1;
    const int64_t gw = bwd_gw_floats(n_nodes, n_edges, kmsg, kupd, heads);
    if (gw < 0 || tw + 1 + nv > 128) return 0;
    const int ldf = ws_ldf(tw, nv);
    return (heads * (head_floats(n_nodes, n_edges, ld_e, ld_n, ldf) + 15 * 64) + (size_t)gw + 64) * sizeof(float) + 256 +
           heads * head_frag_u4(kmsg, kupd, ldf) * sizeof(u32x4) + 256;
}

extern "C" int msmp_mp_layer_bwd_f32(const float* grad_out, const float* h, const float* u, const float* pos, const float* vars,
                                     const int32_t* rowptr, const int32_t* col, const int32_t* tgt, const int32_t* src_rowptr,
                                     const int32_t* src_perm, const int32_t* graph_ptr,
                                     int64_t n_nodes, int64_t n_edges, int64_t n_graphs, int tw, int nv,
                                     const float* const* params_main, const float* const* params_gate, int mode, float eps,
                                     float* dh_out, float* const* grads_main, float* const* grads_gate, void* workspace,
                                     size_t workspace_bytes, msmp_stream_t stream) {
    MSMP_REQUIRE(grad_out && h && u && pos && vars && rowptr && col && tgt && graph_ptr && params_main && dh_out && grads_main && workspace,
                 MSMP_ERR_ARG, "msmp_mp_layer_bwd_f32: null pointer");
    MSMP_REQUIRE((params_gate != nullptr) == (grads_gate != nullptr), MSMP_ERR_ARG, "msmp_mp_layer_bwd_f32: give both gate arguments or none");
    MSMP_REQUIRE((src_rowptr != nullptr) == (src_perm != nullptr), MSMP_ERR_ARG, "msmp_mp_layer_bwd_f32: give both of src_rowptr, src_perm or neither");
    const bool gated = params_gate != nullptr;
    MSMP_REQUIRE(mode == MSMP_LAYER_LIN || mode == MSMP_LAYER_RESIDUAL_SWISH, MSMP_ERR_ARG, "msmp_mp_layer_bwd_f32: bad mode %d", mode);
    MSMP_REQUIRE(!gated || mode == MSMP_LAYER_LIN, MSMP_ERR_ARG, "msmp_mp_layer_bwd_f32: the gated pair uses GNN_LayerLin layers");
    MSMP_REQUIRE(n_nodes > 0 && n_edges >= 0 && n_graphs > 0 && n_nodes < (1L << 31) && n_edges < (1L << 31) && tw >= 1 && nv >= 1 &&
                     nv <= MSMP_MAX_VARS && tw + 1 + nv <= 128, MSMP_ERR_ARG, "msmp_mp_layer_bwd_f32: bad sizes");
    for (int i = 0; i < 8; ++i) {
        MSMP_REQUIRE(params_main[i] && grads_main[i], MSMP_ERR_ARG, "msmp_mp_layer_bwd_f32: null parameter / gradient pointer %d", i);
        MSMP_REQUIRE(!gated || (params_gate[i] && grads_gate[i]), MSMP_ERR_ARG, "msmp_mp_layer_bwd_f32: null gate parameter / gradient pointer %d", i);
    }
    const size_t need = msmp_mp_layer_bwd_workspace_bytes(n_nodes, n_edges, tw, nv, gated);
    MSMP_REQUIRE(need && workspace_bytes >= need, MSMP_ERR_WORKSPACE, "msmp_mp_layer_bwd_f32: workspace %zu < %zu", workspace_bytes, need);
    // rows_gemm_kernel from 32 768 edges on (measured E2 MSMP-PDE, ms per training iteration, library / own: batch 16 5.6 / 6.5,
    // batch 128 12.8 / 12.1, batch 512 39.0 / 34.0: below that the 128-row workgroups do not fill the chip); tune "bwd_gemm": 0 never, 2 always
    const int bg_mode = msmp_tune_get("bwd_gemm");
    const bool own_gemm = bg_mode != 0;        // 0: rocblas_sgemm (kept for A/B runs); the library is never loaded otherwise
    // a tail wider than 64 columns (2-D windows of 50) takes the factorised message_net_1 only: the per-edge form's [E, kmsg] weight
    // gradient (kmsg up to 365) is past the weight-gradient kernel's 319 columns
    MSMP_REQUIRE(tw + 1 + nv <= 64 || n_edges == 0 || (own_gemm && src_rowptr), MSMP_ERR_UNSUPPORTED,
                 "msmp_mp_layer_bwd_f32: tw + 1 + nv = %d > 64 needs src_rowptr / src_perm and the own GEMMs (msmp_tune(\"bwd_gemm\") != 0)", tw + 1 + nv);
    static Blas none;
    Blas& bl = own_gemm ? none : blas();
    hipStream_t st = (hipStream_t)stream;
    if (!own_gemm) {
        MSMP_REQUIRE(bl.handle, MSMP_ERR_UNSUPPORTED, "msmp_mp_layer_bwd_f32: librocblas (rocblas_sgemm) is not available in this process");
        MSMP_REQUIRE(bl.set_stream(bl.handle, st) == rocblas_status_success, MSMP_ERR_HIP, "msmp_mp_layer_bwd_f32: rocblas_set_stream failed");
    }

    BwdCtx c{h, u, pos, vars, rowptr, col, tgt, graph_ptr, src_rowptr, src_perm, (long)n_nodes, (long)n_edges, (long)n_graphs, tw, nv,
             2 * H + tw + 1 + nv, 2 * H + nv, 0, 0, st};
    c.ld_e = (c.kmsg + 3) / 4 * 4;
    c.ld_n = (c.kupd + 3) / 4 * 4;
    float* p = reinterpret_cast<float*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    HeadBuf bm, bg;
    const int ldf_ws = ws_ldf(tw, nv);
    carve(p, c.n, c.e, c.ld_e, c.ld_n, ldf_ws, bm);
    if (gated) carve(p, c.n, c.e, c.ld_e, c.ld_n, ldf_ws, bg);
    float* gw_ws = p;
    const int64_t gw_floats = bwd_gw_floats(c.n, c.e, c.kmsg, c.kupd, gated ? 2 : 1);
    const long n4 = c.n * 32;
    GwJobs jobs;
    HeadFrags fm, fg;
    const HeadFrags *frm = nullptr, *frg = nullptr;
    if (own_gemm) {      // split the weights of the call's head(s) into bf16 fragments: one launch
        u32x4* fp = reinterpret_cast<u32x4*>(((uintptr_t)(gw_ws + gw_floats + 64) + 255) & ~(uintptr_t)255);
        RgPackArgs pa;
        pa.n_jobs = 0;
        int blocks = 0;
        const bool fact = src_rowptr != nullptr && c.e > 0;
        const int ldf = fact_ldf(tw, nv);
        if (fact) {      // WP / WQ of the per-node projections first: the split launch below reads them
            hipLaunchKernelGGL(pq_weights_kernel, dim3(grid_for((long)H * ldf)), dim3(256), 0, st, params_main[0], c.kmsg, tw, nv, ldf, bm.wp, bm.wq);
            if (gated) hipLaunchKernelGGL(pq_weights_kernel, dim3(grid_for((long)H * ldf)), dim3(256), 0, st, params_gate[0], c.kmsg, tw, nv, ldf, bg.wp, bg.wq);
        }
        carve_frags(fp, c.kmsg, c.kupd, ldf_ws, fm);
        pack_head_frags(params_main, c.kmsg, c.kupd, fm, pa, blocks, fact ? bm.wp : nullptr, bm.wq, ldf);
        frm = &fm;
        if (gated) {
            carve_frags(fp, c.kmsg, c.kupd, ldf_ws, fg);
            pack_head_frags(params_gate, c.kmsg, c.kupd, fg, pa, blocks, fact ? bg.wp : nullptr, bg.wq, ldf);
            frg = &fg;
        }
        RC(launch_rg_pack(pa, blocks, st));
    }

    RC(head_recompute(c, bl, frm, params_main, bm, true));
    if (gated) {
        bg.cat_e = bm.cat_e;                      // both heads read the same per-edge input
        bg.feat = bm.feat;                        // ... or the same per-node feature rows
        RC(head_recompute(c, bl, frg, params_gate, bg, false));
        RC(msmp_gate_blend_bwd_f32(grad_out, h, bg.upd, bm.upd, graph_ptr, n_graphs, eps, bg.dupd, bm.dupd, dh_out, stream));
        RC(head_backward(c, bl, frm, params_main, bm, dh_out, grads_main, jobs));
        RC(head_backward(c, bl, frg, params_gate, bg, dh_out, grads_gate, jobs));
    } else if (mode == MSMP_LAYER_LIN) {          // out = IN(upd): no direct path to h
        RC(msmp_instance_norm_bwd_f32(bm.upd, grad_out, graph_ptr, n_graphs, eps, bm.dupd, stream));
        hipLaunchKernelGGL(fill_kernel, dim3(grid_for(c.n * H)), dim3(256), 0, st, dh_out, 0.f, c.n * H);
        RC(head_backward(c, bl, frm, params_main, bm, dh_out, grads_main, jobs));
    } else {                                      // out = IN(h + Swish(upd))
        hipLaunchKernelGGL(residual_silu_kernel, dim3(grid_for(n4)), dim3(256), 0, st, h, bm.upd, bm.dcat_n, n4);
        RC(msmp_instance_norm_bwd_f32(bm.dcat_n, grad_out, graph_ptr, n_graphs, eps, dh_out, stream));
        hipLaunchKernelGGL(dsilu_mul_kernel, dim3(grid_for(n4)), dim3(256), 0, st, dh_out, bm.upd, bm.dupd, n4);
        RC(head_backward(c, bl, frm, params_main, bm, dh_out, grads_main, jobs));
    }
    RC(launch_grad_weights(jobs.n, jobs.a, jobs.b, jobs.rows, jobs.lda, jobs.ldb, jobs.k2, jobs.out_w, jobs.out_b, gw_ws, gw_floats, st));
    if (frm && src_rowptr && c.e > 0) {           // assemble dW1 of the factorised message_net_1 from its two node-sized products
        const int kf = H + tw + 1 + nv, kq = H + tw + 1;
        hipLaunchKernelGGL(combine_w1_kernel, dim3(grid_for((long)H * c.kmsg)), dim3(256), 0, st, bm.t1, bm.t2, kf, kq, c.kmsg, tw, grads_main[0]);
        if (gated) hipLaunchKernelGGL(combine_w1_kernel, dim3(grid_for((long)H * c.kmsg)), dim3(256), 0, st, bg.t1, bg.t2, kf, kq, c.kmsg, tw, grads_gate[0]);
        RC(check_launch("combine_w1_kernel"));
    }
    return MSMP_OK;
}
