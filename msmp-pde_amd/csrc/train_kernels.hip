// Glue kernels of the training backward of a message-passing layer.  The backward pass
// re-evaluates a layer in materialised form -- every GEMM (data and weight gradients, K = E or N rows) is a plain
// rocBLAS call made by the host layer -- and these kernels are everything between the GEMMs that is not a single
// elementwise library op:
//   msmp_edge_concat_f32          the per-edge input of message_net_1 (models_gnn.py:69-75: cat(x_i, x_j, u_i - u_j, pos_i - pos_j, variables_i))
//   msmp_mean_bwd_dswish_f32      backward of aggr='mean' (:42,107) fused with the Swish' of message_net_2
//   msmp_instance_norm_bwd_f32    backward of PyG InstanceNorm (:59,66; affine=False, biased variance)
//   msmp_gate_blend_bwd_f32       backward of the gated blend (:1204-1207) through both InstanceNorms in one launch
// All fp32, HBM-bound, one pass per tensor where the per-graph statistics allow it.
#include "graph_norm.h"
#include "mfma_tiles.h"
#include "train_internal.h"

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

// ----------------------------------------------------------------------------------------------
// Weight gradients:  dW[m][n] = sum_r A[r][m] B[r][n]  and  db[m] = sum_r A[r][m]  for up to 8 (A, B) pairs in one call
// (A [R,128] (row stride lda) = gradient of a pre-activation, B [R, >= k2] = the input of that linear layer, R = E or N rows).
// These GEMMs are 128 x k2 outputs with a reduction over R >> 1000 rows: the library runs them on 36 workgroups
// (63 us each at R = 9 408); here the rows are split over workgroups (<= 512 splits per pair; fp32 products from six bf16 MFMAs,
// see split_bf16x3; the bias column as a virtual all-ones column k2 of B), and a second kernel sums the partials in a fixed order
// (deterministic).
// ----------------------------------------------------------------------------------------------
namespace msmp {

constexpr int GW_MAX_UNITS = 2 * GW_MAX_JOBS;       // a job of more than 160 columns is two column groups
struct GradWeightJob {
    const float* a;      // [rows, lda], columns 0..127 used
    const float* b;      // [rows, ldb], columns 0..k2-1 used (0..ksplit-1 when b2 is given)
    const float* b2;     // optional second matrix [rows, ldb2]: column c >= ksplit of the virtual B = [b | b2] is b2's column c - ksplit
    float* out_w;        // [128, k2]
    float* out_b;        // [128]
    float* partial;      // [splits][128][ldp]
    int rows, lda, ldb, k2, ldp, rows_per_split, splits, first_block;
    int c0;              // first column of B of this unit's group (0 or 160)
    int ldb2, ksplit;
};
struct GradWeightArgs {
    GradWeightJob job[GW_MAX_JOBS];       // the reduction's view: one entry per job
    GradWeightJob unit[GW_MAX_UNITS];     // the product kernel's view: one entry per (job, column group)
    int n_jobs, n_units;
};

// One workgroup = one row split of one job's column group (<= 5 output tiles = 160 columns of B; jobs with more columns are cut
// into groups so that the accumulators (80 registers) leave room for TWO 16-row blocks of operands in flight (96 registers): the
// loop is bound by load latency otherwise (measured: a 9-tile body with one block in flight ran 2.6x SLOWER than the fp32-MFMA
// kernel it replaced, ten dependent memory round trips per block).
constexpr int GW_NT = 5;
constexpr int GW_FRAG_U4 = GW_NT * 3 * 64;           // 16-byte fragments of one 16-row block of B: [tile][plane][lane] = 15 KB

// One 16-row block: lane (m, kk) of wave w loads rows rbase .. rbase + 7 of column 32 w + m of A (its own MFMA operand) and of
// column c0 + 32 w + m of B (tile w); tile 4 of the group is loaded by the wave whose turn it is (block index mod 4).  Every load is
// a 128-byte row segment across 32 lanes.  B is converted ONCE per workgroup and shared through LDS as bf16x3 fragments: with every
// wave loading and converting all five tiles itself (first round-2 edition) the B rows crossed the L1 four times and the
// conversion was 85 % of the vector work.
struct GwRegs {
    float a[8], b[8], b4[8];
};
template <bool FULL>
__device__ __forceinline__ void gw_load(const GradWeightJob& j, const float* acol, const float* bcol, int bld, const float* bcol4, int bld4, bool mine4,
                                        int rbase, int rlim, GwRegs& r) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const size_t row = FULL ? rbase + i : rbase + min(i, max(rlim - 1, 0));
        const bool in = FULL || i < rlim;
        const float va = acol[row * j.lda], vb = bcol[row * bld];
        r.a[i] = in ? va : 0.f;
        r.b[i] = in ? vb : 0.f;
    }
    if (mine4) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const size_t row = FULL ? rbase + i : rbase + min(i, max(rlim - 1, 0));
            const float v = bcol4[row * bld4];
            r.b4[i] = FULL || i < rlim ? v : 0.f;
        }
    } else {
        // defined on both paths: left untouched here, r.b4 is merged with its old value behind the branch by copies that wait for the
        // loads above (vmcnt(0) with the whole block's loads the youngest in flight: the prefetch was waited for where it was issued)
#pragma unroll
        for (int i = 0; i < 8; ++i) r.b4[i] = 0.f;
    }
}
__device__ __forceinline__ void gw_publish(const float (&b)[8], float keep, float ones, u32x4* frag_tile, int lane) {
    float bv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) bv[i] = fmaf(b[i], keep, ones);          // column past k2: 0; the bias column k2: 1
    const Bf3 b3 = split_bf16x3(bv);
    frag_tile[lane] = __builtin_bit_cast(u32x4, b3.hi);
    frag_tile[64 + lane] = __builtin_bit_cast(u32x4, b3.mid);
    frag_tile[128 + lane] = __builtin_bit_cast(u32x4, b3.lo);
}
__device__ __forceinline__ void gw_mma(const Bf3& a3, const u32x4* frags, int lane, f32x16 (&acc)[GW_NT]) {
#pragma unroll
    for (int t = 0; t < GW_NT; ++t) {
        const u32x4* f = frags + (size_t)t * 3 * 64 + lane;
        const bf16x8 bh = __builtin_bit_cast(bf16x8, f[0]), bm = __builtin_bit_cast(bf16x8, f[64]), bl = __builtin_bit_cast(bf16x8, f[128]);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3.lo, bh, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3.hi, bl, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3.mid, bm, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3.mid, bh, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3.hi, bm, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3.hi, bh, acc[t], 0, 0, 0);
    }
}

// Phase profile (build with MSMP_PROF=gw; scripts/prof_gw.py): cycle sums of wave 0 of every 8th workgroup with at least 100 blocks
#if MSMP_PROF_GW
__device__ unsigned long long g_prof_gw[8];
#define GWP_DECL long long gp[5] = {0, 0, 0, 0, 0}; long long gt = __builtin_readcyclecounter();
#define GWP(i) do { const long long t_ = __builtin_readcyclecounter(); gp[i] += t_ - gt; gt = t_; } while (0)
#define GWP_FLUSH if (wave == 0 && lane == 0 && n_blocks >= 100 && (split & 7) == 0) { for (int i_ = 0; i_ < 5; ++i_) atomicAdd(&g_prof_gw[i_], (unsigned long long)gp[i_]); atomicAdd(&g_prof_gw[6], (unsigned long long)n_blocks); atomicAdd(&g_prof_gw[7], 1ull); }
#else
#define GWP_DECL
#define GWP(i)
#define GWP_FLUSH
#endif
__device__ __forceinline__ void grad_weight_body(const GradWeightJob& j, int split, int wave, int lane, u32x4* frags /* LDS [2][GW_FRAG_U4] */) {
    const int m = lane & 31, kk = lane >> 5;
    f32x16 acc[GW_NT];
#pragma unroll
    for (int t = 0; t < GW_NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int r0 = split * j.rows_per_split, r1 = min(r0 + j.rows_per_split, j.rows);
    const float* acol = j.a + 32 * wave + m;
    auto colptr = [&](int t, float& keep, float& ones, int& ld) {
        const int c = j.c0 + 32 * t + m;
        keep = c < j.k2 ? 1.0f : 0.f;
        ones = c == j.k2 ? 1.0f : 0.f;
        const bool second = j.b2 != nullptr && c >= j.ksplit && c < j.k2;      // the virtual concatenation [b | b2]
        ld = second ? j.ldb2 : j.ldb;
        return second ? j.b2 + (c - j.ksplit) : j.b + (c < j.k2 ? c : 0);
    };
    float keep, ones, keep4, ones4;
    int bld, bld4;
    const float* bcol = colptr(wave, keep, ones, bld);
    const float* bcol4 = colptr(4, keep4, ones4, bld4);
    const int n_blocks = (r1 - r0 + 15) / 16;            // the last one may be ragged: it takes the predicated loads
    const int n_full = (r1 - r0) / 16;
    GwRegs cur, nxt;
    auto load_block = [&](int blk, GwRegs& dst) {
        const int rb = r0 + 16 * blk + 8 * kk;
        if (blk < n_full) gw_load<true>(j, acol, bcol, bld, bcol4, bld4, (blk & 3) == wave, rb, 8, dst);
        else gw_load<false>(j, acol, bcol, bld, bcol4, bld4, (blk & 3) == wave, min(rb, r1 - 1), r1 - rb, dst);
    };
    GWP_DECL
    if (n_blocks > 0) load_block(0, cur);
    // The first block's values are pinned in registers HERE (an empty asm that "modifies" them: the loads must have landed).  Without it
    // the loop header inherits "loads pending on cur" from this prologue, and the wait the compiler places at the top of the loop for the
    // first trip (vmcnt(14) ... vmcnt(0) through the publish phase) is executed on EVERY trip -- where the youngest loads are the next
    // block's prefetch, issued a few instructions earlier: every block waited for its own prefetch (round 4 phase profile: 2 640 of
    // 5 000 cycles per block).
#pragma unroll
    for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(cur.a[i]), "+v"(cur.b[i]), "+v"(cur.b4[i]));
    __builtin_amdgcn_sched_barrier(0);
    for (int blk = 0; blk < n_blocks; ++blk) {
        if (blk + 1 < n_blocks) load_block(blk + 1, nxt);
        __builtin_amdgcn_sched_barrier(0);               // all loads of the next block are requested before this block's work
        GWP(0);
        u32x4* fb = frags + (size_t)(blk & 1) * GW_FRAG_U4;
        gw_publish(cur.b, keep, ones, fb + (size_t)wave * 3 * 64, lane);
        if ((blk & 3) == wave) gw_publish(cur.b4, keep4, ones4, fb + (size_t)4 * 3 * 64, lane);
        const Bf3 a3 = split_bf16x3(cur.a);
        GWP(1);
        __syncthreads();                                 // fragments of this block visible; the other buffer is free for the next block
        GWP(2);
        gw_mma(a3, fb, lane, acc);
        __builtin_amdgcn_sched_barrier(0);
        GWP(3);
#pragma unroll
        for (int i = 0; i < 8; ++i) { cur.a[i] = nxt.a[i]; cur.b[i] = nxt.b[i]; cur.b4[i] = nxt.b4[i]; }
    }
    GWP(4);
    GWP_FLUSH
    float* p = j.partial + (size_t)split * H * j.ldp + j.c0;
#pragma unroll
    for (int t = 0; t < GW_NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (j.c0 + 32 * t < j.ldp) p[(size_t)(32 * wave + acc_row(r, kk)) * j.ldp + 32 * t + m] = acc[t][r];
}

__global__ __launch_bounds__(256, 3) void grad_weight_kernel(GradWeightArgs a) {
    int ji = 0;
#pragma unroll
    for (int i = 1; i < GW_MAX_UNITS; ++i)
        if (i < a.n_units && (int)blockIdx.x >= a.unit[i].first_block) ji = i;
    const GradWeightJob& j = a.unit[ji];
    __shared__ u32x4 frags[2 * GW_FRAG_U4];              // 30 KB
    grad_weight_body(j, blockIdx.x - j.first_block, threadIdx.x >> 6, threadIdx.x & 63, frags);
}

// out[row][col] = sum over splits, in split order; grid.y = job
__global__ __launch_bounds__(256) void grad_weight_reduce_kernel(GradWeightArgs a) {
    const GradWeightJob& j = a.job[blockIdx.y];
    const int w = j.k2 + 1, ldp = j.ldp, total = H * w;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += gridDim.x * blockDim.x) {
        const int row = p / w, c = p - row * w;
        const float* src = j.partial + (size_t)row * ldp + c;
        float s = 0.f;
        for (int k = 0; k < j.splits; ++k) s += src[(size_t)k * H * ldp];
        if (c < j.k2) j.out_w[(size_t)row * j.k2 + c] = s;
        else j.out_b[row] = s;
    }
}

static int gw_tiles(int k2) { const int t = (k2 + 1 + 31) / 32; return t <= 5 ? 5 : t <= 9 ? 9 : t <= 10 ? 10 : -1; }
// rows per workgroup: 128, more once a pair would exceed its split limit (the partial products, splits x 128 x 32 nt floats, are
// written and re-read by the reduction).  Round 1 measured limits 128 / 256 / 512 with the fp32 kernel (E2 MSMP-PDE): batch 16
// 7.1 / 7.0 / 6.3 ms (the LEM pairs have 40 000 rows), batch 128 15.0 / 14.9 / 14.9, batch 512 51.1 / 49.7 / 48.9.
static int gw_rows_per_split(int64_t rows) {
    // small jobs keep up to 512 splits (they need the parallelism); large ones 128 (measured at batch 512, ms per iteration, cap
    // 512 / 256 / 128 / 64: 24.0 / 23.7 / 23.7 / 25.2: fewer partials to write and re-read until the splits no longer fill the chip)
    const int64_t lim = rows > 32768 ? 128 : 512;
    int64_t rps = 128;
    if ((rows + rps - 1) / rps > lim) rps = ((rows + lim - 1) / lim + 15) / 16 * 16;
    return (int)rps;
}

}  // namespace msmp

#if MSMP_PROF_GW
extern "C" __attribute__((visibility("default"))) int msmp_debug_prof_gw(unsigned long long* out8, int reset) {
    if (reset) { unsigned long long z[8] = {0}; return (int)hipMemcpyToSymbol(HIP_SYMBOL(msmp::g_prof_gw), z, sizeof(z)); }
    return (int)hipMemcpyFromSymbol(out8, HIP_SYMBOL(msmp::g_prof_gw), 8 * sizeof(unsigned long long));
}
#endif
extern "C" int64_t msmp_grad_weights_workspace_floats(int n_jobs, const int64_t* rows, const int* k2) {
    if (n_jobs < 1 || n_jobs > GW_MAX_JOBS || !rows || !k2) return -1;
    int64_t total = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const int nt = gw_tiles(k2[i]);
        if (nt < 0 || rows[i] < 1) return -1;
        const int rps = gw_rows_per_split(rows[i]);
        total += ((rows[i] + rps - 1) / rps) * H * 32 * nt;
    }
    return total;
}

namespace msmp {
// launches of msmp_grad_weights_f32 on validated arguments (also used by the layer backward below)
int launch_grad_weights(int n_jobs, const float* const* a, const float* const* b, const int64_t* rows, const int* lda,
                        const int* ldb, const int* k2, float* const* out_w, float* const* out_b, float* workspace,
                        int64_t workspace_floats, hipStream_t stream, const float* const* b2, const int* ldb2, const int* ksplit) {
    GradWeightArgs args;
    args.n_jobs = n_jobs;
    int64_t used = 0;
    int blocks = 0, max_w = 0, nu = 0;
    for (int i = 0; i < n_jobs; ++i) {
        MSMP_REQUIRE(a[i] && b[i] && out_w[i] && out_b[i], MSMP_ERR_ARG, "msmp_grad_weights_f32: null pointer in job %d", i);
        MSMP_REQUIRE(rows[i] >= 1 && rows[i] < (1L << 31) && k2[i] >= 1 && (ldb[i] >= k2[i] || (b2 && b2[i])) && lda[i] >= H, MSMP_ERR_ARG, "msmp_grad_weights_f32: bad sizes in job %d", i);
        const int nt = gw_tiles(k2[i]);
        MSMP_REQUIRE(nt > 0, MSMP_ERR_UNSUPPORTED, "msmp_grad_weights_f32: k2=%d > 319", k2[i]);
        GradWeightJob& j = args.job[i];
        j.a = a[i]; j.b = b[i]; j.out_w = out_w[i]; j.out_b = out_b[i]; j.partial = workspace + used;
        j.b2 = b2 ? b2[i] : nullptr; j.ldb2 = j.b2 ? ldb2[i] : 0; j.ksplit = j.b2 ? ksplit[i] : 0;
        MSMP_REQUIRE(!j.b2 || (j.ksplit >= 1 && j.ksplit < k2[i] && j.ldb2 >= k2[i] - j.ksplit && ldb[i] >= j.ksplit), MSMP_ERR_ARG, "msmp_grad_weights_f32: bad split of job %d", i);
        j.rows = (int)rows[i]; j.lda = lda[i]; j.ldb = ldb[i]; j.k2 = k2[i]; j.ldp = 32 * nt;
        j.rows_per_split = gw_rows_per_split(rows[i]);
        j.splits = (j.rows + j.rows_per_split - 1) / j.rows_per_split;
        j.first_block = 0; j.c0 = 0;
        for (int c0 = 0; c0 < 32 * nt; c0 += 32 * GW_NT) {
            GradWeightJob& u = args.unit[nu++];
            u = j; u.c0 = c0; u.first_block = blocks;
            blocks += j.splits;
        }
        used += (int64_t)j.splits * H * 32 * nt;
        max_w = k2[i] + 1 > max_w ? k2[i] + 1 : max_w;
    }
    args.n_units = nu;
    for (int i = n_jobs; i < GW_MAX_JOBS; ++i) args.job[i] = args.job[0];
    for (int i = nu; i < GW_MAX_UNITS; ++i) args.unit[i] = args.unit[0];
    MSMP_REQUIRE(used <= workspace_floats, MSMP_ERR_WORKSPACE, "msmp_grad_weights_f32: workspace of %ld floats, need %ld", (long)workspace_floats, (long)used);
    hipLaunchKernelGGL(grad_weight_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, args);
    hipLaunchKernelGGL(grad_weight_reduce_kernel, dim3((unsigned)((H * max_w + 255) / 256), (unsigned)n_jobs), dim3(256), 0, stream, args);
    return check_launch("grad_weight_kernel");
}
}  // namespace msmp

extern "C" int msmp_grad_weights_f32(int n_jobs, const float* const* a, const float* const* b, const int64_t* rows, const int* lda,
                                     const int* ldb, const int* k2, float* const* out_w, float* const* out_b, float* workspace,
                                     int64_t workspace_floats, msmp_stream_t stream) {
    MSMP_REQUIRE(n_jobs >= 1 && n_jobs <= GW_MAX_JOBS, MSMP_ERR_ARG, "msmp_grad_weights_f32: n_jobs=%d not in 1..%d", n_jobs, GW_MAX_JOBS);
    MSMP_REQUIRE(a && b && rows && lda && ldb && k2 && out_w && out_b && workspace, MSMP_ERR_ARG, "msmp_grad_weights_f32: null pointer");
    return launch_grad_weights(n_jobs, a, b, rows, lda, ldb, k2, out_w, out_b, workspace, workspace_floats, (hipStream_t)stream);
}

extern "C" int msmp_grad_weights_cat_f32(int n_jobs, const float* const* a, const float* const* b, const float* const* b2, const int64_t* rows,
                                         const int* lda, const int* ldb, const int* ldb2, const int* ksplit, const int* k2, float* const* out_w,
                                         float* const* out_b, float* workspace, int64_t workspace_floats, msmp_stream_t stream) {
    MSMP_REQUIRE(n_jobs >= 1 && n_jobs <= GW_MAX_JOBS, MSMP_ERR_ARG, "msmp_grad_weights_cat_f32: n_jobs=%d not in 1..%d", n_jobs, GW_MAX_JOBS);
    MSMP_REQUIRE(a && b && b2 && rows && lda && ldb && ldb2 && ksplit && k2 && out_w && out_b && workspace, MSMP_ERR_ARG, "msmp_grad_weights_cat_f32: null pointer");
    return launch_grad_weights(n_jobs, a, b, rows, lda, ldb, k2, out_w, out_b, workspace, workspace_floats, (hipStream_t)stream, b2, ldb2, ksplit);
}

// ==============================================================================================
// msmp_mp_layer_bwd_f32: the whole backward of one layer / one gated pair behind the C-ABI (the `_bwd` variant of
// msmp_mp_layer_f32): recompute in materialised form, the gated-blend / InstanceNorm backward, the
// data-gradient chain and the eight (sixteen) parameter gradients -- ~60 launches issued from native code instead of ~65
// library ops issued from Python (at the reference's batch of 16 graphs the host was the bound).  GEMMs with edge- or
// node-sized outputs go to rocBLAS (`rocblas_sgemm`, looked up at run time in the librocblas the process already has:
// inference never needs it); everything else is the kernels of this file.
// ==============================================================================================
#include <dlfcn.h>
#include <rocblas/rocblas.h>

namespace msmp {

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

unsigned grid_for(long work_items) {
    const long b = (work_items + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > 32768 ? 32768 : b);
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

// ----------------------------------------------------------------------------------------------------------------------
// Row GEMMs of the layer backward on the bf16 matrix pipe (round 2; they were rocblas_sgemm calls at 27 % of the fp32 MFMA peak
// plus separate bias / Swish / dSwish passes):   OUT[rows, 128] = epilogue( X[rows, K] W_eff^T ),  rows = E or N,  K <= 288.
// Products are fp32-exact (split_bf16x3: six bf16 MFMAs per K = 16 step).  A workgroup owns 128 rows (wave w: rows 32 w .. + 31 as the
// MFMA's A operand, a row per lane, its k slices loaded straight from the row); the weights come as pre-split fragments
// (rg_pack_kernel, once per backward call) streamed through LDS in 24-KB chunks of 32 k.  The output tile is
// [row][channel 4 c + T]: a lane owns four consecutive channels of 16 rows, so results, biases and the saved pre-activations of
// the fused epilogues move as 16-byte pieces of 512-byte rows.
//   EPI 0: a = acc + bias -> out0,  Swish(a) -> out1        (recompute of a hidden layer)
//   EPI 1: acc + bias -> out0                                (recompute of an output layer)
//   EPI 2: acc * Swish'(aux) -> out0                         (data gradient through a hidden layer)
//   EPI 3: acc -> out0                                       (data gradient w.r.t. the layer input; 256 columns = two launches)
//   EPI 4: Swish(acc + bias) -> out0                         (msmp_linear_swish_f32: the *2D classes' double_mlp)
//   EPI 5: out0 += acc                                       (node-level data gradient of the factorised message_net_1)
// ----------------------------------------------------------------------------------------------------------------------
// (RG_CHUNK_U4, RgPackJob, RgPackArgs: train_internal.h)
__global__ __launch_bounds__(256) void rg_pack_kernel(RgPackArgs a) {
    int ji = 0;
    for (int i = 1; i < a.n_jobs; ++i)
        if ((int)blockIdx.x >= a.job[i].first_block) ji = i;
    const RgPackJob& j = a.job[ji];
    const int id = (blockIdx.x - j.first_block) * 256 + threadIdx.x;      // ((chunk * 2 + s) * 4 + T) * 64 + lane
    if (id >= j.n_chunks * 2 * 4 * 64) return;
    const int lane = id & 63, T = (id >> 6) & 3, s = (id >> 8) & 1, chunk = id >> 9;
    const int c = lane & 31, hh = lane >> 5, o = 4 * c + T, k0 = 32 * chunk + 16 * s + 8 * hh;
    float v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int k = k0 + i;
        v[i] = (k < j.K && (j.transposed || j.col0 + o < j.n_rows)) ? (j.transposed ? j.w[(size_t)k * j.ldw + j.col0 + o] : j.w[(size_t)(j.col0 + o) * j.ldw + k]) : 0.f;
    }
    const Bf3 f = split_bf16x3(v);
    u32x4* dst = j.out + (size_t)(((chunk * 2 + s) * 4 + T) * 3) * 64 + lane;
    dst[0] = __builtin_bit_cast(u32x4, f.hi);
    dst[64] = __builtin_bit_cast(u32x4, f.mid);
    dst[128] = __builtin_bit_cast(u32x4, f.lo);
}

struct RgArgs {
    const float* x;      // [rows, ldx], columns 0..K-1 used (ldx a multiple of 4)
    const u32x4* wfrag;  // n_chunks chunks from rg_pack_kernel
    const float* bias;   // [128] (EPI 0, 1)
    const float* aux;    // [rows, 128] saved pre-activation (EPI 2)
    float* out0;         // [rows, ld0]
    float* out1;         // [rows, 128] (EPI 0)
    long rows;
    int ldx, K, n_chunks, ld0;
};

template <int EPI>
__global__ __launch_bounds__(256, 2) void rows_gemm_kernel(RgArgs a) {
    __shared__ __attribute__((aligned(16))) float wl[2 * RG_CHUNK_FLOATS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = lane & 31, hh = lane >> 5;
    const long row0 = (long)blockIdx.x * 128 + 32 * wave;
    const long xr = min(row0 + c, a.rows - 1);
    const float* xrow = a.x + (size_t)xr * a.ldx + 8 * hh;
    // this lane's slices of its row for chunk ch: k = 32 ch + 16 s + 8 hh .. + 7; pieces past K read as 0 (K need not be a multiple of 4)
    auto load_x = [&](int ch, f32x4 (&dst)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = 32 * ch + 16 * (i >> 1) + 8 * hh + 4 * (i & 1);
            if (k + 4 <= a.K) dst[i] = *reinterpret_cast<const f32x4*>(xrow + 32 * ch + 16 * (i >> 1) + 4 * (i & 1));
            else {
#pragma unroll
                for (int m = 0; m < 4; ++m) dst[i][m] = k + m < a.K ? xrow[32 * ch + 16 * (i >> 1) + 4 * (i & 1) + m] : 0.f;
            }
        }
    };
    f32x4 wreg[6];
    auto load_w = [&](int ch) {
        const f32x4* src = reinterpret_cast<const f32x4*>(a.wfrag) + (size_t)ch * RG_CHUNK_U4;
#pragma unroll
        for (int i = 0; i < 6; ++i) wreg[i] = src[tid + 256 * i];
    };
    auto store_w = [&](int buf) {
        f32x4* dst = reinterpret_cast<f32x4*>(wl + buf * RG_CHUNK_FLOATS);
#pragma unroll
        for (int i = 0; i < 6; ++i) dst[tid + 256 * i] = wreg[i];
    };
    f32x16 acc[4];
#pragma unroll
    for (int T = 0; T < 4; ++T)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[T][r] = 0.f;
    f32x4 xa[4], xb[4];
    load_w(0);
    load_x(0, xa);
    store_w(0);
    __syncthreads();
    auto chunk_mma = [&](const f32x4 (&xv)[4], int buf) {
        const u32x4* w = reinterpret_cast<const u32x4*>(wl + buf * RG_CHUNK_FLOATS) + lane;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const float v[8] = {xv[2 * s][0], xv[2 * s][1], xv[2 * s][2], xv[2 * s][3], xv[2 * s + 1][0], xv[2 * s + 1][1], xv[2 * s + 1][2], xv[2 * s + 1][3]};
            const Bf3 x3 = split_bf16x3(v);
#pragma unroll
            for (int T = 0; T < 4; ++T) {
                const u32x4* f = w + (size_t)((s * 4 + T) * 3) * 64;
                const bf16x8 whi = __builtin_bit_cast(bf16x8, f[0]), wmid = __builtin_bit_cast(bf16x8, f[64]), wlo = __builtin_bit_cast(bf16x8, f[128]);
                acc[T] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x3.lo, whi, acc[T], 0, 0, 0);
                acc[T] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x3.hi, wlo, acc[T], 0, 0, 0);
                acc[T] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x3.mid, wmid, acc[T], 0, 0, 0);
                acc[T] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x3.mid, whi, acc[T], 0, 0, 0);
                acc[T] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x3.hi, wmid, acc[T], 0, 0, 0);
                acc[T] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x3.hi, whi, acc[T], 0, 0, 0);
            }
        }
    };
    for (int ch = 0; ch < a.n_chunks; ch += 2) {
        if (ch + 1 < a.n_chunks) { load_w(ch + 1); load_x(ch + 1, xb); }
        chunk_mma(xa, 0);
        if (ch + 1 < a.n_chunks) {
            store_w(1);
            __syncthreads();
            if (ch + 2 < a.n_chunks) { load_w(ch + 2); load_x(ch + 2, xa); }
            chunk_mma(xb, 1);
            if (ch + 2 < a.n_chunks) {
                store_w(0);
                __syncthreads();
            }
        }
    }
    // ---- epilogue: lane c holds channels 4 c .. 4 c + 3 (tiles T = 0..3) of rows row0 + acc_row(r, hh) -----------------------
    f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
    if (EPI <= 1 || EPI == 4) bias4 = *reinterpret_cast<const f32x4*>(a.bias + 4 * c);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long row = row0 + acc_row(r, hh);
        if (row >= a.rows) continue;
        f32x4 v = {acc[0][r], acc[1][r], acc[2][r], acc[3][r]};
        if (EPI <= 1 || EPI == 4) v += bias4;
        if (EPI == 4) {
#pragma unroll
            for (int m = 0; m < 4; ++m) v[m] = swishf(v[m]);
        }
        if (EPI == 2) {
            const f32x4 pre = *reinterpret_cast<const f32x4*>(a.aux + (size_t)row * H + 4 * c);
#pragma unroll
            for (int m = 0; m < 4; ++m) v[m] *= dswish(pre[m]);
        }
        if (EPI == 5) v += *reinterpret_cast<const f32x4*>(a.out0 + (size_t)row * a.ld0 + 4 * c);
        *reinterpret_cast<f32x4*>(a.out0 + (size_t)row * a.ld0 + 4 * c) = v;
        if (EPI == 0) {
            f32x4 sw;
#pragma unroll
            for (int m = 0; m < 4; ++m) sw[m] = swishf(v[m]);
            *reinterpret_cast<f32x4*>(a.out1 + (size_t)row * H + 4 * c) = sw;
        }
    }
}

// Small-batch edition (round 3; VERDICT r02 item 6a: below 32 768 rows the 128-row workgroups above fill a fraction of the chip
// and the layer backward went to rocblas_sgemm): a workgroup owns 32 rows and its four waves split the OUTPUT: wave w computes
// channel tile T = w (the channels 4 c + w of the dealt fragment layout) of the same 32 rows -- a quarter of the MFMAs per wave,
// four times the workgroups, the wave's weight fragments straight from the L2-resident pack (6 x 16 bytes per lane and chunk),
// no LDS, no barrier.  Same fragments, same arithmetic order per output element as rows_gemm_kernel: bit-identical results.
template <int EPI>
__global__ __launch_bounds__(256) void rows_gemm_small_kernel(RgArgs a) {
    const int tid = threadIdx.x, lane = tid & 63;
    const int T = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5;
    const long row0 = (long)blockIdx.x * 32;
    const long xr = min(row0 + c, a.rows - 1);
    const float* xrow = a.x + (size_t)xr * a.ldx + 8 * hh;
    auto load_x = [&](int ch, f32x4 (&dst)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = 32 * ch + 16 * (i >> 1) + 8 * hh + 4 * (i & 1);
            if (k + 4 <= a.K) dst[i] = *reinterpret_cast<const f32x4*>(xrow + 32 * ch + 16 * (i >> 1) + 4 * (i & 1));
            else {
#pragma unroll
                for (int m = 0; m < 4; ++m) dst[i][m] = k + m < a.K ? xrow[32 * ch + 16 * (i >> 1) + 4 * (i & 1) + m] : 0.f;
            }
        }
    };
    auto load_w = [&](int ch, u32x4 (&dst)[6]) {
        const u32x4* src = a.wfrag + (size_t)ch * RG_CHUNK_U4 + lane;
#pragma unroll
        for (int s = 0; s < 2; ++s)
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) dst[3 * s + pl] = src[(size_t)((s * 4 + T) * 3 + pl) * 64];
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    f32x4 xa[4], xb[4];
    u32x4 wa[6], wb[6];
    auto chunk_mma = [&](const f32x4 (&xv)[4], const u32x4 (&w)[6]) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const float v[8] = {xv[2 * s][0], xv[2 * s][1], xv[2 * s][2], xv[2 * s][3], xv[2 * s + 1][0], xv[2 * s + 1][1], xv[2 * s + 1][2], xv[2 * s + 1][3]};
            const Bf3 x3 = split_bf16x3(v);
            const bf16x8 whi = __builtin_bit_cast(bf16x8, w[3 * s]), wmid = __builtin_bit_cast(bf16x8, w[3 * s + 1]), wlo = __builtin_bit_cast(bf16x8, w[3 * s + 2]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x3.lo, whi, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x3.hi, wlo, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x3.mid, wmid, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x3.mid, whi, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x3.hi, wmid, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(x3.hi, whi, acc, 0, 0, 0);
        }
    };
    load_w(0, wa);
    load_x(0, xa);
    for (int ch = 0; ch < a.n_chunks; ch += 2) {
        if (ch + 1 < a.n_chunks) { load_w(ch + 1, wb); load_x(ch + 1, xb); }
        chunk_mma(xa, wa);
        if (ch + 1 < a.n_chunks) {
            if (ch + 2 < a.n_chunks) { load_w(ch + 2, wa); load_x(ch + 2, xa); }
            chunk_mma(xb, wb);
        }
    }
    // epilogue: lane c holds channel 4 c + T of rows row0 + acc_row(r, hh)
    const int chn = 4 * c + T;
    float bias1 = 0.f;
    if (EPI <= 1 || EPI == 4) bias1 = a.bias[chn];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const long row = row0 + acc_row(r, hh);
        if (row >= a.rows) continue;
        float v = acc[r];
        if (EPI <= 1 || EPI == 4) v += bias1;
        if (EPI == 4) v = swishf(v);
        if (EPI == 2) v *= dswish(a.aux[(size_t)row * H + chn]);
        if (EPI == 5) v += a.out0[(size_t)row * a.ld0 + chn];
        a.out0[(size_t)row * a.ld0 + chn] = v;
        if (EPI == 0) a.out1[(size_t)row * H + chn] = swishf(v);
    }
}

constexpr long RG_SMALL_ROWS = 32768;      // below this many rows the 32-row workgroups fill the chip better (294 x 4 waves at E = 9 408)

int rows_gemm(int epi, const float* x, int ldx, long rows, int K, const u32x4* wfrag, const float* bias, const float* aux, float* out0,
              int ld0, float* out1, hipStream_t st) {
    RgArgs a{x, wfrag, bias, aux, out0, out1, rows, ldx, K, (K + 31) / 32, ld0};
    if (rows < RG_SMALL_ROWS) {
        const dim3 gs((unsigned)((rows + 31) / 32));
        switch (epi) {
            case 0: hipLaunchKernelGGL(rows_gemm_small_kernel<0>, gs, dim3(256), 0, st, a); break;
            case 1: hipLaunchKernelGGL(rows_gemm_small_kernel<1>, gs, dim3(256), 0, st, a); break;
            case 2: hipLaunchKernelGGL(rows_gemm_small_kernel<2>, gs, dim3(256), 0, st, a); break;
            case 4: hipLaunchKernelGGL(rows_gemm_small_kernel<4>, gs, dim3(256), 0, st, a); break;
            case 5: hipLaunchKernelGGL(rows_gemm_small_kernel<5>, gs, dim3(256), 0, st, a); break;
            default: hipLaunchKernelGGL(rows_gemm_small_kernel<3>, gs, dim3(256), 0, st, a); break;
        }
        return check_launch("rows_gemm_small_kernel");
    }
    const dim3 grid((unsigned)((rows + 127) / 128));
    switch (epi) {
        case 0: hipLaunchKernelGGL(rows_gemm_kernel<0>, grid, dim3(256), 0, st, a); break;
        case 1: hipLaunchKernelGGL(rows_gemm_kernel<1>, grid, dim3(256), 0, st, a); break;
        case 2: hipLaunchKernelGGL(rows_gemm_kernel<2>, grid, dim3(256), 0, st, a); break;
        case 4: hipLaunchKernelGGL(rows_gemm_kernel<4>, grid, dim3(256), 0, st, a); break;
        case 5: hipLaunchKernelGGL(rows_gemm_kernel<5>, grid, dim3(256), 0, st, a); break;
        default: hipLaunchKernelGGL(rows_gemm_kernel<3>, grid, dim3(256), 0, st, a); break;
    }
    return check_launch("rows_gemm_kernel");
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
void add_pack(RgPackArgs& a, int& blocks, const float* w, int ldw, int K, int col0, int transposed, u32x4* out) {
    RgPackJob& j = a.job[a.n_jobs++];
    j.w = w; j.out = out; j.ldw = ldw; j.K = K; j.n_chunks = (K + 31) / 32; j.col0 = col0; j.transposed = transposed; j.first_block = blocks;
    j.n_rows = 0x7fffffff;
    blocks += (j.n_chunks * 512 + 255) / 256;
}
// the split launch for the jobs collected by add_pack (for callers outside this file: train_internal.h)
int launch_rg_pack(RgPackArgs& a, int blocks, hipStream_t st) {
    for (int i = a.n_jobs; i < RG_MAX_PACK; ++i) a.job[i] = a.job[0];
    hipLaunchKernelGGL(rg_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return check_launch("rg_pack_kernel");
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
#define RC(call) do { const int rc_ = (call); if (rc_) return rc_; } while (0)

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

// Swish(x W^T + b) for a row-major x [rows, k] and a Linear weight w [n_out, k] (n_out a multiple of 128, k <= 288 a multiple of 4):
// the `double_mlp` of the *2D solver classes (experiments/models_gnn2D.py:66-70: Linear(128, 256) + Swish + Unflatten) on the row-GEMM
// kernel above (fp32-exact bf16x3 products), one launch per 128 output columns after one weight-split launch.
extern "C" size_t msmp_linear_swish_workspace_bytes(int k, int n_out) {
    if (k < 4 || k > 288 || k % 4 || n_out < 128 || n_out % 128 || n_out > 128 * RG_MAX_PACK) return 0;
    return (size_t)(n_out / 128) * ((k + 31) / 32) * RG_CHUNK_U4 * sizeof(u32x4) + 256;
}
extern "C" int msmp_linear_swish_f32(const float* x, int64_t rows, int k, const float* w, const float* bias, int n_out, float* out,
                                     void* workspace, size_t workspace_bytes, msmp_stream_t stream) {
    MSMP_REQUIRE(x && w && bias && out && workspace, MSMP_ERR_ARG, "msmp_linear_swish_f32: null pointer");
    const size_t need = msmp_linear_swish_workspace_bytes(k, n_out);
    MSMP_REQUIRE(need, MSMP_ERR_UNSUPPORTED, "msmp_linear_swish_f32: k = %d (a multiple of 4 up to 288), n_out = %d (a multiple of 128 up to %d)", k, n_out, 128 * RG_MAX_PACK);
    MSMP_REQUIRE(rows > 0 && rows < (1L << 31), MSMP_ERR_ARG, "msmp_linear_swish_f32: bad rows");
    MSMP_REQUIRE(workspace_bytes >= need, MSMP_ERR_WORKSPACE, "msmp_linear_swish_f32: workspace %zu < %zu", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    u32x4* fp = reinterpret_cast<u32x4*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    const int groups = n_out / 128, chunks = (k + 31) / 32;
    RgPackArgs pa;
    pa.n_jobs = 0;
    int blocks = 0;
    for (int g = 0; g < groups; ++g) add_pack(pa, blocks, w, k, k, 128 * g, 0, fp + (size_t)g * chunks * RG_CHUNK_U4);
    for (int i = pa.n_jobs; i < RG_MAX_PACK; ++i) pa.job[i] = pa.job[0];
    hipLaunchKernelGGL(rg_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, pa);
    RC(check_launch("rg_pack_kernel"));
    for (int g = 0; g < groups; ++g)
        RC(rows_gemm(4, x, k, (long)rows, k, fp + (size_t)g * chunks * RG_CHUNK_U4, bias + 128 * g, nullptr, out + 128 * g, n_out, nullptr, st));
    return MSMP_OK;
}

// General row GEMM of the width-generic layer path (the GLU classes, hidden width 164: experiments/models_gnn.py:1379-1523,
// models_gnn2D.py:1198-1366):  out[rows, 0:128 g] = f(x[rows, 0:k] w[n_out, k]^T + bias)  in 128-column groups on the fp32-exact bf16x3
// row-GEMM kernel above; columns n_out .. 128 ceil(n_out / 128) - 1 of `out` are written too (as f(0 + 0)): ld_out must cover them.
//   mode 0: acc + bias    1: Swish(acc + bias)    2: out += acc (bias ignored)
extern "C" size_t msmp_linear_workspace_bytes(int k, int n_out) {
    if (k < 1 || k > 1024 || n_out < 1 || n_out > 128 * (RG_MAX_PACK / 2)) return 0;
    const int groups = (n_out + 127) / 128;
    return (size_t)groups * ((k + 31) / 32) * RG_CHUNK_U4 * sizeof(u32x4) + (size_t)groups * 128 * sizeof(float) + 512;
}
__global__ void linear_pad_bias_kernel(const float* __restrict__ bias, int n_out, int n_pad, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n_pad) out[i] = (bias && i < n_out) ? bias[i] : 0.f;
}
extern "C" int msmp_linear_f32(const float* x, int ldx, int64_t rows, int k, const float* w, int ldw, const float* bias, int n_out, int mode,
                               float* out, int ld_out, void* workspace, size_t workspace_bytes, msmp_stream_t stream) {
    MSMP_REQUIRE(x && w && out && workspace, MSMP_ERR_ARG, "msmp_linear_f32: null pointer");
    MSMP_REQUIRE(mode >= 0 && mode <= 2, MSMP_ERR_ARG, "msmp_linear_f32: mode %d", mode);
    const size_t need = msmp_linear_workspace_bytes(k, n_out);
    MSMP_REQUIRE(need, MSMP_ERR_UNSUPPORTED, "msmp_linear_f32: k = %d (1..1024), n_out = %d (1..%d)", k, n_out, 128 * (RG_MAX_PACK / 2));
    const int groups = (n_out + 127) / 128, chunks = (k + 31) / 32;
    MSMP_REQUIRE(rows > 0 && rows < (1L << 31) && ldx >= k && ldx % 4 == 0 && ldw >= k && ld_out >= 128 * groups && ld_out % 4 == 0 &&
                 ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 15) == 0, MSMP_ERR_ARG,
                 "msmp_linear_f32: bad sizes (ldx, ld_out multiples of 4, 16-byte aligned rows, ld_out >= %d)", 128 * groups);
    MSMP_REQUIRE(workspace_bytes >= need, MSMP_ERR_WORKSPACE, "msmp_linear_f32: workspace %zu < %zu", workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    u32x4* fp = reinterpret_cast<u32x4*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    float* bpad = reinterpret_cast<float*>(fp + (size_t)groups * chunks * RG_CHUNK_U4);
    RgPackArgs pa;
    pa.n_jobs = 0;
    int blocks = 0;
    for (int g = 0; g < groups; ++g) {
        add_pack(pa, blocks, w, ldw, k, 128 * g, 0, fp + (size_t)g * chunks * RG_CHUNK_U4);
        pa.job[pa.n_jobs - 1].n_rows = n_out;
    }
    for (int i = pa.n_jobs; i < RG_MAX_PACK; ++i) pa.job[i] = pa.job[0];
    hipLaunchKernelGGL(rg_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, pa);
    RC(check_launch("rg_pack_kernel"));
    hipLaunchKernelGGL(linear_pad_bias_kernel, dim3((unsigned)((128 * groups + 255) / 256)), dim3(256), 0, st, mode == 2 ? nullptr : bias, n_out, 128 * groups, bpad);
    RC(check_launch("linear_pad_bias_kernel"));
    const int epi = mode == 0 ? 1 : (mode == 1 ? 4 : 5);
    for (int g = 0; g < groups; ++g)
        RC(rows_gemm(epi, x, ldx, (long)rows, k, fp + (size_t)g * chunks * RG_CHUNK_U4, bpad + 128 * g, nullptr, out + 128 * g, ld_out, nullptr, st));
    return MSMP_OK;
}

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
        for (int i = pa.n_jobs; i < RG_MAX_PACK; ++i) pa.job[i] = pa.job[0];
        hipLaunchKernelGGL(rg_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, pa);
        RC(check_launch("rg_pack_kernel"));
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

// ------------------------------------------------------------------------------------------------------------------------
// Deterministic reductions for the pieces of a training iteration that stay in PyTorch (encoder / decoder bias gradients, the loss
// sum, experiments/train_helper.py:125-141): two launches each, partial sums in a caller's workspace, fixed order, no atomics and
// no zero-initialised semaphore -- a library reduction's hipMemsetAsync becomes a memset NODE in a captured training step and was
// seen to replay out of order.
// ------------------------------------------------------------------------------------------------------------------------
namespace msmp {
constexpr int RED_BLOCKS = 128;
// partial[b][c] = sum of x[r][c] over the rows of block b
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ x, long rows, int cols, float* __restrict__ partial) {
    const long per = (rows + gridDim.x - 1) / gridDim.x;
    const long r0 = (long)blockIdx.x * per, r1 = min(r0 + per, rows);
    for (int c = threadIdx.x; c < cols; c += 256) {
        float s = 0.f;
        for (long r = r0; r < r1; ++r) s += x[(size_t)r * cols + c];
        partial[(size_t)blockIdx.x * cols + c] = s;
    }
}
__device__ __forceinline__ float block_sum_256(float v, float* red) {       // fixed tree, every thread returns the total
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}
// out[j] = sum over blocks and over the `group` consecutive columns of output j: one workgroup per output, element (b, g) of the
// blocks x group set at thread (b group + g) % 256 -- fixed order, then the fixed tree
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* __restrict__ partial, int blocks, int cols, int group, float* __restrict__ out) {
    __shared__ float red[256];
    const int j = blockIdx.x;
    float s = 0.f;
    for (int i = threadIdx.x; i < blocks * group; i += 256) s += partial[(size_t)(i / group) * cols + j * group + i % group];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) out[j] = s;
}
__global__ __launch_bounds__(256) void sqerr_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, float* __restrict__ partial) {
    __shared__ float red[256];
    float s = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float d = a[i] - b[i];
        s = fmaf(d, d, s);
    }
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void sum_final_kernel(const float* __restrict__ partial, int n, float* __restrict__ out) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) out[0] = s;
}
}  // namespace msmp

extern "C" size_t msmp_reduce_workspace_bytes(int cols) { return (size_t)RED_BLOCKS * (size_t)(cols > 1 ? cols : 1) * sizeof(float); }

extern "C" int msmp_colsum_f32(const float* x, int64_t rows, int cols, int group, float* out, void* workspace, size_t workspace_bytes,
                               msmp_stream_t stream) {
    MSMP_REQUIRE(x && out && workspace, MSMP_ERR_ARG, "msmp_colsum_f32: null pointer");
    MSMP_REQUIRE(rows >= 0 && cols >= 1 && group >= 1 && cols % group == 0, MSMP_ERR_ARG, "msmp_colsum_f32: bad sizes");
    MSMP_REQUIRE(workspace_bytes >= msmp_reduce_workspace_bytes(cols), MSMP_ERR_WORKSPACE, "msmp_colsum_f32: workspace %zu < %zu", workspace_bytes,
                 msmp_reduce_workspace_bytes(cols));
    const int blocks = (int)(rows < RED_BLOCKS ? (rows > 0 ? rows : 1) : RED_BLOCKS);
    hipLaunchKernelGGL(colsum_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, (long)rows, cols, (float*)workspace);
    hipLaunchKernelGGL(colsum_final_kernel, dim3((unsigned)(cols / group)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, blocks,
                       cols, group, out);
    return check_launch("colsum_kernel");
}

extern "C" int msmp_sqerr_sum_f32(const float* a, const float* b, int64_t n, float* out, void* workspace, size_t workspace_bytes,
                                  msmp_stream_t stream) {
    MSMP_REQUIRE(a && b && out && workspace, MSMP_ERR_ARG, "msmp_sqerr_sum_f32: null pointer");
    MSMP_REQUIRE(n >= 0 && workspace_bytes >= msmp_reduce_workspace_bytes(1), MSMP_ERR_ARG, "msmp_sqerr_sum_f32: bad sizes / workspace");
    hipLaunchKernelGGL(sqerr_partial_kernel, dim3(RED_BLOCKS), dim3(256), 0, (hipStream_t)stream, a, b, (long)n, (float*)workspace);
    hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, RED_BLOCKS, out);
    return check_launch("sqerr_sum_kernel");
}

// ------------------------------------------------------------------------------------------------------------------------
// Fused AdamW (experiments/train.py:410: optim.AdamW(model.parameters(), lr)): every parameter tensor of the model in one or two
// launches.  A launch carries up to ADAMW_MAX_TENSORS tensor descriptors in its kernel arguments; block b works on chunk
// (b - first_block[t]) of tensor t.  Decoupled weight decay, bias-corrected moments, the same order of operations as
// torch.optim.AdamW (p *= 1 - lr wd;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)).
// ------------------------------------------------------------------------------------------------------------------------
namespace msmp {
constexpr int ADAMW_MAX_TENSORS = 48;
constexpr int ADAMW_CHUNK = 4096;           // elements per block (256 threads x 4 x 4)
struct AdamWArgs {
    float* p[ADAMW_MAX_TENSORS];
    const float* g[ADAMW_MAX_TENSORS];
    float* m[ADAMW_MAX_TENSORS];
    float* v[ADAMW_MAX_TENSORS];
    int numel[ADAMW_MAX_TENSORS];
    int first_block[ADAMW_MAX_TENSORS + 1];
    int n;
    float lr, beta1, beta2, eps, decay, bc1_inv, bc2_rsqrt;      // decay = 1 - lr wd;  bc1_inv = 1 / (1 - b1^t);  bc2_rsqrt = 1 / sqrt(1 - b2^t)
    // capturable form (a hipGraph replays the same kernel arguments): step count and learning rate are read from device memory
    const long long* step_dev;
    const float* lr_dev;
    float weight_decay;
    const int* verdict_dev;     // guarded form only (msmp_adamw_guarded_f32): a non-zero word leaves every tensor alone
};

__global__ void adamw_advance_kernel(long long* step) {
    if (threadIdx.x == 0 && blockIdx.x == 0) step[0] += 1;
}

template <bool DEV, bool GUARD = false>
__global__ __launch_bounds__(256) void adamw_kernel(AdamWArgs a) {
    if (GUARD && a.verdict_dev[0] != 0) return;          // uniform over the grid: the same word for every block
    int t = 0;
    while (t + 1 < a.n && (int)blockIdx.x >= a.first_block[t + 1]) ++t;
    const int base = ((int)blockIdx.x - a.first_block[t]) * ADAMW_CHUNK;
    const int n = a.numel[t];
    float* __restrict__ p = a.p[t];
    const float* __restrict__ g = a.g[t];
    float* __restrict__ m = a.m[t];
    float* __restrict__ v = a.v[t];
    if (DEV) {          // the host entry's arithmetic, per block (two pow calls: nothing beside 4096 elements)
        const double st = (double)a.step_dev[0];
        a.lr = a.lr_dev[0];
        a.decay = 1.0f - a.lr * a.weight_decay;
        a.bc1_inv = (float)(1.0 / (1.0 - pow((double)a.beta1, st)));
        a.bc2_rsqrt = (float)(1.0 / sqrt(1.0 - pow((double)a.beta2, st)));
    }
    const float step = a.lr * a.bc1_inv;
#pragma unroll
    for (int k = 0; k < ADAMW_CHUNK / 256; ++k) {
        const int i = base + k * 256 + threadIdx.x;
        if (i < n) {
            const float gi = g[i];
            const float mi = a.beta1 * m[i] + (1.0f - a.beta1) * gi;
            const float vi = a.beta2 * v[i] + (1.0f - a.beta2) * gi * gi;
            m[i] = mi;
            v[i] = vi;
            p[i] = p[i] * a.decay - step * (mi / (sqrtf(vi) * a.bc2_rsqrt + a.eps));
        }
    }
}
}  // namespace msmp

static int adamw_launch(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                        float* const* exp_avg_sq, const int64_t* numel, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int64_t step, int64_t* step_dev, const float* lr_dev, msmp_stream_t stream,
                        const int* verdict_dev = nullptr);

extern "C" int msmp_adamw_f32(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                              float* const* exp_avg_sq, const int64_t* numel, float lr, float beta1, float beta2, float eps,
                              float weight_decay, int64_t step, msmp_stream_t stream) {
    MSMP_REQUIRE(step >= 1, MSMP_ERR_ARG, "msmp_adamw_f32: bad hyper-parameters");
    return adamw_launch(n_tensors, params, grads, exp_avg, exp_avg_sq, numel, lr, beta1, beta2, eps, weight_decay, step, nullptr, nullptr, stream);
}

extern "C" int msmp_adamw_capturable_f32(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                                         float* const* exp_avg_sq, const int64_t* numel, const float* lr_dev, float beta1, float beta2,
                                         float eps, float weight_decay, int64_t* step_dev, msmp_stream_t stream) {
    MSMP_REQUIRE(lr_dev && step_dev, MSMP_ERR_ARG, "msmp_adamw_capturable_f32: null pointer");
    hipLaunchKernelGGL(adamw_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long*)step_dev);
    return adamw_launch(n_tensors, params, grads, exp_avg, exp_avg_sq, numel, 0.f, beta1, beta2, eps, weight_decay, 1, step_dev, lr_dev, stream);
}

static int adamw_launch(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                        float* const* exp_avg_sq, const int64_t* numel, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int64_t step, int64_t* step_dev, const float* lr_dev, msmp_stream_t stream,
                        const int* verdict_dev) {
    MSMP_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || (params && grads && exp_avg && exp_avg_sq && numel)), MSMP_ERR_ARG, "msmp_adamw_f32: null pointer");
    MSMP_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, MSMP_ERR_ARG, "msmp_adamw_f32: bad hyper-parameters");
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    for (int t0 = 0; t0 < n_tensors; t0 += ADAMW_MAX_TENSORS) {
        AdamWArgs a;
        a.n = n_tensors - t0 < ADAMW_MAX_TENSORS ? n_tensors - t0 : ADAMW_MAX_TENSORS;
        int blocks = 0;
        for (int i = 0; i < a.n; ++i) {
            MSMP_REQUIRE(params[t0 + i] && grads[t0 + i] && exp_avg[t0 + i] && exp_avg_sq[t0 + i] && numel[t0 + i] >= 0 && numel[t0 + i] < (1L << 31),
                         MSMP_ERR_ARG, "msmp_adamw_f32: bad tensor %d", t0 + i);
            a.p[i] = params[t0 + i]; a.g[i] = grads[t0 + i]; a.m[i] = exp_avg[t0 + i]; a.v[i] = exp_avg_sq[t0 + i];
            a.numel[i] = (int)numel[t0 + i];
            a.first_block[i] = blocks;
            blocks += (int)((numel[t0 + i] + ADAMW_CHUNK - 1) / ADAMW_CHUNK);
        }
        a.first_block[a.n] = blocks;
        a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.decay = 1.0f - lr * weight_decay;
        a.bc1_inv = (float)(1.0 / bc1); a.bc2_rsqrt = (float)(1.0 / sqrt(bc2));
        a.step_dev = (const long long*)step_dev; a.lr_dev = lr_dev; a.weight_decay = weight_decay; a.verdict_dev = verdict_dev;
        if (blocks && step_dev && verdict_dev) hipLaunchKernelGGL((adamw_kernel<true, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
        else if (blocks && step_dev) hipLaunchKernelGGL(adamw_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
        else if (blocks) hipLaunchKernelGGL(adamw_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    }
    return check_launch("adamw_kernel");
}

// ------------------------------------------------------------------------------------------------------------------------
// The guard of a training step (experiments/train_helper.py:125-141 has none: the reference has no input range to leave).  A
// non-finite loss gives non-finite gradients, and AdamW writes them into every weight and both moments; these three entries let
// the step refuse such an update without a host read-back, so a captured step stays one graph:
//   msmp_status_poison_f32    the sticky range status becomes a NaN in the loss scalar (every rank of a data-parallel step then
//                             sees it through the scalar all-reduce it makes anyway);
//   msmp_grads_finite_f32     one int32 verdict over all gradients and a few watched scalars, by the rules of the reductions
//                             above: every block overwrites its own workspace slot, a final block overwrites the verdict;
//   msmp_adamw_guarded_f32    msmp_adamw_capturable_f32 that leaves everything alone, and counts, when the verdict is not 0.
// ------------------------------------------------------------------------------------------------------------------------
namespace msmp {
constexpr int FINITE_MAX_SCALARS = 4;
struct FiniteArgs {
    const float* g[ADAMW_MAX_TENSORS];
    int numel[ADAMW_MAX_TENSORS];
    int first_block[ADAMW_MAX_TENSORS + 1];
    int n;
    int* slots;          // this launch's part of the workspace: one word per block
};
struct FiniteScalars {
    const float* s[FINITE_MAX_SCALARS];
    int n;
};

__device__ __forceinline__ int nonfinite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }      // exponent all ones: NaN, +-Inf

// slot[block] = 1 if one of the block's 4096 elements is NaN or +-Inf, else 0 (written either way: nothing is zeroed beforehand)
__global__ __launch_bounds__(256) void finite_partial_kernel(FiniteArgs a) {
    int t = 0;
    while (t + 1 < a.n && (int)blockIdx.x >= a.first_block[t + 1]) ++t;
    const int base = ((int)blockIdx.x - a.first_block[t]) * ADAMW_CHUNK;
    const int n = a.numel[t];
    const float* __restrict__ g = a.g[t];
    int bad = 0;
#pragma unroll
    for (int k = 0; k < ADAMW_CHUNK / 256; ++k) {
        const int i = base + k * 256 + threadIdx.x;
        if (i < n) bad |= nonfinite_bits(g[i]);
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) a.slots[blockIdx.x] = bad ? 1 : 0;
}

// verdict[0] = (any slot set ? GRAD : 0) | (any watched scalar non-finite ? SCALAR : 0), overwritten on every run
__global__ __launch_bounds__(256) void finite_final_kernel(const int* __restrict__ slots, int n_slots, FiniteScalars sc, int* __restrict__ verdict) {
    int bad = 0;
    for (int i = threadIdx.x; i < n_slots; i += 256) bad |= slots[i];
    bad = __syncthreads_or(bad);
    int sbad = 0;
    if ((int)threadIdx.x < sc.n) sbad = nonfinite_bits(sc.s[threadIdx.x][0]);
    sbad = __syncthreads_or(sbad);
    if (threadIdx.x == 0) verdict[0] = (bad ? MSMP_NONFINITE_GRAD : 0) | (sbad ? MSMP_NONFINITE_SCALAR : 0);
}

// the guarded form of adamw_advance_kernel: a refused step advances the other counter
__global__ void adamw_advance_guarded_kernel(long long* step, const int* verdict, long long* skipped) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        if (verdict[0] == 0) step[0] += 1;
        else skipped[0] += 1;
    }
}

// scalar[0] = NaN if the status word is raised (system scope: the word may be host memory, and the forward's kernels raised it with
// system-scope atomic ORs earlier in this stream)
__global__ __launch_bounds__(64) void status_poison_kernel(const int* status, float* scalar) {
    if (threadIdx.x == 0 && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) scalar[0] = __uint_as_float(0x7fc00000u);
}

static int64_t finite_blocks(int n_tensors, const int64_t* numel) {
    int64_t blocks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (numel[i] < 0 || numel[i] >= (1L << 31)) return -1;
        blocks += (numel[i] + ADAMW_CHUNK - 1) / ADAMW_CHUNK;
    }
    return blocks;
}
}  // namespace msmp

extern "C" size_t msmp_grads_finite_workspace_bytes(int n_tensors, const int64_t* numel) {
    if (n_tensors < 0 || (n_tensors > 0 && !numel)) return 0;
    const int64_t blocks = finite_blocks(n_tensors, numel);
    return blocks < 0 ? 0 : (size_t)(blocks > 0 ? blocks : 1) * sizeof(int);
}

extern "C" int msmp_grads_finite_f32(int n_tensors, const float* const* grads, const int64_t* numel, int n_scalars, const float* const* scalars,
                                     int32_t* verdict_dev, void* workspace, size_t workspace_bytes, msmp_stream_t stream) {
    MSMP_REQUIRE(n_tensors >= 0 && n_scalars >= 0 && n_scalars <= FINITE_MAX_SCALARS, MSMP_ERR_ARG,
                 "msmp_grads_finite_f32: bad counts (n_tensors=%d, n_scalars=%d not in 0..%d)", n_tensors, n_scalars, FINITE_MAX_SCALARS);
    MSMP_REQUIRE(verdict_dev && workspace && (n_tensors == 0 || (grads && numel)) && (n_scalars == 0 || scalars), MSMP_ERR_ARG,
                 "msmp_grads_finite_f32: null pointer");
    FiniteScalars sc;
    sc.n = n_scalars;
    for (int i = 0; i < FINITE_MAX_SCALARS; ++i) {
        MSMP_REQUIRE(i >= n_scalars || scalars[i], MSMP_ERR_ARG, "msmp_grads_finite_f32: null pointer (scalar %d)", i);
        sc.s[i] = i < n_scalars ? scalars[i] : nullptr;
    }
    for (int i = 0; i < n_tensors; ++i)
        MSMP_REQUIRE((grads[i] || numel[i] == 0) && numel[i] >= 0 && numel[i] < (1L << 31), MSMP_ERR_ARG,       // an empty tensor is never read
                     "msmp_grads_finite_f32: bad tensor %d (null pointer or element count)", i);
    const int64_t total = finite_blocks(n_tensors, numel);
    MSMP_REQUIRE(total < (1L << 31), MSMP_ERR_ARG, "msmp_grads_finite_f32: bad sizes (%ld chunks)", (long)total);
    MSMP_REQUIRE(workspace_bytes >= msmp_grads_finite_workspace_bytes(n_tensors, numel), MSMP_ERR_WORKSPACE, "msmp_grads_finite_f32: workspace %zu < %zu",
                 workspace_bytes, msmp_grads_finite_workspace_bytes(n_tensors, numel));
    int* slots = static_cast<int*>(workspace);
    int used = 0;
    for (int t0 = 0; t0 < n_tensors; t0 += ADAMW_MAX_TENSORS) {
        FiniteArgs a;
        a.n = n_tensors - t0 < ADAMW_MAX_TENSORS ? n_tensors - t0 : ADAMW_MAX_TENSORS;
        int blocks = 0;
        for (int i = 0; i < a.n; ++i) {
            a.g[i] = grads[t0 + i];
            a.numel[i] = (int)numel[t0 + i];
            a.first_block[i] = blocks;
            blocks += (int)((numel[t0 + i] + ADAMW_CHUNK - 1) / ADAMW_CHUNK);
        }
        a.first_block[a.n] = blocks;
        a.slots = slots + used;
        if (blocks) hipLaunchKernelGGL(finite_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
        used += blocks;
    }
    hipLaunchKernelGGL(finite_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int*)slots, used, sc, (int*)verdict_dev);
    return check_launch("finite_kernel");
}

extern "C" int msmp_adamw_guarded_f32(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                                      float* const* exp_avg_sq, const int64_t* numel, const float* lr_dev, float beta1, float beta2,
                                      float eps, float weight_decay, int64_t* step_dev, const int32_t* verdict_dev, int64_t* skipped_dev,
                                      msmp_stream_t stream) {
    MSMP_REQUIRE(lr_dev && step_dev && verdict_dev && skipped_dev, MSMP_ERR_ARG, "msmp_adamw_guarded_f32: null pointer");
    // everything adamw_launch refuses is refused here first: the counters must not move for a call that updates nothing
    MSMP_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || (params && grads && exp_avg && exp_avg_sq && numel)), MSMP_ERR_ARG, "msmp_adamw_guarded_f32: null pointer");
    MSMP_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, MSMP_ERR_ARG, "msmp_adamw_guarded_f32: bad hyper-parameters");
    for (int i = 0; i < n_tensors; ++i)
        MSMP_REQUIRE(params[i] && grads[i] && exp_avg[i] && exp_avg_sq[i] && numel[i] >= 0 && numel[i] < (1L << 31), MSMP_ERR_ARG,
                     "msmp_adamw_guarded_f32: bad tensor %d (null pointer or element count)", i);
    hipLaunchKernelGGL(adamw_advance_guarded_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long*)step_dev, (const int*)verdict_dev,
                       (long long*)skipped_dev);
    return adamw_launch(n_tensors, params, grads, exp_avg, exp_avg_sq, numel, 0.f, beta1, beta2, eps, weight_decay, 1, step_dev, lr_dev, stream,
                        (const int*)verdict_dev);
}

extern "C" int msmp_status_poison_f32(float* scalar, msmp_stream_t stream) {
    MSMP_REQUIRE(scalar, MSMP_ERR_ARG, "msmp_status_poison_f32: null pointer");
    const int* status = status_ptr();
    if (!status) return MSMP_OK;          // no status word: nothing can have been raised
    hipLaunchKernelGGL(status_poison_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, status, scalar);
    return check_launch("status_poison_kernel");
}
