// The gradient gate (G2) of MP_PDE_Solver2DLEMLinG2 (experiments/models_gnn2D.py:598-611) between the two layer calls of a pair: gate
// statistic, tanh and blend as ONE launch forward, and its backward as one node pass and one gather pass.  With t = Swish(a) (a: the gate
// layer's output after its InstanceNorm), b the main layer's output, out(i) the out-edges of node i in the order of
// GraphStructure.by_source() and D_i = max(|out(i)|, 1):
//
//   forward    m_i   = (1 / D_i) sum_{j in out(i)} (t_i - t_j)^2     (summed edge by edge in that order, square and add rounded separately,
//                                                                      then times 1 / D_i, as scatter_mean_kernel forms a mean)
//              tau_i = tanh(m_i)
//              out_i = (1 - tau_i) h_i + tau_i Swish(b_i)
//   backward   dh_i  = (1 - tau_i) g_i                                g = dL/dout
//              db_i  = tau_i g_i Swish'(b_i)
//              q_i   = g_i (Swish(b_i) - h_i) (1 - tau_i^2) / D_i     (node pass; q is the node-sized workspace)
//              dt_i  = 2 q_i sum_{j in out(i)} (t_i - t_j) - 2 sum_{s in in(i)} q_s (t_s - t_i)        (gather pass: out-list, then in-list)
//              da_i  = dt_i Swish'(a_i)
//
// Nothing edge-sized is read or written but the two int32 neighbour lists: Swish(a_j) is recomputed per edge (a row of a is 512 B at width
// 128 and stays in L2 between the ~D neighbours that read it).  Thread layout: one thread per (node, 4 channels), consecutive threads on
// consecutive channel groups of a node -- at width 128 the 32 lanes x 16 B of scatter_mean_kernel, eight nodes per 256-thread block; at other
// widths a wave simply covers 64 * 4 / width nodes.  Every thread runs its node's edge list on its own, four rows in flight, so there is
// no cross-lane step, no LDS, no atomic and no memset, and the summation order is the list's: two runs give the same bits.  Plain fp32:
// no input range, the range status is neither read nor raised.  tau is saved by the forward for the backward (one [N, ld] tensor).
#include "msmp_common.h"

namespace msmp {

__device__ __forceinline__ f32x4 swish4(f32x4 x) {
    f32x4 r;
#pragma unroll
    for (int m = 0; m < 4; ++m) r[m] = swishf(x[m]);
    return r;
}

// s + (ti - Swish(aj))^2 with the square rounded before it is added (the per-edge tensor of the PyTorch route is a rounded square)
__device__ __forceinline__ f32x4 add_sq_diff(f32x4 s, f32x4 ti, f32x4 aj) {
#pragma clang fp contract(off)
    const f32x4 d = ti - swish4(aj);
    const f32x4 sq = d * d;
    return s + sq;
}

struct G2Args {
    const float *h, *gate, *mainp;
    const int *out_rowptr, *out_nbr;
    float *out, *tau_out;
    long n_nodes;
    int ld4, w4;
};

template <bool SAVE_TAU>
__global__ __launch_bounds__(256) void g2_gate_blend_kernel(G2Args a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long node = idx / a.w4;
    if (node >= a.n_nodes) return;
    const int c = (int)(idx - node * a.w4);
    const f32x4* gp = reinterpret_cast<const f32x4*>(a.gate) + c;
    const size_t o = (size_t)node * a.ld4 + c;
    const f32x4 ti = swish4(gp[(size_t)node * a.ld4]);
    const int r0 = a.out_rowptr[node], r1 = a.out_rowptr[node + 1];
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    int r = r0;
    for (; r + 4 <= r1; r += 4) {
        const int j0 = a.out_nbr[r], j1 = a.out_nbr[r + 1], j2 = a.out_nbr[r + 2], j3 = a.out_nbr[r + 3];
        const f32x4 a0 = gp[(size_t)j0 * a.ld4], a1 = gp[(size_t)j1 * a.ld4], a2 = gp[(size_t)j2 * a.ld4], a3 = gp[(size_t)j3 * a.ld4];
        s = add_sq_diff(s, ti, a0);
        s = add_sq_diff(s, ti, a1);
        s = add_sq_diff(s, ti, a2);
        s = add_sq_diff(s, ti, a3);
    }
    for (; r < r1; ++r) s = add_sq_diff(s, ti, gp[(size_t)a.out_nbr[r] * a.ld4]);
    const float inv = 1.0f / (float)max(r1 - r0, 1);
    const f32x4 hv = reinterpret_cast<const f32x4*>(a.h)[o], bv = reinterpret_cast<const f32x4*>(a.mainp)[o];
    f32x4 tau, res;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        tau[m] = tanhf(s[m] * inv);
        res[m] = (1.0f - tau[m]) * hv[m] + tau[m] * swishf(bv[m]);
    }
    reinterpret_cast<f32x4*>(a.out)[o] = res;
    if (SAVE_TAU) reinterpret_cast<f32x4*>(a.tau_out)[o] = tau;
}

struct G2BwdArgs {
    const float *gout, *h, *gate, *mainp, *tau;
    const int *out_rowptr, *out_nbr, *in_rowptr, *in_col;
    float *dh, *da, *db, *q;        // q [n_nodes, 4 w4] dense
    long n_nodes;
    int ld4, w4;
};

// dh, db and q: a node's own rows only
__global__ __launch_bounds__(256) void g2_gate_bwd_node_kernel(G2BwdArgs a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long node = idx / a.w4;
    if (node >= a.n_nodes) return;
    const int c = (int)(idx - node * a.w4);
    const size_t o = (size_t)node * a.ld4 + c;
    const f32x4 g = reinterpret_cast<const f32x4*>(a.gout)[o], hv = reinterpret_cast<const f32x4*>(a.h)[o];
    const f32x4 bv = reinterpret_cast<const f32x4*>(a.mainp)[o], tau = reinterpret_cast<const f32x4*>(a.tau)[o];
    const float inv = 1.0f / (float)max(a.out_rowptr[node + 1] - a.out_rowptr[node], 1);
    f32x4 dh, db, q;
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        dh[m] = (1.0f - tau[m]) * g[m];
        db[m] = tau[m] * g[m] * dswish(bv[m]);
        q[m] = g[m] * (swishf(bv[m]) - hv[m]) * (1.0f - tau[m] * tau[m]) * inv;
    }
    reinterpret_cast<f32x4*>(a.dh)[o] = dh;
    reinterpret_cast<f32x4*>(a.db)[o] = db;
    reinterpret_cast<f32x4*>(a.q)[idx] = q;
}

// da: node i's out-list (its own q) and in-list (the sources' q), each in list order
__global__ __launch_bounds__(256) void g2_gate_bwd_gather_kernel(G2BwdArgs a) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const long node = idx / a.w4;
    if (node >= a.n_nodes) return;
    const int c = (int)(idx - node * a.w4);
    const f32x4* gp = reinterpret_cast<const f32x4*>(a.gate) + c;
    const f32x4* qp = reinterpret_cast<const f32x4*>(a.q) + c;
    const f32x4 ai = gp[(size_t)node * a.ld4];
    const f32x4 ti = swish4(ai);
    f32x4 so = {0.f, 0.f, 0.f, 0.f}, si = {0.f, 0.f, 0.f, 0.f};
    int r = a.out_rowptr[node];
    const int r1 = a.out_rowptr[node + 1];
    for (; r + 4 <= r1; r += 4) {
        const int j0 = a.out_nbr[r], j1 = a.out_nbr[r + 1], j2 = a.out_nbr[r + 2], j3 = a.out_nbr[r + 3];
        const f32x4 a0 = gp[(size_t)j0 * a.ld4], a1 = gp[(size_t)j1 * a.ld4], a2 = gp[(size_t)j2 * a.ld4], a3 = gp[(size_t)j3 * a.ld4];
        so += ti - swish4(a0);
        so += ti - swish4(a1);
        so += ti - swish4(a2);
        so += ti - swish4(a3);
    }
    for (; r < r1; ++r) so += ti - swish4(gp[(size_t)a.out_nbr[r] * a.ld4]);
    int e = a.in_rowptr[node];
    const int e1 = a.in_rowptr[node + 1];
    for (; e + 2 <= e1; e += 2) {
        const int s0 = a.in_col[e], s1 = a.in_col[e + 1];
        const f32x4 a0 = gp[(size_t)s0 * a.ld4], a1 = gp[(size_t)s1 * a.ld4];
        const f32x4 q0 = qp[(size_t)s0 * a.w4], q1 = qp[(size_t)s1 * a.w4];
        si += q0 * (swish4(a0) - ti);
        si += q1 * (swish4(a1) - ti);
    }
    for (; e < e1; ++e) {
        const int s0 = a.in_col[e];
        si += qp[(size_t)s0 * a.w4] * (swish4(gp[(size_t)s0 * a.ld4]) - ti);
    }
    const f32x4 qi = qp[(size_t)node * a.w4];
    f32x4 da;
#pragma unroll
    for (int m = 0; m < 4; ++m) da[m] = (2.0f * qi[m] * so[m] - 2.0f * si[m]) * dswish(ai[m]);
    reinterpret_cast<f32x4*>(a.da)[(size_t)node * a.ld4 + c] = da;
}

static bool g2_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static bool g2_width_ok(const char* who, int width) {
    if (width < 4 || width > 256 || width % 4) {
        set_error("%s: width=%d is not a multiple of 4 in 4..256", who, width);
        return false;
    }
    return true;
}

}  // namespace msmp

using namespace msmp;

#define G2_ROWS(who, p) MSMP_REQUIRE((p) && g2_aligned16(p), MSMP_ERR_ARG, who ": %s is %s", #p, (p) ? "not 16-byte aligned" : "a null pointer")
#define G2_LIST(who, p) MSMP_REQUIRE(p, MSMP_ERR_ARG, who ": %s is a null pointer", #p)
#define G2_SIZES(who)                                                                                                                     \
    MSMP_REQUIRE(ld >= width && ld % 4 == 0, MSMP_ERR_ARG, who ": ld=%d is not a multiple of 4 that is at least width=%d", ld, width);   \
    MSMP_REQUIRE(n_nodes > 0 && n_nodes < (1L << 31), MSMP_ERR_ARG, who ": n_nodes=%lld outside 1 .. 2^31 - 1", (long long)n_nodes);     \
    MSMP_REQUIRE(n_edges >= 0 && n_edges < (1L << 31), MSMP_ERR_ARG, who ": n_edges=%lld outside 0 .. 2^31 - 1", (long long)n_edges)

extern "C" int msmp_g2_gate_blend_f32(const float* h, const float* gate, const float* main, int ld, const int32_t* out_rowptr,
                                      const int32_t* out_nbr, int64_t n_nodes, int64_t n_edges, int width, float* out, float* tau_out,
                                      msmp_stream_t stream) {
    if (!g2_width_ok("msmp_g2_gate_blend_f32", width)) return MSMP_ERR_UNSUPPORTED;
    G2_ROWS("msmp_g2_gate_blend_f32", h);
    G2_ROWS("msmp_g2_gate_blend_f32", gate);
    G2_ROWS("msmp_g2_gate_blend_f32", main);
    G2_LIST("msmp_g2_gate_blend_f32", out_rowptr);
    G2_LIST("msmp_g2_gate_blend_f32", out_nbr);
    G2_ROWS("msmp_g2_gate_blend_f32", out);
    MSMP_REQUIRE(g2_aligned16(tau_out), MSMP_ERR_ARG, "msmp_g2_gate_blend_f32: tau_out is not 16-byte aligned");
    G2_SIZES("msmp_g2_gate_blend_f32");
    const G2Args a{h, gate, main, out_rowptr, out_nbr, out, tau_out, (long)n_nodes, ld / 4, width / 4};
    const unsigned grid = (unsigned)((n_nodes * a.w4 + 255) / 256);
    timing_begin(MSMP_K_NORM, (hipStream_t)stream);
    if (tau_out)
        hipLaunchKernelGGL(g2_gate_blend_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(g2_gate_blend_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    timing_end(MSMP_K_NORM, (hipStream_t)stream);
    return check_launch("g2_gate_blend_kernel");
}

extern "C" size_t msmp_g2_gate_blend_bwd_workspace_bytes(int64_t n_nodes, int width) {
    if (!g2_width_ok("msmp_g2_gate_blend_bwd_workspace_bytes", width)) return 0;
    if (n_nodes <= 0 || n_nodes >= (1L << 31)) {
        set_error("msmp_g2_gate_blend_bwd_workspace_bytes: n_nodes=%lld outside 1 .. 2^31 - 1", (long long)n_nodes);
        return 0;
    }
    return (size_t)n_nodes * (size_t)width * sizeof(float);
}

extern "C" int msmp_g2_gate_blend_bwd_f32(const float* grad_out, const float* h, const float* gate, const float* main, const float* tau,
                                          int ld, const int32_t* out_rowptr, const int32_t* out_nbr, const int32_t* in_rowptr,
                                          const int32_t* in_col, int64_t n_nodes, int64_t n_edges, int width, float* dh, float* da,
                                          float* db, void* workspace, size_t workspace_bytes, msmp_stream_t stream) {
    if (!g2_width_ok("msmp_g2_gate_blend_bwd_f32", width)) return MSMP_ERR_UNSUPPORTED;
    G2_ROWS("msmp_g2_gate_blend_bwd_f32", grad_out);
    G2_ROWS("msmp_g2_gate_blend_bwd_f32", h);
    G2_ROWS("msmp_g2_gate_blend_bwd_f32", gate);
    G2_ROWS("msmp_g2_gate_blend_bwd_f32", main);
    G2_ROWS("msmp_g2_gate_blend_bwd_f32", tau);
    G2_LIST("msmp_g2_gate_blend_bwd_f32", out_rowptr);
    G2_LIST("msmp_g2_gate_blend_bwd_f32", out_nbr);
    G2_LIST("msmp_g2_gate_blend_bwd_f32", in_rowptr);
    G2_LIST("msmp_g2_gate_blend_bwd_f32", in_col);
    G2_ROWS("msmp_g2_gate_blend_bwd_f32", dh);
    G2_ROWS("msmp_g2_gate_blend_bwd_f32", da);
    G2_ROWS("msmp_g2_gate_blend_bwd_f32", db);
    G2_ROWS("msmp_g2_gate_blend_bwd_f32", workspace);
    G2_SIZES("msmp_g2_gate_blend_bwd_f32");
    MSMP_REQUIRE(workspace_bytes >= (size_t)n_nodes * (size_t)width * sizeof(float), MSMP_ERR_WORKSPACE,
                 "msmp_g2_gate_blend_bwd_f32: workspace_bytes=%zu below %zu", workspace_bytes, (size_t)n_nodes * (size_t)width * sizeof(float));
    const G2BwdArgs a{grad_out, h, gate, main, tau, out_rowptr, out_nbr, in_rowptr, in_col, dh, da, db, static_cast<float*>(workspace),
                      (long)n_nodes, ld / 4, width / 4};
    const unsigned grid = (unsigned)((n_nodes * a.w4 + 255) / 256);
    timing_begin(MSMP_K_NORM, (hipStream_t)stream);
    hipLaunchKernelGGL(g2_gate_bwd_node_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(g2_gate_bwd_gather_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, a);
    timing_end(MSMP_K_NORM, (hipStream_t)stream);
    return check_launch("g2_gate_bwd_kernel");
}
