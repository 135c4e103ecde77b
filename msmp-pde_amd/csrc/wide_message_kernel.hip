// The message half of GNN_LayerLin at ANY hidden width W <= 256 as one launch (msmp_wide_message_f32):
//     agg[n] = mean over the CSR row of n of  Swish(W2 Swish(P[n] + Q[col]) + b2)       (experiments/models_gnn.py:132-138, aggr = 'mean' :107)
// with message_net_1 already factorised per node into P / Q (layers.wide_weights).  The width-generic path evaluated this as three
// launches (wide_gather_swish, msmp_linear_f32, wide_scatter_mean) around two edge-sized [E, ld] tensors; here nothing edge-sized goes to
// memory.  One matrix fits the register file (the structure of lem_encoder_ws3_kernel, not of lem_wide_kernel):
//   * a workgroup has one wave per 32-channel output slice (KT = Wp / 32 waves, Wp = 32 ceil(W / 32)); wave T keeps the fp16 hi / lo A
//     fragments of rows 32 T .. 32 T + 31 of W2 in registers for the whole kernel (2 KT k-steps x 2 planes x 4 = 16 KT registers);
//   * workgroups are persistent and loop over tiles of `tile_nodes` = 64 / max_in_degree consecutive target nodes, whose <= 64 in-edges
//     (consecutive CSR rows) are the 2 x 32 columns of the tile's MFMAs;
//   * per tile wave T gathers channels 32 T .. 32 T + 31 of p[target] and q[source] for all edges (16-byte loads, a full 128-byte line per
//     edge and wave), forms Swish once per element, splits it and publishes the hi / lo B fragments in LDS as
//     [k-step][plane][column block][lane] half8 (wide_frags.h);
//   * every wave reads all B fragments: three MFMAs per K = 16 step (split_mfma3) into one fp32 accumulator initialised with
//     b2 2^s; Swish(acc 2^-s) goes to the wave's OWN message area in LDS ([edge][32 channels], row stride 36 floats) and
//     the wave sums its 32 channels per target in CSR order in fp32 and stores them: no other wave is involved after the MFMAs;
//   * for KT <= 6 the next tile's gathers are issued before the current tile's MFMAs and wait in registers (64 of them); above, the
//     register file has no room beside the 16 KT weight registers and they are issued after the tile's stores.
// A message depends on nothing but its own edge (an MFMA column) and a target's mean is a sequential fp32 sum over its CSR row, so the
// result does not depend on how the targets are cut into tiles, on the tile slot, or on the workgroup.
// Rows / columns W .. Wp - 1 of the packed W2 and of the bias are exact zeros: the padded channels come out as Swish(0) = 0.
#include "wide_frags.h"

namespace msmp {

constexpr int WMSG_NB = 2;                    // 32-edge column blocks per tile
constexpr int WMSG_TE = 32 * WMSG_NB;         // edges per tile = the largest in-degree the kernel takes
constexpr int WMSG_MROW = 36;                 // floats per message row: 4 x odd, so the 16-lane groups of a 16-byte access hit 16 distinct slots

// packed blob (floats): scales [8] (2^s, then 2^-s at [4]) | bias 2^s [Wp] | A fragments [T KT][k-step 2 KT][plane 2: hi, lo][lane 64][8 halfs],
// natural k order (split_k_natural)
struct WideMsgLayout {
    int64_t scales, bias, w, total;
};
__host__ __device__ inline WideMsgLayout wide_msg_layout(int kt) {
    WideMsgLayout L;
    L.scales = 0;
    L.bias = 8;
    L.w = L.bias + 32 * kt;
    L.total = L.w + (int64_t)1024 * kt * kt;
    return L;
}

struct WideMsgPackArgs {
    const float *w2, *b2;
    int width, kt;
    float* out;
};

// scales[0] = 2^s with max(|W2|, |b2|) 2^s in [16, 32), scales[4] = 2^-s
__global__ __launch_bounds__(256) void pack_wide_msg_scale_kernel(WideMsgPackArgs a) {
    const int sft = block_scale_shift(fmaxf(abs_max_part(a.w2, a.width * a.width), abs_max_part(a.b2, a.width)));
    if (threadIdx.x == 0) {
        store_scale_group(a.out, 0, sft, 0);
        a.out[1] = a.out[3] = a.out[5] = a.out[7] = 0.f;        // (no second scale group)
    }
}

__global__ void pack_wide_msg_kernel(WideMsgPackArgs a) {
    const WideMsgLayout L = wide_msg_layout(a.kt);
    const float sc = a.out[L.scales];
    const int kt = a.kt, W = a.width;
    const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = tid0; p < 32 * kt; p += stride) a.out[L.bias + p] = p < W ? a.b2[p] * sc : 0.f;
    pack_split_fragments(reinterpret_cast<_Float16*>(a.out + L.w), (int64_t)2 * kt * kt, [&](int fr, int lane, int j) {
        const int ks = fr % (2 * kt), T = fr / (2 * kt);
        const int row = 32 * T + (lane & 31), k = split_k_natural(ks, lane >> 5, j);
        return row < W && k < W ? a.w2[(size_t)row * W + k] * sc : 0.f;
    });
}

struct WideMsgArgs {
    const float *p, *q;         // [N, ld]
    const int *rowptr, *col;
    int n_nodes, tile_nodes, n_tiles, width, ld;
    const float* scales;
    const float* bias;          // [Wp], times 2^s
    const half8* w;
    float* agg;                 // [N, ld]
    int* status;
};

// the p and q values of one gather item: 8 consecutive channels of one edge's target and source rows
struct WideMsgItem {
    f32x4 p0, p1, q0, q1;
};

struct WideMsgTile {            // wave-uniform description of a tile
    int n0, cnt, e0, ne;        // first target, targets, first edge, edges
};

// Per-tile maps in LDS (ints): edge slot -> target slot [TE] | first edge slot of each target and the end [TE + 1] | first edge of the tile.
// Everything a tile needs from rowptr is read from memory ONCE, a tile ahead: a memory load between the issue of the prefetched gathers
// and their use would be waited for behind them (the vector memory counter retires in order) and drain the prefetch.
constexpr int WMSG_MAP_RP = WMSG_TE, WMSG_MAP_E0 = 2 * WMSG_TE + 1, WMSG_MAP_INTS = 2 * WMSG_TE + 4;

// threads 0 .. cnt - 1 walk their CSR row (<= WMSG_TE edges per tile by the host's choice of tile_nodes; the bounds are enforced again
// here, so a malformed rowptr cannot write outside the maps)
__device__ __forceinline__ void wmsg_fill_maps(const WideMsgArgs& a, long tile, int* map, int tid) {
    const int n0 = (int)(tile * a.tile_nodes), cnt = min(a.tile_nodes, a.n_nodes - n0);
    if (tid < cnt) {
        const int e0 = a.rowptr[n0];
        const int r0 = min(max(a.rowptr[n0 + tid] - e0, 0), WMSG_TE), r1 = min(max(a.rowptr[n0 + tid + 1] - e0, r0), WMSG_TE);
        for (int r = r0; r < r1; ++r) map[r] = tid;
        map[WMSG_MAP_RP + tid] = r0;
        if (tid == cnt - 1) map[WMSG_MAP_RP + cnt] = r1;
        if (tid == 0) map[WMSG_MAP_E0] = e0;
    }
}

// (after the barrier behind wmsg_fill_maps)
__device__ __forceinline__ WideMsgTile wmsg_tile(const WideMsgArgs& a, long tile, const int* map) {
    WideMsgTile t;
    t.n0 = (int)(tile * a.tile_nodes);
    t.cnt = min(a.tile_nodes, a.n_nodes - t.n0);
    t.e0 = __builtin_amdgcn_readfirstlane(map[WMSG_MAP_E0]);
    t.ne = __builtin_amdgcn_readfirstlane(map[WMSG_MAP_RP + t.cnt]);
    return t;
}

// wave T's items of a tile: item i is column block i % NB of k-step 2 T + i / NB; lane (c, hh) takes channels 16 s + 8 hh .. + 7 of edge
// 32 nb + c.  Every address is clamped into the tensors (row 0, the last four columns): loads are unconditional, masking happens at the use.
template <int KT>
__device__ __forceinline__ void wmsg_gather(const WideMsgArgs& a, const WideMsgTile& t, const int* tl, int T, int c, int hh,
                                            WideMsgItem (&g)[2 * WMSG_NB]) {
    const int ld = a.ld;
    // (both source indices first: a col load behind the first block's row loads would be waited for together with them)
    const float *pr[WMSG_NB], *qr[WMSG_NB];
#pragma unroll
    for (int nb = 0; nb < WMSG_NB; ++nb) {
        const int le = 32 * nb + c;
        const bool live = le < t.ne;
        const int src = a.col[live ? t.e0 + le : 0];
        const int tgt = live ? (int)min((unsigned)(t.n0 + tl[le]), (unsigned)(a.n_nodes - 1)) : 0;       // (clamped: a malformed rowptr leaves a slot unset)
        pr[nb] = a.p + (size_t)tgt * ld;
        qr[nb] = a.q + (size_t)src * ld;
    }
#pragma unroll
    for (int nb = 0; nb < WMSG_NB; ++nb)
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            const int k0 = 16 * (2 * T + ss) + 8 * hh;
            WideMsgItem& it = g[ss * WMSG_NB + nb];
            const int ka = min(k0, ld - 4), kb = min(k0 + 4, ld - 4);
            it.p0 = *reinterpret_cast<const f32x4*>(pr[nb] + ka);
            it.p1 = *reinterpret_cast<const f32x4*>(pr[nb] + kb);
            it.q0 = *reinterpret_cast<const f32x4*>(qr[nb] + ka);
            it.q1 = *reinterpret_cast<const f32x4*>(qr[nb] + kb);
        }
}

// Swish(p + q) of the gathered items -> hi / lo B fragments of the tile (publish_split); `worst`: the largest |activation| (track_abs_max)
template <int KT>
__device__ __forceinline__ void wmsg_publish(const WideMsgArgs& a, int ne, int T, int c, int hh, const WideMsgItem (&g)[2 * WMSG_NB],
                                             char* b_lane, unsigned& worst) {
#pragma unroll
    for (int i = 0; i < 2 * WMSG_NB; ++i) {
        const int nb = i % WMSG_NB, s = 2 * T + i / WMSG_NB;
        const int k0 = 16 * s + 8 * hh;
        const bool live = 32 * nb + c < ne;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float x = j < 4 ? g[i].p0[j] + g[i].q0[j] : g[i].p1[j - 4] + g[i].q1[j - 4];
            v[j] = swishf(live && k0 + j < a.width ? x : 0.f);
            track_abs_max(worst, v[j]);
        }
        publish_split<WMSG_NB>(v, b_lane, s, nb);
        // one item at a time, its maximum taken here: left alone the compiler sinks the 32 maxima of a tile to the end of the tile loop and
        // keeps the 32 activations in registers across the MFMAs for it
        asm volatile("" : "+v"(worst));
        __builtin_amdgcn_sched_barrier(0);
    }
}

template <int KT>
__global__ __launch_bounds__(64 * KT, 2) void wide_message_kernel(WideMsgArgs a) {
    constexpr int NB = WMSG_NB, TE = WMSG_TE, KS = 2 * KT;
    constexpr bool PREFETCH = KT <= 6;
    constexpr int BBYTES = KS * 2 * NB * 1024, MBYTES = TE * WMSG_MROW * 4, BIAS = BBYTES + KT * MBYTES, MAPS = BIAS + 32 * KT * 4;
    // one LDS object: B fragments of the tile | one message area per wave | bias 2^s | the maps of three tiles (slot = tile round % 3)
    __shared__ __attribute__((aligned(16))) char lds[MAPS + 3 * WMSG_MAP_INTS * 4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int T = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5;
    const int ld = a.ld;
    const float inv = uniform_ro(a.scales, 4);
    char* const b_lane = lds + lane * 16;
    float* const msg = reinterpret_cast<float*>(lds + BBYTES + T * MBYTES);
    const float* const bias = reinterpret_cast<const float*>(lds + BIAS) + 32 * T + 4 * hh;
    int* const maps = reinterpret_cast<int*>(lds + MAPS);

    // this wave's rows of W2, for the whole kernel
    half8 ah[KS], al[KS];
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        ah[ks] = a.w[((T * KS + ks) * 2 + 0) * 64 + lane];
        al[ks] = a.w[((T * KS + ks) * 2 + 1) * 64 + lane];
    }

    long tile = blockIdx.x;         // (the grid is at most n_tiles)
    if (tid < 32 * KT) reinterpret_cast<float*>(lds + BIAS)[tid] = a.bias[tid];
    wmsg_fill_maps(a, tile, maps, tid);
    __syncthreads();
    WideMsgTile cur = wmsg_tile(a, tile, maps), nxt = cur;
    WideMsgItem g[2 * NB];
    wmsg_gather<KT>(a, cur, maps, T, c, hh, g);
    unsigned worst = 0;

    for (int slot = 0; tile < a.n_tiles; tile += gridDim.x, slot = slot == 2 ? 0 : slot + 1) {
        const bool more = tile + gridDim.x < a.n_tiles;
        const int* const map = maps + slot * WMSG_MAP_INTS;
        int* const map_next = maps + (slot == 2 ? 0 : slot + 1) * WMSG_MAP_INTS;
        wmsg_publish<KT>(a, cur.ne, T, c, hh, g, b_lane, worst);
        // (the slot of tile t + 1 was last read for tile t - 2: in its sums, in front of the first barrier of round t - 1)
        if (more) wmsg_fill_maps(a, tile + gridDim.x, map_next, tid);
        __syncthreads();            // the tile's B fragments and the next tile's maps are complete
        if (more) nxt = wmsg_tile(a, tile + gridDim.x, map_next);
        if (PREFETCH && more) wmsg_gather<KT>(a, nxt, map_next, T, c, hh, g);

        f32x16 acc[NB];
        acc_bias_init(bias, acc);
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            // fence per k-step: left alone the scheduler hoists the unrolled loop's LDS reads far ahead of their MFMAs
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) {
                const half8 bh = frag_lds(b_lane, (2 * ks + 0) * NB + nb), bl = frag_lds(b_lane, (2 * ks + 1) * NB + nb);
                split_mfma3(ah[ks], al[ks], bh, bl, acc[nb]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();            // every wave has read the B fragments: the next tile's may be written

        // messages of this wave's 32 channels -> its own area, [edge][channel]
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                f32x4 m;
#pragma unroll
                for (int i = 0; i < 4; ++i) m[i] = swishf(acc[nb][4 * q + i] * inv);
                *reinterpret_cast<f32x4*>(msg + (32 * nb + c) * WMSG_MROW + 8 * q + 4 * hh) = m;
            }
            __builtin_amdgcn_sched_barrier(0);      // (one column block's activations at a time: 16 temporaries, not 32)
        }
        // (written and read by this wave only: the LDS operations of one wave execute in order)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // mean per target in CSR order: lane = (4-channel group, target slot mod 8)
        {
            const int cg = lane & 7, ch = 32 * T + 4 * cg;
            for (int j = lane >> 3; j < cur.cnt; j += 8) {
                const int r0 = map[WMSG_MAP_RP + j], r1 = map[WMSG_MAP_RP + j + 1];
                f32x4 s = {0.f, 0.f, 0.f, 0.f};
                for (int r = r0; r < r1; ++r) s += *reinterpret_cast<const f32x4*>(msg + r * WMSG_MROW + 4 * cg);
                if (ch < ld) *reinterpret_cast<f32x4*>(a.agg + (size_t)(cur.n0 + j) * ld + ch) = s * (1.0f / (float)max(r1 - r0, 1));
            }
        }
        // columns Wp .. ld - 1 of the tile's rows
        {
            const int extra = (ld - 32 * KT) / 4;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            for (int i = tid; i < cur.cnt * extra; i += 64 * KT)
                *reinterpret_cast<f32x4*>(a.agg + (size_t)(cur.n0 + i / extra) * ld + 32 * KT + 4 * (i % extra)) = zero;
        }
        if (!PREFETCH && more) wmsg_gather<KT>(a, nxt, map_next, T, c, hh, g);
        cur = nxt;
    }
    if (node_range_exceeded(worst)) status_raise(a.status, MSMP_STATUS_NODE_SATURATED);
}

}  // namespace msmp

using namespace msmp;

extern "C" int64_t msmp_packed_wide_msg_floats(int width) {
    if (!wide_width_ok("msmp_packed_wide_msg_floats", width)) return 0;
    return wide_msg_layout((width + 31) / 32).total;
}

extern "C" int msmp_pack_wide_msg_f32(const float* w2, const float* b2, int width, float* packed_out, msmp_stream_t stream) {
    if (!wide_width_ok("msmp_pack_wide_msg_f32", width)) return MSMP_ERR_ARG;
    MSMP_REQUIRE(w2 && b2 && packed_out, MSMP_ERR_ARG, "msmp_pack_wide_msg_f32: null pointer");
    WideMsgPackArgs a{w2, b2, width, (width + 31) / 32, packed_out};
    hipLaunchKernelGGL(pack_wide_msg_scale_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(pack_wide_msg_kernel, dim3(64), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("pack_wide_msg_kernel");
}

extern "C" int msmp_wide_message_max_in_degree(int width) {
    if (!wide_width_ok("msmp_wide_message_max_in_degree", width)) return 0;
    return WMSG_TE;
}

extern "C" int msmp_wide_message_f32(const float* p, const float* q, const int32_t* rowptr, const int32_t* col, int64_t n_nodes, int64_t n_edges,
                                     int max_in_degree, int width, int ld, const float* packed, float* agg_out, msmp_stream_t stream) {
    if (!wide_width_ok("msmp_wide_message_f32", width)) return MSMP_ERR_ARG;
    MSMP_REQUIRE(ld >= width && ld % 4 == 0 && ld <= 4096, MSMP_ERR_ARG, "msmp_wide_message_f32: ld=%d is not a multiple of 4 in width..4096", ld);
    MSMP_REQUIRE(p && q && rowptr && col && packed && agg_out, MSMP_ERR_ARG, "msmp_wide_message_f32: null pointer");
    MSMP_REQUIRE(n_nodes >= 0 && n_nodes < (1L << 31) && n_edges >= 0 && n_edges < (1L << 31) && max_in_degree >= 0, MSMP_ERR_ARG,
                 "msmp_wide_message_f32: bad sizes");
    MSMP_REQUIRE(((uintptr_t)p | (uintptr_t)q | (uintptr_t)agg_out | (uintptr_t)packed) % 16 == 0, MSMP_ERR_ARG,
                 "msmp_wide_message_f32: p, q, packed and agg_out must be 16-byte aligned");
    if (max_in_degree > WMSG_TE) {
        set_error("msmp_wide_message_f32: max_in_degree=%d above %d (take the gather / GEMM / scatter path)", max_in_degree, WMSG_TE);
        return MSMP_ERR_UNSUPPORTED;
    }
    if (n_nodes == 0) return MSMP_OK;
    hipStream_t st = (hipStream_t)stream;
    if (n_edges == 0) {
        if (hipMemsetAsync(agg_out, 0, (size_t)n_nodes * ld * sizeof(float), st) != hipSuccess) return check_launch("msmp_wide_message_f32 (memset)");
        return MSMP_OK;
    }
    const int kt = (width + 31) / 32;
    const WideMsgLayout L = wide_msg_layout(kt);
    const int tile_nodes = WMSG_TE / (max_in_degree > 1 ? max_in_degree : 1);
    const long n_tiles = (n_nodes + tile_nodes - 1) / tile_nodes;
    WideMsgArgs a{p, q, rowptr, col, (int)n_nodes, tile_nodes, (int)n_tiles, width, ld, packed + L.scales, packed + L.bias,
                  reinterpret_cast<const half8*>(packed + L.w), agg_out, status_ptr()};
    dispatch_kt(kt, [&](auto K) {
        constexpr int KT = decltype(K)::value;
        // persistent (LDS: 8 KT KB of fragments + 9 KT KB of messages + bias + maps)
        constexpr int lds_bytes = 2 * KT * 2 * WMSG_NB * 1024 + KT * WMSG_TE * WMSG_MROW * 4 + 32 * KT * 4 + 3 * WMSG_MAP_INTS * 4;
        const long resident = resident_workgroups(device_cus(), lds_bytes, KT);
        const unsigned grid = (unsigned)(a.n_tiles < resident ? a.n_tiles : resident);
        hipLaunchKernelGGL((wide_message_kernel<KT>), dim3(grid), dim3(64 * KT), 0, st, a);
    });
    return check_launch("wide_message_kernel");
}
