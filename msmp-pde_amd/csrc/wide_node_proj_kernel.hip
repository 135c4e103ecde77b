// The per-node projections of the factorised message_net_1 of GNN_LayerLin at ANY hidden width W <= 256 as one launch per layer
// (msmp_wide_node_proj_f32), both heads of a gated pair (experiments/models_gnn.py:132-138):
//     P[n] = W1[:, 0:W]  h_n + W1[:, 2W:] [u_n | pos_n | vars_n] + b1          the edge's target side
//     Q[n] = W1[:, W:2W] h_n - W1[:, 2W:2W+tw+1] [u_n | pos_n]                 the edge's source side
// (message_net_1 of edge j -> i is then Swish(P[i] + Q[j]): wide_message_kernel.hip).  The width-generic path evaluated this per layer as a
// concatenation [h | u | pos | vars] and four row GEMMs over it; here nothing node-sized but h, the packed feature rows and the outputs
// touches memory, and the rows are staged and split ONCE for the (up to) four output matrices.  Wave-to-channel assignment of the sibling
// kernels:
//   * a workgroup has one wave per 32-channel output slice (KT = Wp / 32 waves, Wp = 32 ceil(W / 32)) and is persistent over tiles of 64
//     consecutive nodes = two 32-node MFMA column blocks;
//   * per tile the waves split the h rows (wave T: k-steps 2 T, 2 T + 1) and the packed [u | pos | vars | 0] rows (tail k-step t goes to wave
//     t mod KT) into fp16 hi / lo B fragments in LDS: K = Wp + 16 tail_steps, tail_steps = ceil((tw + 1 + nv) / 16) <= 8 (a template parameter beside KT);
//   * the weights stream: an A fragment (row slice T, k-step) has exactly one consumer wave, so it goes from L2 into that wave's registers
//     through a three-slot ring and serves both column blocks.  P and Q of a head run TOGETHER over the k-steps (64 accumulator registers,
//     a ring slot holds the hi / lo fragments of both): a B fragment read from LDS then feeds six MFMAs instead of three, which halves the
//     LDS traffic of the GEMM; this kernel has no other use for the registers.  The ring never drains: the first two
//     k-steps of the next head (or of the next tile's first head) are requested before the epilogue's stores.
// Arithmetic of wide_frags.h, with the node rows scaled by 2^8 and split (split8_node), P's accumulators initialised with the scaled bias and
// Q's with zero.  Rows / columns W .. Wp - 1 and the tail columns up to the k-step of the packed weights are exact zeros.  A node is one
// MFMA column: its result depends on nothing but its own rows and the weights, not on the tile it falls into, the batch, or the run.
#include "wide_frags.h"

namespace msmp {

constexpr int WNP_NB = 2;                     // column blocks of a tile (64 nodes)
constexpr int WNP_TILE = 32 * WNP_NB;
constexpr int WNP_MAX_TAIL = 128;             // columns of [u | pos | vars]

__host__ __device__ inline int wide_proj_tail_steps(int tw, int nv) { return (tw + 1 + nv + 15) / 16; }

// packed blob (floats): scales [8]: 2^s, 0, 0, 0, 2^-(s + 8), 0, 0, 0 | b1 2^(s + 8) [Wp] |
//   w: [T KT][matrix 2: P, Q][k-step 2 KT + tail_steps][plane 2: hi, lo][lane 64][8 halfs], natural k order: k-steps 0 .. 2 KT - 1 the h
//      columns (P: W1[:, 0:W], Q: W1[:, W:2W]), then the tail (P: W1[:, 2W:], Q: -W1[:, 2W:2W+tw+1] and zeros for the variables)
struct WideProjLayout {
    int64_t scales, b1, w, total;
};
__host__ __device__ inline WideProjLayout wide_proj_layout(int kt, int ts) {
    WideProjLayout L;
    L.scales = 0;
    L.b1 = 8;
    L.w = L.b1 + 32 * kt;
    L.total = L.w + (int64_t)512 * kt * 2 * (2 * kt + ts);
    return L;
}

struct WideProjPackArgs {
    const float *w1, *b1;
    int width, tw, nv, kt, ts;
    float* out;
};

// scales[0] = 2^s with max(|W1|, |b1|) 2^s in [16, 32), scales[4] = 2^-(s + 8) (the node rows carry 2^8).  grid = 1.
__global__ __launch_bounds__(256) void pack_wide_proj_scale_kernel(WideProjPackArgs a) {
    const int sft = block_scale_shift(fmaxf(abs_max_part(a.w1, a.width * (2 * a.width + a.tw + 1 + a.nv)), abs_max_part(a.b1, a.width)));
    if (threadIdx.x == 0) {
        store_scale_group(a.out, 0, sft, 8);
        a.out[1] = a.out[3] = a.out[5] = a.out[7] = 0.f;
    }
}

__global__ void pack_wide_proj_kernel(WideProjPackArgs a) {
    const WideProjLayout L = wide_proj_layout(a.kt, a.ts);
    const float s = a.out[L.scales];
    const int kt = a.kt, W = a.width, nks = 2 * kt + a.ts, tail_p = a.tw + 1 + a.nv, tail_q = a.tw + 1, kin = 2 * W + tail_p;
    const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = tid0; p < 32 * kt; p += stride) a.out[L.b1 + p] = p < W ? a.b1[p] * s * 256.0f : 0.f;
    pack_split_fragments(reinterpret_cast<_Float16*>(a.out + L.w), (int64_t)2 * kt * nks, [&](int fr, int lane, int j) {
        const int ks = fr % nks, q = (fr / nks) & 1, T = fr / (2 * nks);
        const int row = 32 * T + (lane & 31), hh = lane >> 5;
        int col = -1;
        if (ks < 2 * kt) {
            const int k = split_k_natural(ks, hh, j);
            if (k < W) col = q * W + k;
        } else {
            const int k = split_k_natural(ks - 2 * kt, hh, j);
            if (k < (q ? tail_q : tail_p)) col = 2 * W + k;
        }
        if (row >= W || col < 0) return 0.f;
        const float w = a.w1[(size_t)row * kin + col] * s;
        return q && ks >= 2 * kt ? -w : w;
    });
}

struct WideProjHead {
    const float* scales;        // null: no such head
    const float* b1;            // [Wp], scaled
    const half8* w;
    float *p, *q;               // [N, ld]
};

struct WideProjArgs {
    const float *h, *feat;      // [N, ld], [N, fs]
    int n_nodes, width, ld, fs, tail;           // tail = tw + 1 + nv columns of feat
    WideProjHead main, gate;
    int* status;
};

// the A fragments of one k-step: hi / lo of this wave's row slice of P and of Q
struct WideProjSlot {
    half8 ph, pl, qh, ql;
};
// wp / wq: this wave's fragment streams ([k-step][plane][lane] half8)
__device__ __forceinline__ void wnp_slot_load(WideProjSlot& s, const half8* wp, const half8* wq, int ks, unsigned lo) {
    s.ph = frag_global(wp, 2 * ks + 0, lo);
    s.pl = frag_global(wp, 2 * ks + 1, lo);
    s.qh = frag_global(wq, 2 * ks + 0, lo);
    s.ql = frag_global(wq, 2 * ks + 1, lo);
}
// wave T's P stream of a head (its Q stream follows nks k-steps later), in a register the compiler cannot see through: as invariants of
// the tile loop the base + constant addresses of an unrolled GEMM take more scalar registers than there are
__device__ __forceinline__ const half8* wnp_stream(const WideProjHead& hd, int T, int nks) {
    const half8* wp = hd.w + (size_t)(2 * T) * nks * 128;
    asm volatile("" : "+s"(wp));
    return wp;
}

// the fragments in flight, two k-steps ahead of their MFMAs: slot ks % 3 holds k-step ks
struct WideProjRing {
    WideProjSlot s[3];
};
__device__ __forceinline__ void wnp_ring_start(WideProjRing& r, const WideProjHead& hd, int T, int nks, unsigned lo) {
    const half8* const wp = wnp_stream(hd, T, nks);
    wnp_slot_load(r.s[0], wp, wp + (size_t)nks * 128, 0, lo);
    wnp_slot_load(r.s[1], wp, wp + (size_t)nks * 128, 1, lo);       // (nks >= 3: two k-steps of h and one of the tail at the least)
}

// P += A_p B, Q += A_q B over NKS k-steps for both column blocks: wp / wq this wave's fragment streams (already started in the ring),
// b_lane the per-lane LDS address of fragment (k-step 0, hi, block 0)
template <int NKS>
__device__ __forceinline__ void wnp_gemm(WideProjRing& r, const half8* wp, const half8* wq, unsigned lo, const char* b_lane, f32x16 (&p)[WNP_NB],
                                         f32x16 (&q)[WNP_NB]) {
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        // fence per k-step: left alone the scheduler hoists the unrolled loop's LDS reads far ahead of their MFMAs
        __builtin_amdgcn_sched_barrier(0);
        if (ks + 2 < NKS) wnp_slot_load(r.s[(ks + 2) % 3], wp, wq, ks + 2, lo);
        const WideProjSlot& cur = r.s[ks % 3];
#pragma unroll
        for (int blk = 0; blk < WNP_NB; ++blk) {
            const half8 bh = frag_lds(b_lane, (ks * 2 + 0) * WNP_NB + blk), bl = frag_lds(b_lane, (ks * 2 + 1) * WNP_NB + blk);
            split_mfma3(cur.ph, cur.pl, bh, bl, p[blk]);
            split_mfma3(cur.qh, cur.ql, bh, bl, q[blk]);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}

// one K = 16 step (source k-step s) of the tile's rows of `src` ([n_nodes, ld]), both column blocks: lane (c, hh) takes k = 16 s + 8 hh .. + 7
// of node n0 + 32 block + c.  Every address is clamped into the tensor.
__device__ __forceinline__ void wnp_load_step(const float* src, int ld, int n0, int n_nodes, int s, int c, int hh, f32x4 (&v)[2 * WNP_NB]) {
#pragma unroll
    for (int blk = 0; blk < WNP_NB; ++blk) {
        const int node = min(n0 + 32 * blk + c, n_nodes - 1);
        const float* row = src + (size_t)node * ld;
        const int k0 = 16 * s + 8 * hh;
        v[2 * blk + 0] = *reinterpret_cast<const f32x4*>(row + min(k0, ld - 4));
        v[2 * blk + 1] = *reinterpret_cast<const f32x4*>(row + min(k0 + 4, ld - 4));
    }
}
// ... -> hi / lo B fragments of k-step s_dst, scaled by 2^8; dead nodes (local index >= cnt) and columns >= kmax become zeros
__device__ __forceinline__ void wnp_publish_step(const f32x4 (&v)[2 * WNP_NB], int kmax, int cnt, int s, int s_dst, int c, int hh, char* lane_base,
                                                 unsigned& worst) {
#pragma unroll
    for (int blk = 0; blk < WNP_NB; ++blk) {
        const int k0 = 16 * s + 8 * hh;
        const bool live = 32 * blk + c < cnt;
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            x[j] = live && k0 + j < kmax ? (j < 4 ? v[2 * blk][j] : v[2 * blk + 1][j - 4]) : 0.f;
            track_abs_max(worst, x[j]);
        }
        publish_split<WNP_NB, true>(x, lane_base, s_dst, blk);
    }
}

// the epilogue of one output matrix: acc 2^-(s + 8) -> rows n0 .. n0 + cnt - 1 of out, 16 bytes per store, columns W .. Wp - 1 as zeros
__device__ __forceinline__ void wnp_store(const f32x16 (&acc)[WNP_NB], float inv, float* out, int n0, int cnt, int W, int ld, int T, int c, int hh) {
#pragma unroll
    for (int blk = 0; blk < WNP_NB; ++blk) {
        if (32 * blk + c < cnt) {
            float* const row = out + (size_t)(n0 + 32 * blk + c) * ld;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int ch = 32 * T + 8 * q + 4 * hh;
                if (ch < ld) {
                    f32x4 res;
#pragma unroll
                    for (int m = 0; m < 4; ++m) res[m] = ch + m < W ? acc[blk][4 * q + m] * inv : 0.f;
                    *reinterpret_cast<f32x4*>(row + ch) = res;
                }
            }
        }
    }
}

// P and Q of one head for the staged tile.  The ring holds the head's first two k-steps on entry and those of `next` (the head that follows:
// the other one of a pair, or this tile's first head again for the next tile) on return.
template <int KT, int TS>
__device__ __forceinline__ void wnp_head(const WideProjArgs& a, const WideProjHead& hd, const WideProjHead& next, WideProjRing& r, int n0, int cnt,
                                         int T, int tid, unsigned lo, const char* lds) {
    // (the lane offset is made opaque again in every pass: no fragment address formed from it lives longer than the pass)
    asm volatile("" : "+v"(lo));
    const int lane = lo >> 4, c = lane & 31, hh = lane >> 5;
    constexpr int nks = 2 * KT + TS;
    const half8* const wp = wnp_stream(hd, T, nks);
    const half8* const wq = wp + (size_t)nks * 128;
    f32x16 p[WNP_NB], q[WNP_NB];
    acc_bias_init(hd.b1 + 32 * T + 4 * hh, p);
#pragma unroll
    for (int blk = 0; blk < WNP_NB; ++blk)
#pragma unroll
        for (int i = 0; i < 16; ++i) q[blk][i] = 0.f;
    wnp_gemm<nks>(r, wp, wq, lo, lds + lo, p, q);
    wnp_ring_start(r, next, T, nks, lo);
    const float inv = uniform_ro(hd.scales, 4);
    wnp_store(p, inv, hd.p, n0, cnt, a.width, a.ld, T, c, hh);
    wnp_store(q, inv, hd.q, n0, cnt, a.width, a.ld, T, c, hh);
    // columns Wp .. ld - 1 of the tile's rows
    const int extra = (a.ld - 32 * KT) / 4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < cnt * extra; i += 64 * KT) {
        const size_t at = (size_t)(n0 + i / extra) * a.ld + 32 * KT + 4 * (i % extra);
        *reinterpret_cast<f32x4*>(hd.p + at) = zero;
        *reinterpret_cast<f32x4*>(hd.q + at) = zero;
    }
}

constexpr int wnp_lds_bytes(int kt, int ts) { return (2 * kt + ts) * 2 * WNP_NB * 1024; }

// TS: the tail's k-steps (a template parameter: the GEMM is unrolled over all 2 KT + TS k-steps, and every fragment address is the wave's
// base + the lane offset + a constant)
template <int KT, int TS>
__global__ __launch_bounds__(64 * KT, 2) void wide_node_proj_kernel(WideProjArgs a) {
    constexpr int KS = 2 * KT, nks = KS + TS;
    // B fragments of the tile: [k-step 2 KT + TS][plane][block][lane] half8
    __shared__ __attribute__((aligned(16))) char lds[wnp_lds_bytes(KT, TS)];
    const int tid = threadIdx.x;
    const int T = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n_tiles = (a.n_nodes + WNP_TILE - 1) / WNP_TILE;
    const bool gated = a.gate.scales != nullptr;
    unsigned worst = 0;
    WideProjRing ring;
    if ((int)blockIdx.x < n_tiles) wnp_ring_start(ring, a.main, T, nks, (tid & 63) * 16);

    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        // everything that depends on the lane is formed again per tile from an opaque copy: as loop invariants the per-lane addresses of the
        // staging loads, the fragments and the stores stay in registers across the whole loop body
        int lane = tid & 63;
        asm volatile("" : "+v"(lane));
        const int c = lane & 31, hh = lane >> 5;
        const unsigned lo = lane * 16;
        const int n0 = tile * WNP_TILE;
        const int cnt = min(a.n_nodes - n0, WNP_TILE);
        {
            f32x4 vh[2][2 * WNP_NB], vf[2 * WNP_NB];
            wnp_load_step(a.h, a.ld, n0, a.n_nodes, 2 * T, c, hh, vh[0]);
            wnp_load_step(a.h, a.ld, n0, a.n_nodes, 2 * T + 1, c, hh, vh[1]);
            if (T < TS) wnp_load_step(a.feat, a.fs, n0, a.n_nodes, T, c, hh, vf);
            wnp_publish_step(vh[0], a.width, cnt, 2 * T, 2 * T, c, hh, lds + lo, worst);
            wnp_publish_step(vh[1], a.width, cnt, 2 * T + 1, 2 * T + 1, c, hh, lds + lo, worst);
            if (T < TS) wnp_publish_step(vf, a.tail, cnt, T, KS + T, c, hh, lds + lo, worst);
#pragma unroll 1
            for (int t = T + KT; t < TS; t += KT) {           // (more tail k-steps than waves: narrow layers with long windows)
                wnp_load_step(a.feat, a.fs, n0, a.n_nodes, t, c, hh, vf);
                wnp_publish_step(vf, a.tail, cnt, t, KS + t, c, hh, lds + lo, worst);
            }
        }
        __syncthreads();                // the tile's fragments are complete
        if (gated) {
            wnp_head<KT, TS>(a, a.main, a.gate, ring, n0, cnt, T, tid, lo, lds);
            wnp_head<KT, TS>(a, a.gate, a.main, ring, n0, cnt, T, tid, lo, lds);
        } else {
            wnp_head<KT, TS>(a, a.main, a.main, ring, n0, cnt, T, tid, lo, lds);
        }
        __syncthreads();                // every wave has read the fragments: the next tile may be staged over them
    }
    if (node_range_exceeded(worst)) status_raise(a.status, MSMP_STATUS_NODE_SATURATED);
}

}  // namespace msmp

using namespace msmp;

// msmp_tune("wide_proj", 1): the host layer takes this kernel at widths other than 128; 0 (default): the concatenation and two msmp_linear_f32
// per head.  It ships at 0 until the per-step A/B and the full-depth error of DESIGN.md 4.21 are measured on the MI355X.

static bool wide_proj_shape_ok(const char* who, int tw, int nv) {
    if (tw < 1 || nv < 1 || nv > MSMP_MAX_VARS) {
        set_error("%s: tw=%d, nv=%d outside tw >= 1, nv in 1..%d", who, tw, nv, MSMP_MAX_VARS);
        return false;
    }
    return true;
}
static bool wide_proj_tail_ok(const char* who, int tw, int nv) {
    if ((int64_t)tw + 1 + nv > WNP_MAX_TAIL) {
        set_error("%s: tw + 1 + nv = %lld tail columns above %d", who, (long long)tw + 1 + nv, WNP_MAX_TAIL);
        return false;
    }
    return true;
}

extern "C" int64_t msmp_packed_wide_proj_floats(int width, int tw, int nv) {
    const char* who = "msmp_packed_wide_proj_floats";
    if (!wide_width_ok(who, width) || !wide_proj_shape_ok(who, tw, nv) || !wide_proj_tail_ok(who, tw, nv)) return 0;
    return wide_proj_layout((width + 31) / 32, wide_proj_tail_steps(tw, nv)).total;
}

extern "C" int msmp_pack_wide_proj_f32(const float* w1, const float* b1, int width, int tw, int nv, float* packed_out, msmp_stream_t stream) {
    const char* who = "msmp_pack_wide_proj_f32";
    if (!wide_width_ok(who, width) || !wide_proj_shape_ok(who, tw, nv) || !wide_proj_tail_ok(who, tw, nv)) return MSMP_ERR_ARG;
    MSMP_REQUIRE(w1 && b1 && packed_out, MSMP_ERR_ARG, "msmp_pack_wide_proj_f32: null pointer");
    WideProjPackArgs a{w1, b1, width, tw, nv, (width + 31) / 32, wide_proj_tail_steps(tw, nv), packed_out};
    hipLaunchKernelGGL(pack_wide_proj_scale_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(pack_wide_proj_kernel, dim3(128), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("pack_wide_proj_kernel");
}

extern "C" int msmp_wide_node_proj_f32(const float* h, const float* feat, int64_t n_nodes, int tw, int nv, int width, int ld, const float* packed_main,
                                       const float* packed_gate, float* p_main, float* q_main, float* p_gate, float* q_gate, msmp_stream_t stream) {
    const char* who = "msmp_wide_node_proj_f32";
    if (!wide_width_ok(who, width)) return MSMP_ERR_UNSUPPORTED;
    if (!wide_proj_shape_ok(who, tw, nv)) return MSMP_ERR_ARG;
    if (!wide_proj_tail_ok(who, tw, nv)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(ld >= width && ld % 4 == 0 && ld <= 4096, MSMP_ERR_ARG, "msmp_wide_node_proj_f32: ld=%d is not a multiple of 4 in width..4096", ld);
    MSMP_REQUIRE(h && feat && packed_main && p_main && q_main, MSMP_ERR_ARG, "msmp_wide_node_proj_f32: null pointer");
    MSMP_REQUIRE((packed_gate != nullptr) == (p_gate != nullptr) && (packed_gate != nullptr) == (q_gate != nullptr), MSMP_ERR_ARG,
                 "msmp_wide_node_proj_f32: the gate head needs its blob and both outputs (packed_gate, p_gate and q_gate, or none of them)");
    MSMP_REQUIRE(n_nodes >= 0 && n_nodes < (1L << 31) - WNP_TILE, MSMP_ERR_ARG, "msmp_wide_node_proj_f32: bad sizes");
    MSMP_REQUIRE(((uintptr_t)h | (uintptr_t)feat | (uintptr_t)packed_main | (uintptr_t)packed_gate | (uintptr_t)p_main | (uintptr_t)q_main |
                  (uintptr_t)p_gate | (uintptr_t)q_gate) % 16 == 0,
                 MSMP_ERR_ARG, "msmp_wide_node_proj_f32: h, feat, packed, p and q must be 16-byte aligned");
    if (n_nodes == 0) return MSMP_OK;
    const int kt = (width + 31) / 32, ts = wide_proj_tail_steps(tw, nv);
    const WideProjLayout L = wide_proj_layout(kt, ts);
    auto head = [&](const float* packed, float* p, float* q) {
        if (!packed) return WideProjHead{nullptr, nullptr, nullptr, nullptr, nullptr};
        return WideProjHead{packed + L.scales, packed + L.b1, reinterpret_cast<const half8*>(packed + L.w), p, q};
    };
    WideProjArgs a{h, feat, (int)n_nodes, width, ld, msmp_node_feature_stride(tw, nv), tw + 1 + nv, head(packed_main, p_main, q_main),
                   head(packed_gate, p_gate, q_gate), status_ptr()};
    const long n_tiles = (n_nodes + WNP_TILE - 1) / WNP_TILE;
    dispatch_kt(kt, [&](auto K) {
        dispatch_kt(ts, [&](auto S) {       // (the same 1 .. 8)
            constexpr int KT = decltype(K)::value, TS = decltype(S)::value;
            const long resident = resident_workgroups(device_cus(), wnp_lds_bytes(KT, TS), KT);         // persistent
            const unsigned grid = (unsigned)(n_tiles < resident ? n_tiles : resident);
            hipLaunchKernelGGL((wide_node_proj_kernel<KT, TS>), dim3(grid), dim3(64 * KT), 0, (hipStream_t)stream, a);
        });
    });
    return check_launch("wide_node_proj_kernel");
}
