// The node half of GNN_LayerLin at ANY hidden width W <= 256 as one launch per layer (msmp_wide_node_tail_f32), both heads of a gated pair:
//     z_k = Swish(W3_k [h | agg_k | vars] + b3_k)          update_net_1                 (experiments/models_gnn.py:140-149)
//     y_k = W4_k z_k + b4_k                                update_net_2 (GNN_LayerLin: no activation, no residual)
//     n_k = InstanceNorm per graph and channel (biased variance, eps)                   (:129)
//     out = n_main                                         without a gate head
//     out = (1 - tau) h + tau Swish(n_main),  tau = sigmoid(n_gate)                     (:1486-1489)
// The width-generic path evaluated this per head as a concatenation, two row GEMMs around z and y [N, ld], and then
// msmp_wide_norm_blend_f32 over both y; here nothing node-sized but the inputs and `out` touches memory.  The 128-wide
// node_tail_split_kernel is cut for 4 x 32 channels in every dimension; this is the width-generic edition, with the wave-to-channel
// assignment of wide_message_kernel:
//   * a workgroup has one wave per 32-channel output slice (KT = Wp / 32 waves, Wp = 32 ceil(W / 32)) and handles ONE graph (<= 128
//     nodes = four 32-node MFMA column blocks) at a time, persistent over the graphs; wave T owns channels 32 T .. 32 T + 31 of z and y
//     for every node of the graph, so a channel's InstanceNorm statistics are sums over that wave's accumulator registers and the 32
//     lanes of a half wave: no cross-wave reduction, and the blend is wave-local as well;
//   * the graph is processed as two PAIRS of column blocks (64 nodes).  Per pair the h rows are split into fp16 hi / lo B fragments ONCE
//     for both heads (8 KT KB of LDS); per pair and head the agg rows and the variables follow (8 KT + 4 KB), GEMM 1 runs over
//     K = 2 Wp + 16, Swish(z) is published as B fragments over the agg area (it is dead by then), and GEMM 2 accumulates y into the
//     registers that wait for the statistics: 16 per column block, 64 per head, 128 for a gated pair;
//   * the weights stream: an A fragment (row slice T, k-step) has exactly one consumer wave, so it goes from L2 into that wave's
//     registers through a three-slot ring (as in lem_wide_kernel.hip) and serves the two column blocks of the pair.  Sharing a pass over the
//     weights among all four blocks would halve the L2 traffic but needs 64 more accumulator registers for z beside the 128 of y
//     and K-chunked staging of every operand; with two blocks the stream is 2 KB per wave and k-step against six MFMAs.
//   * update_net_2 is CENTRED per graph and head (as in the 128-wide tail): InstanceNorm removes any per-graph, per-channel
//     constant of y, so GEMM 2 runs on Swish(z_n) - Swish(z_ref), z_ref the graph's first node, from zero accumulators and without b4
//     (the blob keeps b4's place; the kernel never reads it).  The fp32 accumulator of the three-MFMA split rounds relative to what it
//     holds: now the variation of y over the graph, which is what the norm divides by, instead of |y|.  Wave T publishes only its own 32
//     channels of z, so Swish(z_ref) is wave-local: one 32-float LDS row per head and wave behind the fragments, written by the two
//     lanes that hold node 0 in pair 0 and read back (as a broadcast) by the same wave in both pairs; no barrier of its own.
//     The difference is multiplied by 2^6 before its hi / lo split (WNT_Z_SCALE; the Swish operands of the 128-wide path carry the same
//     factor, |difference| < 1024): untrained, Swish(z) is of order 0.02, and the lo half of an unscaled value below 2^-3 is an fp16
//     denormal with an absolute step of 2^-24 -- an operand error that no centring removes and that set the error of this kernel
//     (scripts/diag_wide_tail.py: 7.9e-7 rms per layer pair without the factor, 1.5e-7 with it; numpy float32 2.4e-7).
// Arithmetic of wide_frags.h, with the node rows scaled by 2^8 and split (split8_node) and GEMM 1's accumulators initialised with the scaled bias.
// Rows / columns W .. Wp - 1 of the packed weights and biases are exact zeros.  One workgroup per graph and fixed-order sums: the result
// of a graph does not depend on the batch around it, on its position, or on the run.
#include "wide_frags.h"

namespace msmp {

constexpr int WNT_MAX_NODES = 128;            // four 32-node column blocks
constexpr int WNT_NB = 2;                     // column blocks that share one pass over the weights
constexpr float WNT_Z_SCALE = 64.0f;          // update_net_2's operand Swish(z_n) - Swish(z_ref) is split as this multiple; y carries it too

// LDS of a workgroup of kt waves: the fragments [k-step 4 kt + 1][plane 2][block NB][lane 64] half8, then Swish(z_ref) [head 2][Wp] floats
__host__ __device__ constexpr int wnt_frag_bytes(int kt) { return (4 * kt + 1) * 2 * WNT_NB * 1024; }
__host__ __device__ constexpr int wnt_lds_bytes(int kt) { return wnt_frag_bytes(kt) + 2 * 32 * kt * 4; }

// packed blob (floats): scales [8]: 2^s3, 2^s4, 0, 0, 2^-(s3 + 8), 2^-s4, 0, 0 | b3 2^(s3 + 8) [Wp] | b4 2^s4 [Wp] (unread: centring) |
//   w3: [T KT][k-step 4 KT + 1][plane 2: hi, lo][lane 64][8 halfs], natural k order: k-steps 0 .. 2 KT - 1 the h columns,
//       2 KT .. 4 KT - 1 the agg columns, the last one the variables (k 0 .. nv - 1, zeros above) |
//   w4: [T KT][k-step 2 KT][plane 2][lane 64][8 halfs], acc order (split_k_acc: its B operand is published from accumulators)
struct WideTailLayout {
    int64_t scales, b3, b4, w3, w4, total;
};
__host__ __device__ inline WideTailLayout wide_tail_layout(int kt) {
    WideTailLayout L;
    L.scales = 0;
    L.b3 = 8;
    L.b4 = L.b3 + 32 * kt;
    L.w3 = L.b4 + 32 * kt;
    L.w4 = L.w3 + (int64_t)512 * kt * (4 * kt + 1);
    L.total = L.w4 + (int64_t)1024 * kt * kt;
    return L;
}

struct WideTailPackArgs {
    const float *w3, *b3, *w4, *b4;
    int width, nv, kt;
    float* out;
};

// block 0: (W3, b3), block 1: (W4, b4): scales[i] = 2^s with max(|M|, |b|) 2^s in [16, 32); scales[4] = 2^-(s3 + 8) (the node rows carry
// 2^8), scales[5] = 2^-s4.  grid = 2.
__global__ __launch_bounds__(256) void pack_wide_tail_scale_kernel(WideTailPackArgs a) {
    const int n_w = blockIdx.x == 0 ? a.width * (2 * a.width + a.nv) : a.width * a.width;
    const int sft = block_scale_shift(fmaxf(abs_max_part(blockIdx.x == 0 ? a.w3 : a.w4, n_w), abs_max_part(blockIdx.x == 0 ? a.b3 : a.b4, a.width)));
    if (threadIdx.x == 0) store_scale_group(a.out, blockIdx.x, sft, blockIdx.x == 0 ? 8 : 0);
}

__global__ void pack_wide_tail_kernel(WideTailPackArgs a) {
    const WideTailLayout L = wide_tail_layout(a.kt);
    const float s3 = a.out[L.scales], s4 = a.out[L.scales + 1];
    const int kt = a.kt, W = a.width, nv = a.nv, k1s = 4 * kt + 1, kin = 2 * W + nv;
    const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = tid0; p < 32 * kt; p += stride) {
        a.out[L.b3 + p] = p < W ? a.b3[p] * s3 * 256.0f : 0.f;
        a.out[L.b4 + p] = p < W ? a.b4[p] * s4 : 0.f;
    }
    pack_split_fragments(reinterpret_cast<_Float16*>(a.out + L.w3), (int64_t)kt * k1s, [&](int fr, int lane, int j) {
        const int ks = fr % k1s, T = fr / k1s;
        const int row = 32 * T + (lane & 31), hh = lane >> 5;
        int col = -1;
        if (ks < 4 * kt) {
            const int part = ks >= 2 * kt, k = split_k_natural(ks - part * 2 * kt, hh, j);
            if (k < W) col = part * W + k;
        } else if (hh == 0 && j < nv)
            col = 2 * W + j;
        return row < W && col >= 0 ? a.w3[(size_t)row * kin + col] * s3 : 0.f;
    });
    pack_split_fragments(reinterpret_cast<_Float16*>(a.out + L.w4), (int64_t)2 * kt * kt, [&](int fr, int lane, int j) {
        const int ks = fr % (2 * kt), T = fr / (2 * kt);
        const int row = 32 * T + (lane & 31), k = 32 * (ks >> 1) + split_k_acc(ks & 1, lane >> 5, j);
        return row < W && k < W ? a.w4[(size_t)row * W + k] * s4 : 0.f;
    });
}

struct WideTailHead {
    const float* agg;           // [N, ld]; null: no such head
    const float* scales;
    const float* b3;            // [Wp], scaled
    const half8 *w3, *w4;
};

struct WideTailArgs {
    const float *h, *vars;      // [N, ld], [N, nv]
    const int* graph_ptr;
    int n_nodes, n_graphs, nv, width, ld;
    float eps;
    WideTailHead main, gate;
    float* out;                 // [N, ld]
    int* status;
};

// the A fragments in flight (two k-steps ahead of their MFMAs): slot ks % 3 holds k-step ks
struct WideTailRing {
    half8 h[3], l[3];
};
__device__ __forceinline__ void wnt_ring_start(WideTailRing& r, const half8* w, unsigned lo, int nks) {
    r.h[0] = frag_global(w, 0, lo);
    r.l[0] = frag_global(w, 1, lo);
    if (nks > 1) {
        r.h[1] = frag_global(w, 2, lo);
        r.l[1] = frag_global(w, 3, lo);
    }
}

// acc[blk] += W[32 T .., :] B[:, blk] over NKS k-steps: w this wave's fragment stream (already started in the ring), b_lane the per-lane
// LDS address of fragment (k-step 0, hi, block 0) of [k-step][plane][block][lane] half8
template <int NKS>
__device__ __forceinline__ void wnt_gemm(WideTailRing& r, const half8* w, unsigned lo, const char* b_lane, f32x16 (&acc)[WNT_NB]) {
#pragma unroll
    for (int ks = 0; ks < NKS; ++ks) {
        // fence per k-step: left alone the scheduler hoists the unrolled loop's LDS reads far ahead of their MFMAs
        __builtin_amdgcn_sched_barrier(0);
        if (ks + 2 < NKS) {
            r.h[(ks + 2) % 3] = frag_global(w, (ks + 2) * 2 + 0, lo);
            r.l[(ks + 2) % 3] = frag_global(w, (ks + 2) * 2 + 1, lo);
        }
        const half8 ah = r.h[ks % 3], al = r.l[ks % 3];
#pragma unroll
        for (int blk = 0; blk < WNT_NB; ++blk) {
            const half8 bh = frag_lds(b_lane, (ks * 2 + 0) * WNT_NB + blk), bl = frag_lds(b_lane, (ks * 2 + 1) * WNT_NB + blk);
            split_mfma3(ah, al, bh, bl, acc[blk]);
        }
    }
    __builtin_amdgcn_sched_barrier(0);
}

// wave T's share of a pair's rows of `src` ([N, ld]: h or agg): k-steps 2 T, 2 T + 1 of both column blocks (a 128-byte line per node and
// wave) -> hi / lo B fragments scaled by 2^8 at area_lane + ((k-step 2 + plane) NB + block) KB.  Every address is clamped into the tensor;
// dead nodes (local index >= cnt) and channels >= W become zeros.  `worst`: the largest |value| (track_abs_max).
__device__ __forceinline__ void wnt_stage_rows(const float* src, int ld, int W, int n0, int n_nodes, int cnt, int pbase, int T, int c, int hh,
                                               char* area_lane, unsigned& worst) {
    f32x4 v0[2 * WNT_NB], v1[2 * WNT_NB];
#pragma unroll
    for (int blk = 0; blk < WNT_NB; ++blk) {
        const int node = min(n0 + pbase + 32 * blk + c, n_nodes - 1);
        const float* row = src + (size_t)node * ld;
#pragma unroll
        for (int ss = 0; ss < 2; ++ss) {
            const int k0 = 16 * (2 * T + ss) + 8 * hh;
            v0[ss * WNT_NB + blk] = *reinterpret_cast<const f32x4*>(row + min(k0, ld - 4));
            v1[ss * WNT_NB + blk] = *reinterpret_cast<const f32x4*>(row + min(k0 + 4, ld - 4));
        }
    }
#pragma unroll
    for (int i = 0; i < 2 * WNT_NB; ++i) {
        const int blk = i % WNT_NB, s = 2 * T + i / WNT_NB;
        const int k0 = 16 * s + 8 * hh;
        const bool live = pbase + 32 * blk + c < cnt;
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            x[j] = live && k0 + j < W ? (j < 4 ? v0[i][j] : v1[i][j - 4]) : 0.f;
            track_abs_max(worst, x[j]);
        }
        publish_split<WNT_NB, true>(x, area_lane, s, blk);
    }
}

// the variables of a pair's nodes as ONE natural k-step (k 0 .. nv - 1 on the hh = 0 lanes, zeros elsewhere), scaled by 2^8 like the rows
// beside them: frag_base is the address of fragment (that k-step, hi, block 0)
__device__ __forceinline__ void wnt_stage_vars(const WideTailArgs& a, int n0, int cnt, int pbase, char* frag_base, int tid, int threads) {
    for (int i = tid; i < 64 * WNT_NB; i += threads) {
        const int blk = i >> 6, l = i & 63, ln = pbase + 32 * blk + (l & 31);
        const int node = min(n0 + ln, a.n_nodes - 1);
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = (l < 32 && j < a.nv && ln < cnt) ? a.vars[(size_t)node * a.nv + j] : 0.f;
        half8 hi, lo;
        split8_node(x, hi, lo);
        *reinterpret_cast<half8*>(frag_base + (0 * WNT_NB + blk) * 1024 + l * 16) = hi;
        *reinterpret_cast<half8*>(frag_base + (1 * WNT_NB + blk) * 1024 + l * 16) = lo;
    }
}

// sum over the 32 lanes of a half wave (the nodes of a column block), the same bits in every lane: a + b and b + a round alike
__device__ __forceinline__ float wnt_half_wave_sum(float v) {
#pragma unroll
    for (int m = 1; m < 32; m <<= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// y (accumulators of all four column blocks, still times 1 / inv_scale = 2^s4 WNT_Z_SCALE) -> InstanceNorm over the graph's cnt nodes, in place: two passes, biased
// variance, the formula of wide_norm_blend_kernel.  Register r of lane (c, hh) is channel 32 T + acc_row(r, hh) of node 32 block + c.
__device__ __forceinline__ void wnt_instance_norm(f32x16 (&y)[4], float inv_scale, int cnt, int c, float eps, bool& bad) {
    const float inv_cnt = 1.0f / (float)cnt;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        float s = 0.f;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            y[b][r] *= inv_scale;
            s += 32 * b + c < cnt ? y[b][r] : 0.f;
        }
        const float mean = wnt_half_wave_sum(s) * inv_cnt;
        float q = 0.f;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            y[b][r] -= mean;
            q += 32 * b + c < cnt ? y[b][r] * y[b][r] : 0.f;
        }
        const float var = wnt_half_wave_sum(q) * inv_cnt;
        bad |= !(fabsf(mean) <= 3.0e38f) || !(var <= 3.0e38f);
        const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
        for (int b = 0; b < 4; ++b) y[b][r] *= rstd;
    }
}

// one head (HEAD 0: gate, 1: main) on one pair of column blocks: stage agg + vars, GEMM 1, Swish(z) - Swish(z_ref) -> z fragments, GEMM 2
// into y[0 .. 1] (the pair's blocks).  Node 0 of the graph is column c = 0 of block 0 of pair 0: lanes 0 and 32 hold its 16 + 16 channels.
template <int KT, int HEAD>
__device__ __forceinline__ void wnt_head_pair(const WideTailArgs& a, const WideTailHead& hd, int n0, int cnt, int pbase, int T, int c, int hh,
                                              int tid, unsigned lo, char* lds, f32x16& y0, f32x16& y1, unsigned& worst) {
    constexpr int KS = 2 * KT, HB = KS * 2 * WNT_NB * 1024;       // the h area; the agg + vars area (and z over it) follows
    // (the lane offset is made opaque again in every pass: no fragment address formed from it lives longer than the pass)
    asm volatile("" : "+v"(lo));
    const int lane = lo >> 4;
    const half8* const w3 = hd.w3 + (size_t)(T * (2 * KS + 1)) * 128;
    const half8* const w4 = hd.w4 + (size_t)(T * KS) * 128;
    WideTailRing ring;
    wnt_ring_start(ring, w3, lo, 2 * KS + 1);
    wnt_stage_rows(hd.agg, a.ld, a.width, n0, a.n_nodes, cnt, pbase, T, c, hh, lds + HB + lane * 16, worst);
    wnt_stage_vars(a, n0, cnt, pbase, lds + HB + KS * 2 * WNT_NB * 1024, tid, 64 * KT);
    f32x16 z[WNT_NB];
    acc_bias_init(hd.b3 + 32 * T + 4 * hh, z);
    __syncthreads();                // the pair's h, agg and variables fragments are complete
    wnt_gemm<2 * KS + 1>(ring, w3, lo, lds + lane * 16, z);
    wnt_ring_start(ring, w4, lo, KS);
    __syncthreads();                // every wave has read the agg area: z may be written over it
    const float inv3 = uniform_ro(hd.scales, 4);
    // this wave's row of Swish(z_ref), in accumulator order: [hh][register]
    float* const zref = reinterpret_cast<float*>(lds + wnt_frag_bytes(KT)) + (HEAD * KT + T) * 32 + 16 * hh;
#pragma unroll
    for (int blk = 0; blk < WNT_NB; ++blk) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = swishf(z[blk][8 * s + j] * inv3);
            if (pbase == 0 && blk == 0) {       // the graph's first node is here: its values stay for this pair and the next
                if (c == 0) {
                    *reinterpret_cast<f32x4*>(zref + 8 * s) = f32x4{v[0], v[1], v[2], v[3]};
                    *reinterpret_cast<f32x4*>(zref + 8 * s + 4) = f32x4{v[4], v[5], v[6], v[7]};
                }
                __builtin_amdgcn_wave_barrier();        // written and read by this wave only
            }
            const f32x4 r0 = *reinterpret_cast<const f32x4*>(zref + 8 * s), r1 = *reinterpret_cast<const f32x4*>(zref + 8 * s + 4);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = (v[j] - (j < 4 ? r0[j] : r1[j - 4])) * WNT_Z_SCALE;
            publish_split<WNT_NB>(v, lds + HB + lane * 16, 2 * T + s, blk);
        }
        __builtin_amdgcn_sched_barrier(0);      // (one column block's activations at a time)
    }
    f32x16 y[WNT_NB];
#pragma unroll
    for (int blk = 0; blk < WNT_NB; ++blk)
#pragma unroll
        for (int r = 0; r < 16; ++r) y[blk][r] = 0.f;       // no b4: InstanceNorm removes it
    __syncthreads();                // z is complete
    wnt_gemm<KS>(ring, w4, lo, lds + HB + lane * 16, y);
    __syncthreads();                // every wave has read z: the next agg rows may be staged over it
    y0 = y[0];
    y1 = y[1];
}

template <int KT>
__global__ __launch_bounds__(64 * KT, 2) void wide_node_tail_kernel(WideTailArgs a) {
    constexpr int KS = 2 * KT;
    // one LDS object: h fragments of the pair [k-step 2 KT][plane][block][lane] | agg fragments + the variables' k-step, later z |
    // Swish(z_ref) [head][Wp]
    __shared__ __attribute__((aligned(16))) char lds[wnt_lds_bytes(KT)];
    const int tid = threadIdx.x;
    const int T = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W = a.width, ld = a.ld;
    const bool gated = a.gate.agg != nullptr;
    unsigned worst = 0;
    bool bad = false;

    for (int g = blockIdx.x; g < a.n_graphs; g += gridDim.x) {
        // everything that depends on the lane is formed again per graph from an opaque copy: as loop invariants the per-lane addresses of
        // the staging loads, the fragments and the stores stay in registers across the whole loop body, which has none to spare
        int lane = tid & 63;
        asm volatile("" : "+v"(lane));
        const int c = lane & 31, hh = lane >> 5;
        const unsigned lo = lane * 16;
        const int n0 = __builtin_amdgcn_readfirstlane(min(max(a.graph_ptr[g], 0), a.n_nodes));
        const int cnt = __builtin_amdgcn_readfirstlane(min(min(a.graph_ptr[g + 1], a.n_nodes) - n0, WNT_MAX_NODES));
        if (cnt <= 0) continue;
        f32x16 ym[4], yg[4];
#pragma unroll
        for (int b = 0; b < 4; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) ym[b][r] = yg[b][r] = 0.f;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            if (64 * p < cnt) {
                // the h rows of the pair, split once for both heads (their last readers are behind the barriers of the previous pair)
                wnt_stage_rows(a.h, ld, W, n0, a.n_nodes, cnt, 64 * p, T, c, hh, lds + lo, worst);
                if (gated) wnt_head_pair<KT, 0>(a, a.gate, n0, cnt, 64 * p, T, c, hh, tid, lo, lds, yg[2 * p], yg[2 * p + 1], worst);
                wnt_head_pair<KT, 1>(a, a.main, n0, cnt, 64 * p, T, c, hh, tid, lo, lds, ym[2 * p], ym[2 * p + 1], worst);
            }
        }
        // the statistics of this wave's channels, then tau in place of the gate head's y
        if (gated) {
            wnt_instance_norm(yg, uniform_ro(a.gate.scales, 5) * (1.0f / WNT_Z_SCALE), cnt, c, a.eps, bad);
#pragma unroll
            for (int b = 0; b < 4; ++b)
#pragma unroll
                for (int r = 0; r < 16; ++r) yg[b][r] = sigmoidf_(yg[b][r]);
        }
        wnt_instance_norm(ym, uniform_ro(a.main.scales, 5) * (1.0f / WNT_Z_SCALE), cnt, c, a.eps, bad);
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            if (32 * b + c < cnt) {
                const size_t row = (size_t)(n0 + 32 * b + c) * ld;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ch = 32 * T + 8 * q + 4 * hh;
                    if (ch < ld) {
                        f32x4 res;
                        if (gated) {
                            const f32x4 hv = *reinterpret_cast<const f32x4*>(a.h + row + ch);
#pragma unroll
                            for (int m = 0; m < 4; ++m) {
                                const float tau = yg[b][4 * q + m];
                                res[m] = (1.0f - tau) * hv[m] + tau * swishf(ym[b][4 * q + m]);
                            }
                        } else {
#pragma unroll
                            for (int m = 0; m < 4; ++m) res[m] = ym[b][4 * q + m];
                        }
#pragma unroll
                        for (int m = 0; m < 4; ++m) res[m] = ch + m < W ? res[m] : 0.f;
                        *reinterpret_cast<f32x4*>(a.out + row + ch) = res;
                    }
                }
            }
        }
        // columns Wp .. ld - 1 of the graph's rows
        {
            const int extra = (ld - 32 * KT) / 4;
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            for (int i = tid; i < cnt * extra; i += 64 * KT)
                *reinterpret_cast<f32x4*>(a.out + (size_t)(n0 + i / extra) * ld + 32 * KT + 4 * (i % extra)) = zero;
        }
    }
    if (node_range_exceeded(worst)) status_raise(a.status, MSMP_STATUS_NODE_SATURATED);
    if (bad) status_raise(a.status, MSMP_STATUS_NONFINITE);
}

}  // namespace msmp

using namespace msmp;

// msmp_tune("wide_tail", 1): the host layer takes this kernel at widths other than 128; 0 (default): concatenation + two row GEMMs +
// msmp_wide_norm_blend_f32.  Faster by 22-25 % per step (profiles/r10a_glu_wide_node_tail.md).  update_net_2 is centred per graph (see the
// head of this file), so b4 does not enter the result; full-depth figures under the switch: profiles/r28a_glu_wide_tail_centred.md

static bool wide_tail_nv_ok(const char* who, int nv) {
    if (nv < 0 || nv > MSMP_MAX_VARS) {
        set_error("%s: nv=%d outside 0..%d", who, nv, MSMP_MAX_VARS);
        return false;
    }
    return true;
}

extern "C" int64_t msmp_packed_wide_tail_floats(int width, int nv) {
    if (!wide_width_ok("msmp_packed_wide_tail_floats", width) || !wide_tail_nv_ok("msmp_packed_wide_tail_floats", nv)) return 0;
    return wide_tail_layout((width + 31) / 32).total;
}

extern "C" int msmp_pack_wide_tail_f32(const float* w3, const float* b3, const float* w4, const float* b4, int width, int nv, float* packed_out,
                                       msmp_stream_t stream) {
    if (!wide_width_ok("msmp_pack_wide_tail_f32", width) || !wide_tail_nv_ok("msmp_pack_wide_tail_f32", nv)) return MSMP_ERR_ARG;
    MSMP_REQUIRE(w3 && b3 && w4 && b4 && packed_out, MSMP_ERR_ARG, "msmp_pack_wide_tail_f32: null pointer");
    WideTailPackArgs a{w3, b3, w4, b4, width, nv, (width + 31) / 32, packed_out};
    hipLaunchKernelGGL(pack_wide_tail_scale_kernel, dim3(2), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(pack_wide_tail_kernel, dim3(128), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("pack_wide_tail_kernel");
}

extern "C" int msmp_wide_node_tail_max_graph_nodes(int width) {
    if (!wide_width_ok("msmp_wide_node_tail_max_graph_nodes", width)) return 0;
    return WNT_MAX_NODES;
}

extern "C" int msmp_wide_node_tail_f32(const float* h, const float* agg_main, const float* agg_gate, const float* vars, const int32_t* graph_ptr,
                                       int64_t n_nodes, int64_t n_graphs, int max_graph_nodes, int nv, int width, int ld, const float* packed_main,
                                       const float* packed_gate, float eps, float* out, msmp_stream_t stream) {
    if (!wide_width_ok("msmp_wide_node_tail_f32", width)) return MSMP_ERR_UNSUPPORTED;
    if (!wide_tail_nv_ok("msmp_wide_node_tail_f32", nv)) return MSMP_ERR_ARG;
    MSMP_REQUIRE(ld >= width && ld % 4 == 0 && ld <= 4096, MSMP_ERR_ARG, "msmp_wide_node_tail_f32: ld=%d is not a multiple of 4 in width..4096", ld);
    MSMP_REQUIRE(h && agg_main && (vars || nv == 0) && graph_ptr && packed_main && out, MSMP_ERR_ARG, "msmp_wide_node_tail_f32: null pointer");
    MSMP_REQUIRE((agg_gate != nullptr) == (packed_gate != nullptr), MSMP_ERR_ARG,
                 "msmp_wide_node_tail_f32: the gate head needs both its aggregate and its blob (agg_gate and packed_gate, or neither)");
    MSMP_REQUIRE(n_nodes >= 0 && n_nodes < (1L << 31) && n_graphs >= 0 && n_graphs < (1L << 31) && max_graph_nodes >= 0, MSMP_ERR_ARG,
                 "msmp_wide_node_tail_f32: bad sizes");
    MSMP_REQUIRE(((uintptr_t)h | (uintptr_t)agg_main | (uintptr_t)agg_gate | (uintptr_t)out | (uintptr_t)packed_main | (uintptr_t)packed_gate) % 16 == 0,
                 MSMP_ERR_ARG, "msmp_wide_node_tail_f32: h, agg, packed and out must be 16-byte aligned");
    if (max_graph_nodes > WNT_MAX_NODES) {
        set_error("msmp_wide_node_tail_f32: max_graph_nodes=%d above %d (take the row GEMMs and msmp_wide_norm_blend_f32)", max_graph_nodes, WNT_MAX_NODES);
        return MSMP_ERR_UNSUPPORTED;
    }
    if (n_nodes == 0 || n_graphs == 0) return MSMP_OK;
    const int kt = (width + 31) / 32;
    const WideTailLayout L = wide_tail_layout(kt);
    auto head = [&](const float* agg, const float* packed) {
        if (!packed) return WideTailHead{nullptr, nullptr, nullptr, nullptr, nullptr};
        return WideTailHead{agg, packed + L.scales, packed + L.b3, reinterpret_cast<const half8*>(packed + L.w3),
                            reinterpret_cast<const half8*>(packed + L.w4)};
    };
    WideTailArgs a{h, vars, graph_ptr, (int)n_nodes, (int)n_graphs, nv, width, ld, eps, head(agg_main, packed_main), head(agg_gate, packed_gate), out,
                   status_ptr()};
    dispatch_kt(kt, [&](auto K) {
        constexpr int KT = decltype(K)::value;
        const long resident = resident_workgroups(device_cus(), wnt_lds_bytes(KT), KT);       // persistent (LDS: 16 KT + 4 KB of fragments + 256 KT B)
        const unsigned grid = (unsigned)(a.n_graphs < resident ? a.n_graphs : resident);
        hipLaunchKernelGGL((wide_node_tail_kernel<KT>), dim3(grid), dim3(64 * KT), 0, (hipStream_t)stream, a);
    });
    return check_launch("wide_node_tail_kernel");
}
