// The scaffold of the recurrent TRAINING kernel pairs: a T-step recurrence of four gates with its per-step activations saved, and its
// back-propagation through time, one kernel each.  A CELL (LemCell of lem_wide_train_kernel.hip, LstmCell of lstm_train_kernel.hip) describes
// its equations: which matrix element a (gate, row, column) names, the pointwise work of a forward step and of a BPTT step.  Everything around
// them is here, once: the blob layout and the pack kernel, the workgroup's context, the accumulator init, the weight stream and the products,
// the dG writes, the argument checks and the launches.
//
// Workgroup shape: one 32-node tile per workgroup, 64 KT threads, KT = ceil(W / 32); wave ct owns channel tile ct (32 of the Wp = 32 KT
// channels) of every gate and of every carried tensor, in accumulator layout (one node per lane), for all T steps, so the pointwise cell is
// wave-local.  A GEMM needs all Wp channels of its B operand (a state forward, a gate gradient backward): the operand tensor is PUBLISHED in
// LDS as bf16 hi / mid / lo MFMA fragments in "acc order" (K step s of k-tile kt of a lane is registers 8 s .. 8 s + 7 of wave kt's accumulator
// tile, so a publish is a register split + three 16-byte stores, no transposition; 6 KB per k-tile, 6 KT KB per tensor; ONE area, reused
// between barriers), and every wave multiplies its own 32 rows of the weight block -- bf16x3 A fragments streamed from the L2-resident blob
// through buffer loads, one k-tile (6 KB per wave) ahead in consumption order, nothing staged: a wave needs only ITS 32 rows -- with all
// published fragments: six v_mfma_f32_32x32x16_bf16 per K = 16 step, fp32-exact products (mfma_tiles.h).  No fp16 anywhere, so there is no
// input range and the kernels neither read nor raise the range status.  (The first edition, 128 wide only: v_mfma_f32_32x32x2_f32 with every
// 16-KB weight chunk staged through LDS, 19 barriers and 256 KB of staging per time step; this shape cut the matrix time per node 2.7x.)
// Node tiles per workgroup: two (64 nodes, 228 / 247 registers at width 128, two workgroups per CU) halve the weight-fragment traffic but
// measured the same as one (three workgroups per CU): 30.3 vs 30.0 ms per batch-512 LEM training iteration.
// Channels W .. Wp - 1 carry zero weights and zero bias; a cell keeps its states exact zeros there (its head says how), their dG is an exact
// zero, and they are never written to the state outputs.  A node's arithmetic depends on nothing but its own row.
//
// Memory layouts (all fp32; "position" is the place of a gate in a wave's stream, the order the cell consumes its products in):
//   forward blob, kt = ceil(W / 32), Wp = 32 kt, zero outside the matrices:
//     rec  [wave ct kt][position 4][k-tile kc kt][s 2][plane 3: hi, mid, lo][lane 64][8 bf16]: rows 32 ct .. of the gate's recurrent block,
//          columns 32 kc .., as bf16x3 A fragments in acc order (split_k_acc); a wave's stream of one time step is contiguous |
//     wx   [position 4][ct kt][s 4][lane 64]: the input columns as v_mfma_f32_32x32x2_f32 A fragments, row 32 ct + (lane & 31), input
//          feature 2 s + (lane >> 5) |
//     bias [position 4][Wp]
//   backward blob: rec_t, as rec with the positions of the BPTT and fragment row 32 ct + m, column 32 kc + kk  =  M_gate[32 kc + kk][32 ct + m],
//          M the gate's recurrent block: the TRANSPOSED blocks
//   saved  [6][N][T][Wp]            the cell's planes; every element is written
//   dG     [N][T][4][ldg]           ldg = 128 ceil(W / 128); the cell's gate order; columns W .. ldg - 1 are written as 0
#pragma once
#include "lem_layout.h"       // LEM_MAX_INP, tanhf_, sigmoidf_
#include "train_frags.h"      // the tile, publish and fragment pieces (shared with mlp_train_kernel.hip)

namespace msmp {

constexpr int RT_PLANES = 6;

struct RtLayout {
    int64_t rec, wx, bias, total;
};
__host__ __device__ inline RtLayout rt_layout(int kt) {
    RtLayout L;
    L.rec = 0;
    L.wx = L.rec + (int64_t)4 * kt * kt * LWT_KTILE_FLOATS;
    L.bias = L.wx + (int64_t)4 * kt * 256;
    L.total = L.bias + (int64_t)4 * kt * 32;
    return L;
}
__host__ __device__ inline int64_t rt_bwd_floats(int kt) { return (int64_t)4 * kt * kt * LWT_KTILE_FLOATS; }

struct RtPackArgs {
    const float* p[4];      // the cell's four parameter tensors, in the order of its pack entry
    int ninp, width, kt;
    float* out;
};

// TRANSPOSED = false: the forward blob; true: the backward blob (only the tensors that hold recurrent blocks are read).  One thread per (ct,
// position, kc, s, lane).  The Cell names gates in its own numbering: fwd_gate / bwd_gate (position), and rec / input (gate, row, column):
// the ADDRESS of that element, by arithmetic on ONE selected pointer; bias (gate, row): its value.  Every element is then read by ONE load at
// an index clamped to 0 outside the matrix and selected against zero afterwards: as a chain of conditional loads from several matrices, the
// wx loop below was compiled into divergent blocks in which the lanes of one gate reached the load with neither the matrix nor the row
// assigned (read in the gfx950 assembly of the LEM's first edition: a wild address, the kernel faulted on first use).
template <class Cell, bool TRANSPOSED>
__global__ __launch_bounds__(256) void pack_recurrent_train_kernel(RtPackArgs a) {
    const int kt = a.kt, W = a.width;
    const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t n_rec = (int64_t)4 * kt * kt * 2 * 64;
    for (int64_t p = tid0; p < n_rec; p += stride) {
        const int lane = (int)(p & 63), s = (int)(p >> 6) & 1;
        const int64_t q = p >> 7;
        const int kc = (int)(q % kt), pos = (int)((q / kt) & 3), ct = (int)(q / (4 * kt));
        const int row = 32 * ct + (lane & 31);
        const int gate = TRANSPOSED ? Cell::bwd_gate(pos) : Cell::fwd_gate(pos);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 32 * kc + split_k_acc(s, lane >> 5, j);
            const bool inside = row < W && k < W;
            const int r = inside ? (TRANSPOSED ? k : row) : 0, c = inside ? (TRANSPOSED ? row : k) : 0;
            const float w = *Cell::rec(a, gate, r, c);
            v[j] = inside ? w : 0.f;
        }
        lwt_store_b3(a.out, p >> 6, lane, v);
    }
    if (TRANSPOSED) return;
    const RtLayout L = rt_layout(kt);
    for (int64_t p = tid0; p < (int64_t)4 * kt * 256; p += stride) {
        const int lane = (int)(p & 63), s = (int)(p >> 6) & 3, ct = (int)((p >> 8) % kt), pos = (int)((p >> 8) / kt);
        const int row = 32 * ct + (lane & 31), f = 2 * s + (lane >> 5);
        const bool inside = row < W && f < a.ninp;
        const float w = *Cell::input(a, Cell::fwd_gate(pos), inside ? row : 0, inside ? f : 0);
        a.out[L.wx + p] = inside ? w : 0.f;
    }
    for (int64_t p = tid0; p < (int64_t)4 * kt * 32; p += stride) {
        const int row = (int)(p % (32 * kt)), pos = (int)(p / (32 * kt));
        const float b = Cell::bias(a, Cell::fwd_gate(pos), row < W ? row : 0);
        a.out[L.bias + p] = row < W ? b : 0.f;
    }
}

// Cell::Scalars: the cell's scalar constants (the LEM's dt; none for the LSTM).  h is the state the forward publishes (LEM y), c the other one
// (LEM z).
template <class Cell>
struct RtFwdArgs {
    const float* xin;       // [N, T, stride]
    long n_nodes;
    int t_len, stride, width;
    typename Cell::Scalars k;
    const float *rec, *wx, *bias;
    float* saved;           // [6][N][T][Wp] or NULL
    const float *h0, *c0;   // [N, W] or NULL (zeros)
    float *h_out, *c_out;   // [N, W]; c_out may be NULL
};
template <class Cell>
struct RtBwdArgs {
    const float* gout;      // [N, W] dL/dh_T
    const float* saved;     // [6][N][T][Wp]
    long n_nodes;
    int t_len, width, ldg;
    typename Cell::Scalars k;
    const float* rec_t;
    float* dg;              // [N][T][4][ldg]
    const float* c0;        // the forward's initial c [N, W] (NULL = zeros); h0 is in the saved plane of the entering h
};

// the stream of wave ct: [position 4][k-tile KT] k-tiles of LWT_KTILE_FLOATS, 4 KT * LWT_KTILE_FLOATS floats per wave
template <int KT>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t lwt_stream(const float* rec, int ct_uniform) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(rec + (size_t)ct_uniform * (4 * KT * LWT_KTILE_FLOATS)), 0, 4 * KT * LWT_KTILE_FLOATS * 4,
                                             0x00027000);
}
// one GEMM: the KT k-tiles of stream position GRP against the tensor currently published.  The k-tile after each one is requested before its
// MFMAs (the first of the next position after the last; after position 3 the stream wraps to the next time step), so a GEMM starts with its
// first k-tile in registers.  wA / wB alternate by stream index (4 KT is even: index 0 is always wA).
template <int KT, int GRP>
__device__ __forceinline__ void lwt_gemm(LwtFrag& wA, LwtFrag& wB, __amdgpu_buffer_rsrc_t stream, const u32x4* xf, int lane, unsigned loff, f32x16& acc) {
#pragma unroll
    for (int kc = 0; kc < KT; ++kc) {
        const int i = GRP * KT + kc;
        LwtFrag& cur = (i & 1) ? wB : wA;
        LwtFrag& nxt = (i & 1) ? wA : wB;
        lwt_frag_load(nxt, stream, (i + 1) % (4 * KT), loff);
        lwt_mma(cur, xf, kc, lane, acc);
        __builtin_amdgcn_sched_barrier(0);       // one k-tile of weight fragments ahead, not all of them
    }
}

// What a wave knows for all T steps: its lane and tile, its node (nc: clamped, dead lanes compute on the last node and write nothing), its
// weight stream with the two fragment buffers, and the published area.  The fragment offset loff goes through an empty asm so that the
// compiler cannot fold the lane into the 96 fragment addresses of a step (it would hold them in registers across the t loop).
template <int KT>
struct RtWave {
    static constexpr int WP = 32 * KT;
    int lane, ct, hh, W;
    size_t plane;           // floats of one plane of saved
    __amdgpu_buffer_rsrc_t stream;
    long n, nc;
    bool live;
    u32x4* xf;
    LwtFrag wA, wB;
    unsigned loff;
};
template <int KT, int NS>
struct RtFwd : RtWave<KT> {
    int stride, ns;
    bool save;
    const float *xrow, *wx, *bias;
    float* srow;            // the node's rows of saved (+ 4 hh)
};
template <int KT>
struct RtBwd : RtWave<KT> {
    int ldg;
    const float* srow;
    float* grow;            // the node's rows of dG (+ 4 hh)
};
template <int KT>
__device__ __forceinline__ void rt_decode(RtWave<KT>& c, u32x4* xf, long n_nodes, int t_len, int width, const float* rec) {
    const int tid = threadIdx.x;
    c.lane = tid & 63;
    c.ct = __builtin_amdgcn_readfirstlane(tid >> 6);
    c.hh = c.lane >> 5;
    c.W = width;
    c.plane = (size_t)n_nodes * t_len * c.WP;
    c.stream = lwt_stream<KT>(rec, c.ct);
    c.n = (long)blockIdx.x * 32 + (c.lane & 31);
    c.live = c.n < n_nodes;
    c.nc = c.live ? c.n : n_nodes - 1;
    c.xf = xf;
}
template <int KT>
__device__ __forceinline__ void rt_first_fragment(RtWave<KT>& c) {
    c.loff = 16u * c.lane;
    asm volatile("" : "+v"(c.loff));
    lwt_frag_load(c.wA, c.stream, 0, c.loff);
}
// acc += (recurrent block at stream position POS) (the published tensor)
template <int POS, int KT>
__device__ __forceinline__ void rt_gemm(RtWave<KT>& c, f32x16& acc) {
    lwt_gemm<KT, POS>(c.wA, c.wB, c.stream, c.xf, c.lane, c.loff, acc);
}
template <int KT>
__device__ __forceinline__ void rt_publish(const RtWave<KT>& c, const f32x16& v) {
    lwt_publish(c.xf, c.ct, c.lane, v);
}

// The forward's prologue: h, c = the initial states (zeros without), h published, the first k-tile requested.  NS = 0: the input stride is
// a.stride, read at run time.  NS > 0: it is the compile-time constant 2 NS of the whole body (rt_forward below).
template <int KT, int NS, class Args>
__device__ __forceinline__ void rt_fwd_begin(RtFwd<KT, NS>& c, const Args& a, u32x4* xf, f32x16& h, f32x16& cs) {
    rt_decode(c, xf, a.n_nodes, a.t_len, a.width, a.rec);
    c.stride = NS ? 2 * NS : a.stride;
    c.ns = c.stride >> 1;
    c.save = c.live && a.saved != nullptr;
    c.xrow = a.xin + (size_t)c.nc * a.t_len * c.stride + (NS ? c.hh : 0);
    c.srow = a.saved + (size_t)c.nc * a.t_len * c.WP + 4 * c.hh;
    c.wx = a.wx;
    c.bias = a.bias;
#pragma unroll
    for (int r = 0; r < 16; ++r) { h[r] = 0.f; cs[r] = 0.f; }
    if (a.h0) lwt_dense_load(a.h0 + (size_t)c.nc * c.W, c.ct, c.hh, c.W, h);
    if (a.c0) lwt_dense_load(a.c0 + (size_t)c.nc * c.W, c.ct, c.hh, c.W, cs);
    lwt_publish(xf, c.ct, c.lane, h);
    rt_first_fragment(c);
    __syncthreads();
}
template <int KT, int NS, class Args>
__device__ __forceinline__ void rt_fwd_end(const RtFwd<KT, NS>& c, const Args& a, const f32x16& h, const f32x16& cs) {
    if (c.live) {
        lwt_dense_store(a.h_out + (size_t)c.n * c.W, c.ct, c.hh, c.W, h);
        if (a.c_out) lwt_dense_store(a.c_out + (size_t)c.n * c.W, c.ct, c.hh, c.W, cs);
    }
}

// The inputs of step t: NS > 0: x[s] = feature 2 s + hh of the lane's node; NS = 0: x[f] = feature f (zero past the stride); and the step's
// row of saved.  NS > 0: the input-column fragments are the same in every step; read through an offset the compiler cannot see through
// (wlane), they are loaded where they are used (L1 hits) instead of being held in 4 NS registers for the whole loop: a LEM body alone needs at
// most 164 registers, not 176, and the kernel of the four bodies 168, which is three workgroups per CU instead of two (with two, the LEM
// forward with saving of 51 200 nodes took 1.74 ms, not 1.63).
template <int NS>
struct RtStep {
    float x[NS ? NS : 8];
    float* st;
    int wlane;
};
template <int KT, int NS>
__device__ __forceinline__ void rt_step_begin(const RtFwd<KT, NS>& c, int t, RtStep<NS>& in) {
#pragma unroll
    for (int f = 0; f < (NS ? NS : 8); ++f) {
        if constexpr (NS != 0) in.x[f] = c.xrow[(size_t)t * c.stride + 2 * f];
        else in.x[f] = f < c.stride ? c.xrow[(size_t)t * c.stride + f] : 0.f;
    }
    in.st = c.srow + (size_t)t * c.WP;
    in.wlane = c.lane;
    if constexpr (NS != 0) asm volatile("" : "+v"(in.wlane));
}
template <int KT, int NS>
__device__ __forceinline__ void rt_save(const RtFwd<KT, NS>& c, const RtStep<NS>& in, int plane, const f32x16& v) {
    if (c.save) lwt_tile_store(in.st + plane * c.plane, c.ct, v);
}
// acc (tile ct) = bias + (input columns) x_t of the gate at stream position pos: the input columns as ceil(ninp / 2) fp32 MFMA k-steps (the
// pad of an odd ninp is zero)
template <int KT, int NS>
__device__ __forceinline__ void rt_tile_init(const RtFwd<KT, NS>& c, int pos, const RtStep<NS>& in, f32x16& acc) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(c.bias + (pos * KT + c.ct) * 32 + 8 * q + 4 * c.hh);
#pragma unroll
        for (int m = 0; m < 4; ++m) acc[4 * q + m] = bv[m];
    }
    const float* wf = c.wx + (size_t)(pos * KT + c.ct) * 256 + in.wlane;
#pragma unroll
    for (int s = 0; s < (NS ? NS : 4); ++s) {
        if constexpr (NS != 0) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[s * 64], in.x[s], acc, 0, 0, 0);
        else if (s < c.ns) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(wf[s * 64], c.hh ? in.x[2 * s + 1] : in.x[2 * s], acc, 0, 0, 0);
    }
}

// The forward kernel's body: Cell::forward<KT, NS>.  At KT = 4 (the flagship width) the kernel holds a body for each NS = stride / 2 and
// branches once: at run time the step-input loads and the input-column MFMAs of every step sit behind branches, which at width 128 cost the
// LEM forward 5 % (51 200 nodes) to 13 % (1 600 nodes) against the retired 128-wide kernel, whose NS was a template argument too
// (profiles/r19a_one_lem_training_pair.md).  The other KT keep the run-time body: with four bodies per kernel they would hold 167 - 176
// registers instead of 149 - 160 and lose a workgroup per CU.
template <class Cell, int KT>
__device__ __forceinline__ void rt_forward(const RtFwdArgs<Cell>& a, u32x4* xf) {
    if constexpr (KT == 4) {
        switch (a.stride >> 1) {
            case 1: Cell::template forward<KT, 1>(a, xf); break;
            case 2: Cell::template forward<KT, 2>(a, xf); break;
            case 3: Cell::template forward<KT, 3>(a, xf); break;
            default: Cell::template forward<KT, 4>(a, xf); break;
        }
    } else {
        Cell::template forward<KT, 0>(a, xf);
    }
}

// The BPTT's prologue: dh = dL/dh_T, dc = 0, the first k-tile requested
template <int KT, class Args>
__device__ __forceinline__ void rt_bwd_begin(RtBwd<KT>& c, const Args& a, u32x4* xf, f32x16& dh, f32x16& dc) {
    rt_decode(c, xf, a.n_nodes, a.t_len, a.width, a.rec_t);
    c.ldg = a.ldg;
    c.srow = a.saved + (size_t)c.nc * a.t_len * c.WP + 4 * c.hh;
    c.grow = a.dg + (size_t)c.nc * a.t_len * (4 * c.ldg) + 4 * c.hh;
    lwt_dense_load(a.gout + (size_t)c.nc * c.W, c.ct, c.hh, c.W, dh);
#pragma unroll
    for (int r = 0; r < 16; ++r) dc[r] = 0.f;
    rt_first_fragment(c);
}
// plane `plane` of step t of saved (st: the step's row)
template <int KT>
__device__ __forceinline__ void rt_saved(const RtBwd<KT>& c, const float* st, int plane, f32x16& v) {
    lwt_tile_load(st + plane * c.plane, c.ct, v);
}
// the c that ENTERED step t: plane `plane` of step t - 1, at t = 0 the forward's initial c
template <int KT>
__device__ __forceinline__ void rt_entering_c(const RtBwd<KT>& c, const float* st, int t, int plane, const float* c0, f32x16& v) {
    if (t > 0) lwt_tile_load(st - c.WP + plane * c.plane, c.ct, v);
    else if (c0) lwt_dense_load(c0 + (size_t)c.nc * c.W, c.ct, c.hh, c.W, v);
    else {
#pragma unroll
        for (int r = 0; r < 16; ++r) v[r] = 0.f;
    }
}
// columns Wp .. ldg - 1 of all four gates of step row gt: zeros (the weight-gradient jobs read whole 128-column blocks)
template <int KT>
__device__ __forceinline__ void rt_dg_pad(const RtBwd<KT>& c, float* gt) {
    f32x16 zero;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero[r] = 0.f;
    for (int T2 = KT + c.ct; T2 < (c.ldg >> 5) && c.live; T2 += KT)
#pragma unroll
        for (int gi = 0; gi < 4; ++gi) lwt_tile_store(gt + gi * c.ldg, T2, zero);
}
// One gate gradient p: written to dG (gt_gate: the gate's columns of the step row); published, and acc += M_gate^T p (stream position POS);
// rt_gate_product is the two in a row.  The LEM writes both gradients of a pointwise block before their products and the liveness test of
// rt_dg_pad sits in the loop condition: either way round the compiler's register allocation of a BPTT kernel moves by up to 12 registers
// (profiles/r24a_recurrent_scaffold.md).
template <int KT>
__device__ __forceinline__ void rt_dg_write(const RtBwd<KT>& c, float* gt_gate, const f32x16& p) {
    if (c.live) lwt_tile_store(gt_gate, c.ct, p);
}
template <int POS, int KT>
__device__ __forceinline__ void rt_product(RtBwd<KT>& c, const f32x16& p, f32x16& acc) {
    lwt_publish(c.xf, c.ct, c.lane, p);          // the area is free: the previous product ended with a barrier
    __syncthreads();
    rt_gemm<POS>(c, acc);
    __syncthreads();
}
template <int POS, int KT>
__device__ __forceinline__ void rt_gate_product(RtBwd<KT>& c, float* gt_gate, const f32x16& p, f32x16& acc) {
    rt_dg_write(c, gt_gate, p);
    rt_product<POS>(c, p, acc);
}

// ---- host side: the checks and launches of the eight entries of a cell; `who` is the entry, named in every message ----

inline bool rt_shape_ok(const char* who, int ninp, int width) {
    if (!wide_width_ok(who, width)) return false;
    if (ninp < 1 || ninp > LEM_MAX_INP) {
        set_error("%s: ninp=%d outside 1..%d", who, ninp, LEM_MAX_INP);
        return false;
    }
    return true;
}
inline bool rt_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

inline int64_t rt_packed_floats(const char* who, int ninp, int width, bool transposed) {
    if (!rt_shape_ok(who, ninp, width)) return 0;
    return transposed ? rt_bwd_floats((width + 31) / 32) : rt_layout((width + 31) / 32).total;
}
// floats of saved, or of dG, for n_nodes * t_len rows
inline int64_t rt_rows_floats(const char* who, int64_t n_nodes, int t_len, int width, bool dg) {
    if (!wide_width_ok(who, width)) return 0;
    if (n_nodes < 0 || n_nodes >= (1L << 31) || t_len < 1) {
        set_error("%s: bad sizes", who);
        return 0;
    }
    return n_nodes * t_len * (dg ? (int64_t)4 * (128 * ((width + 127) / 128)) : (int64_t)RT_PLANES * (32 * ((width + 31) / 32)));
}

template <class Cell, bool TRANSPOSED>
int rt_pack(const char* who, const char* kernel, bool pointers, RtPackArgs a, msmp_stream_t stream) {
    if (!rt_shape_ok(who, a.ninp, a.width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(pointers && a.out, MSMP_ERR_ARG, "%s: null pointer", who);
    MSMP_REQUIRE(rt_aligned16(a.out), MSMP_ERR_ARG, "%s: packed_out is not 16-byte aligned", who);
    hipLaunchKernelGGL((pack_recurrent_train_kernel<Cell, TRANSPOSED>), dim3(2 * a.kt * a.kt), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch(kernel);
}

// kernel_of(std::integral_constant<int, KT>) = the cell's kernel for that KT
template <class Args, class KernelOf>
int rt_launch(const char* kernel, const Args& a, int64_t n_nodes, int width, msmp_stream_t stream, KernelOf kernel_of) {
    const unsigned grid = (unsigned)((n_nodes + 31) / 32);
    hipStream_t st = (hipStream_t)stream;
    dispatch_kt((width + 31) / 32, [&](auto K) {
        constexpr int KT = decltype(K)::value;
        hipLaunchKernelGGL(kernel_of(K), dim3(grid), dim3(64 * KT), 0, st, a);
    });
    return check_launch(kernel);
}

// the forward entry; MSMP_OK with nothing launched: no nodes
template <class Cell, class KernelOf>
int rt_fwd_entry(const char* who, const char* kernel, const float* xin, int64_t n_nodes, int t_len, int ninp, int width, typename Cell::Scalars k,
                 const float* packed, const float* h0, const float* c0, float* saved, float* h_out, float* c_out, msmp_stream_t stream,
                 KernelOf kernel_of) {
    if (!rt_shape_ok(who, ninp, width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(t_len >= 1, MSMP_ERR_ARG, "%s: t_len=%d < 1", who, t_len);
    MSMP_REQUIRE(n_nodes >= 0 && n_nodes < (1L << 31), MSMP_ERR_ARG, "%s: bad n_nodes", who);
    MSMP_REQUIRE(xin && packed && h_out, MSMP_ERR_ARG, "%s: null pointer", who);
    MSMP_REQUIRE((h0 == nullptr) == (c0 == nullptr), MSMP_ERR_ARG, "%s: give both initial states or none", who);
    MSMP_REQUIRE(rt_aligned16(packed) && rt_aligned16(saved), MSMP_ERR_ARG, "%s: packed / saved not 16-byte aligned", who);
    if (n_nodes == 0) return MSMP_OK;
    const RtLayout L = rt_layout((width + 31) / 32);
    RtFwdArgs<Cell> a{xin, (long)n_nodes, t_len, msmp_lem_input_stride(ninp), width, k, packed + L.rec, packed + L.wx, packed + L.bias,
                      saved, h0, c0, h_out, c_out};
    return rt_launch(kernel, a, n_nodes, width, stream, kernel_of);
}

// the BPTT entry behind the cell's own first checks (width, t_len, its scalars); states_paired: the cell's condition on the initial states
template <class Cell, class KernelOf>
int rt_bwd_entry(const char* who, const char* kernel, const float* gout, const float* saved, const float* c0, bool states_paired, int64_t n_nodes,
                 int t_len, int width, typename Cell::Scalars k, const float* packed_bwd, float* dg_out, msmp_stream_t stream, KernelOf kernel_of) {
    MSMP_REQUIRE(n_nodes >= 0 && n_nodes < (1L << 31), MSMP_ERR_ARG, "%s: bad n_nodes", who);
    MSMP_REQUIRE(gout && saved && packed_bwd && dg_out, MSMP_ERR_ARG, "%s: null pointer", who);
    MSMP_REQUIRE(states_paired, MSMP_ERR_ARG, "%s: give both initial states or none", who);
    MSMP_REQUIRE(rt_aligned16(packed_bwd) && rt_aligned16(saved) && rt_aligned16(dg_out), MSMP_ERR_ARG,
                 "%s: packed_bwd / saved / dg_out not 16-byte aligned", who);
    if (n_nodes == 0) return MSMP_OK;
    RtBwdArgs<Cell> a{gout, saved, (long)n_nodes, t_len, width, 128 * ((width + 127) / 128), k, packed_bwd, dg_out, c0};
    return rt_launch(kernel, a, n_nodes, width, stream, kernel_of);
}

}  // namespace msmp
