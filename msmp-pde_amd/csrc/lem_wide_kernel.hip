// LEM node encoder at ANY hidden width W <= 256 as one launch (msmp_lem_encoder_wide_f32): the T-step recurrence of the cell restated in
// lem.py (experiments/models_gnn.py:285-342), from initial states (y0, z0) to (y_T, z_T).  The 128-wide kernels of lem_kernel.hip keep the
// four gate matrices in the register file; at the GLU classes' width (164, padded to Wp = 192) they are 4 Wp^2 fp16 hi + lo = 590 KB, more
// than a CU has, so here the STATE is stationary and the WEIGHTS stream:
//   * a workgroup carries LEMW_NT = 2 node tiles of 32 nodes and has one wave per 32-channel slice (KT = Wp / 32 waves, 64 KT threads);
//     wave T computes rows 32 T .. 32 T + 31 of all four gates for both tiles and owns those channels of y and z (fp32, accumulator
//     layout, in registers for all T steps), so every state update is wave-local;
//   * the states are published after every update as fp16 hi / lo B fragments in LDS (2 states x 2 tiles x Wp x 32 x 2 planes x 2 B =
//     16 KT KB: 128 KB at Wp = 256), read by every wave as the B operand of the next GEMMs;
//   * an A fragment (gate g, slice T, k-step) has exactly ONE consumer wave in the workgroup, so it goes from L2 straight into that
//     wave's registers through a three-slot ring (two k-steps ahead), and is used for both node tiles; the LDS has no room for a second
//     copy of the weights beside the states, and staging them there would add a write and a read per fragment for no reuse.
// Fragments and the three-MFMA step are those of wide_frags.h; bias + W[:, W:] x_t enter as one or two
// K = 16 "slot" MFMAs on a zero accumulator (lem_slot_feature, lem_layout.h), and s(a) tanh(b) is evaluated with one reciprocal as in
// lem_encoder_ws3_kernel.  Channels W .. Wp - 1 carry zero weights, zero bias and zero state (their update keeps an exact 0) and are
// never written.  A node's arithmetic depends on nothing but its own row: not on the step index, the workgroup or the tile slot.
// Per step:   phase 1  g2, g3 (B = y)            -> z update, publish z      | barrier
//             phase 2  g1 (B = y), lin (B = z)                               | barrier (every wave has read y)
//                      y update, publish y                                   | barrier
#include "lem_layout.h"
#include "wide_frags.h"

namespace msmp {

constexpr int LEMW_NT = 2;          // node tiles per workgroup (registers and LDS allow no third at Wp = 256)

// packed blob (floats): scales [8] (2^s of W, Wz, 0, 0, then 2^-s) |
//   rec: [gate 4: g2, g3, g1, lin][T KT][k-step 2 KT][plane 2: hi, lo][lane 64][8 halfs], acc order (split_k_acc) |
//   wxh: [gate 4][T KT][m 2][lane 64][8 halfs]: the input columns and the bias as slot fragments
struct LemWideLayout {
    int64_t scales, rec, wxh, total;
};
__host__ __device__ inline LemWideLayout lem_wide_layout(int kt) {
    LemWideLayout L;
    L.scales = 0;
    L.rec = 8;
    L.wxh = L.rec + (int64_t)4096 * kt * kt;
    L.total = L.wxh + (int64_t)2048 * kt;
    return L;
}

struct LemWidePackArgs {
    const float *w, *wz, *b, *bz;
    int ninp, width, kt;
    float* out;
};

// scales[i] = 2^s with max(|M_i|, |b_i|) 2^s in [16, 32) for (W, b), (Wz, bz); scales[4 + i] = 2^-s.  grid = 2.
__global__ __launch_bounds__(256) void pack_lem_wide_scale_kernel(LemWidePackArgs a) {
    const int kin = a.width + a.ninp, rows = blockIdx.x == 0 ? 3 * a.width : a.width;
    const int sft = block_scale_shift(fmaxf(abs_max_part(blockIdx.x == 0 ? a.w : a.wz, rows * kin), abs_max_part(blockIdx.x == 0 ? a.b : a.bz, rows)));
    if (threadIdx.x == 0) store_scale_group(a.out, blockIdx.x, sft, 0);
}

// row `row` (< width) of gate g in consumption order: g2, g3, g1 are rows W.., 2W.., 0.. of `weights`, lin is weights_lin_z
__device__ __forceinline__ float lemw_weight(const LemWidePackArgs& a, int g, int row, int col) {
    const int kin = a.width + a.ninp;
    return g == 0 ? a.w[(size_t)(a.width + row) * kin + col] : g == 1 ? a.w[(size_t)(2 * a.width + row) * kin + col]
           : g == 2 ? a.w[(size_t)row * kin + col] : a.wz[(size_t)row * kin + col];
}
__device__ __forceinline__ float lemw_bias(const LemWidePackArgs& a, int g, int row) {
    return g == 0 ? a.b[a.width + row] : g == 1 ? a.b[2 * a.width + row] : g == 2 ? a.b[row] : a.bz[row];
}

__global__ void pack_lem_wide_kernel(LemWidePackArgs a) {
    const LemWideLayout L = lem_wide_layout(a.kt);
    const float* sc = a.out + L.scales;
    const int kt = a.kt, W = a.width, P = a.ninp;
    const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    pack_split_fragments(reinterpret_cast<_Float16*>(a.out + L.rec), (int64_t)8 * kt * kt, [&](int fr, int lane, int j) {
        const int ks = fr % (2 * kt), T = (fr / (2 * kt)) % kt, g = fr / (2 * kt * kt);
        const int row = 32 * T + (lane & 31), k = 32 * (ks >> 1) + split_k_acc(ks & 1, lane >> 5, j);
        return row < W && k < W ? lemw_weight(a, g, row, k) * sc[g < 3 ? 0 : 1] : 0.f;
    });
    _Float16* wh = reinterpret_cast<_Float16*>(a.out + L.wxh);
    const int64_t n_wx = (int64_t)4096 * kt;
    for (int64_t p = tid0; p < n_wx; p += stride) {
        const int j = (int)(p & 7), lane = (int)(p >> 3) & 63, m = (int)(p >> 9) & 1;
        const int fr = (int)(p >> 10), T = fr % kt, g = fr / kt;
        const int slot = 16 * m + 8 * (lane >> 5) + j, f = lem_slot_feature(slot, P), row = 32 * T + (lane & 31);
        _Float16 v = (_Float16)0.f;
        if (row < W) {
            if (slot == 3 * P || slot == 3 * P + 1) {        // bias slots (paired with 1.0)
                const float bv = lemw_bias(a, g, row) * sc[g < 3 ? 0 : 1];
                const _Float16 hi = (_Float16)bv;
                v = slot == 3 * P ? hi : (_Float16)(bv - (float)hi);
            }
            if (f >= 0) {
                const float w = lemw_weight(a, g, row, W + f) * sc[g < 3 ? 0 : 1];
                const _Float16 hi = (_Float16)w;
                v = lem_slot_part(slot, P) < 2 ? hi : (_Float16)(w - (float)hi);
            }
        }
        wh[p] = v;
    }
}

struct LemWideArgs {
    const float* xin;       // [N, T, stride]
    long n_nodes;
    int t_len, ninp, stride, width;
    float dt;
    const float* scales;
    const half8* rec;
    const half8* wxh;
    const float *y0, *z0;   // [N, W] or null (zeros)
    float *y_out, *z_out;   // [N, W]; z_out may be null
    int* status;
};

// the A fragments of two gates in flight (two k-steps ahead of their MFMAs): slot ks % 3 holds k-step ks
struct LemWideRing {
    half8 h0[3], l0[3], h1[3], l1[3];
};
__device__ __forceinline__ void lemw_ring_load(LemWideRing& r, const half8* w0, const half8* w1, unsigned lo, int ks) {
    r.h0[ks % 3] = frag_global(w0, ks * 2 + 0, lo);
    r.l0[ks % 3] = frag_global(w0, ks * 2 + 1, lo);
    r.h1[ks % 3] = frag_global(w1, ks * 2 + 0, lo);
    r.l1[ks % 3] = frag_global(w1, ks * 2 + 1, lo);
}
__device__ __forceinline__ void lemw_ring_start(LemWideRing& r, const half8* w0, const half8* w1, unsigned lo) {
    lemw_ring_load(r, w0, w1, lo, 0);
    lemw_ring_load(r, w0, w1, lo, 1);
}

// acc0[X] = Wx0 bx[X] + W0 B0[X],  acc1[X] = Wx1 bx[X] + W1 B1[X]  over K = Wp for both node tiles (SAME: B1 = B0).
// w0 / w1: this wave's fragment streams of the two gates (wave-uniform), already started in the ring; bx / b0 / b1: per-lane LDS
// addresses of the input fragments and of the two state areas (tile stride 4 KT fragments).
template <int KT, int M, bool SAME>
__device__ __forceinline__ void lemw_gemm2(LemWideRing& r, const half8* w0, const half8* w1, const half8* wx0, const half8* wx1,
                                           const char* bx, const char* b0, const char* b1, unsigned lo, f32x16 (&acc0)[LEMW_NT],
                                           f32x16 (&acc1)[LEMW_NT]) {
    constexpr int KS = 2 * KT, FR = KT * 4;
    {
        half8 x0[M], x1[M];
#pragma unroll
        for (int m = 0; m < M; ++m) {
            x0[m] = frag_global(wx0, m, lo);
            x1[m] = frag_global(wx1, m, lo);
        }
        const f32x16 zero = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int X = 0; X < LEMW_NT; ++X) {
            const half8 v0 = frag_lds(bx, X * M);
            acc0[X] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x0[0], v0, zero, 0, 0, 0);
            acc1[X] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x1[0], v0, zero, 0, 0, 0);
#pragma unroll
            for (int m = 1; m < M; ++m) {
                const half8 vm = frag_lds(bx, X * M + m);
                acc0[X] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x0[m], vm, acc0[X], 0, 0, 0);
                acc1[X] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x1[m], vm, acc1[X], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int ks = 0; ks < KS; ++ks) {
        // fence per k-step: left alone the scheduler hoists the unrolled loop's LDS reads far ahead of their MFMAs and spills
        __builtin_amdgcn_sched_barrier(0);
        if (ks + 2 < KS) lemw_ring_load(r, w0, w1, lo, ks + 2);
        const half8 ah0 = r.h0[ks % 3], al0 = r.l0[ks % 3], ah1 = r.h1[ks % 3], al1 = r.l1[ks % 3];
#pragma unroll
        for (int X = 0; X < LEMW_NT; ++X) {
            const half8 bh0 = frag_lds(b0, X * FR + ks * 2 + 0), bl0 = frag_lds(b0, X * FR + ks * 2 + 1);
            half8 bh1 = bh0, bl1 = bl0;
            if (!SAME) {
                bh1 = frag_lds(b1, X * FR + ks * 2 + 0);
                bl1 = frag_lds(b1, X * FR + ks * 2 + 1);
            }
            split_mfma3(ah0, al0, bh0, bl0, acc0[X]);
            split_mfma3(ah1, al1, bh1, bl1, acc1[X]);
        }
    }
}

// publish a [32 channels x 32 nodes] state tile as the hi / lo B fragments of this wave's two k-steps: `slice` is the per-lane LDS
// address of fragment (k-step 2 T, hi) of the tile's area
__device__ __forceinline__ void lemw_publish(const f32x16& st, char* slice) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = st[8 * s + j];
        publish_split<1>(v, slice, s, 0);
    }
}

// st <- st + dt s(a0) (tanh(a1) - st), then publish.  One reciprocal per value (lem_ws_update_publish_q of lem_kernel.hip):
// e_a = 2^(c0 a0), e_b = 2^(min(c1 a1, 60)), r = dt / ((1 + e_a)(1 + e_b)), st += r ((1 - e_b) - st (1 + e_b)).
__device__ __forceinline__ void lemw_update_publish(const f32x16& a0, const f32x16& a1, float c0, float c1, float idt, f32x16& st,
                                                    char* slice) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const float ea = msmp_exp2(a0[r] * c0);
        const float eb = msmp_exp2(fminf(a1[r] * c1, 60.f));
        const float qb = eb + 1.0f;
        const float rr = msmp_rcp(__builtin_fmaf(ea, idt, idt) * qb);
        st[r] = __builtin_fmaf(rr, __builtin_fmaf(-st[r], qb, 1.0f - eb), st[r]);
    }
    lemw_publish(st, slice);
    __builtin_amdgcn_sched_barrier(0);
}

// the B fragments of step t's input MFMAs for both tiles -> bx[(X * M + m) * 64 + lane]; slot s = 16 m + 8 hh + j pairs with the A side
// of lem_slot_feature: x_hi | x_lo | x_hi of feature s % P for s < 3 P, then 1, 1 (the bias slots), then 0
template <int KT, int M>
__device__ __forceinline__ void lemw_build_inputs(const LemWideArgs& a, long n0, int t, half8* bx, int tid) {  // bx: the step's half of the area
    const int P = a.ninp;
    bool bad = false;
    for (int i = tid; i < 64 * LEMW_NT * M; i += 64 * KT) {
        const int X = i / (64 * M), m = (i >> 6) % M, l = i & 63;
        long n = n0 + 32 * X + (l & 31);
        n = n < a.n_nodes ? n : a.n_nodes - 1;
        const float* xr = a.xin + ((size_t)n * a.t_len + t) * a.stride;
        half8 v;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int s = 16 * m + 8 * (l >> 5) + j;
            const int part = (int)(s >= P) + (int)(s >= 2 * P) + (int)(s >= 3 * P);
            const int f = s - part * P;
            const float x = part < 3 ? xr[f] : 0.f;
            bad |= out_of_range(x);
            const _Float16 hi = (_Float16)x;
            const _Float16 lo = (_Float16)(x - (float)hi);
            v[j] = part == 3 ? (_Float16)(f < 2 ? 1.f : 0.f) : part == 1 ? lo : hi;
        }
        bx[((X * M) + m) * 64 + l] = v;
    }
    if (bad) status_raise(a.status, MSMP_STATUS_INPUT_RANGE);
}

template <int KT, int M>
__global__ __launch_bounds__(64 * KT) void lem_wide_kernel(LemWideArgs a) {
    constexpr int NT = LEMW_NT, FRB = KT * 4 * 1024;     // bytes per (state, tile): [k-step 2 KT][plane 2][lane 64] half8
    // one LDS object: input fragments of step t in half t & 1 | y areas of the tiles | z areas
    constexpr int XB = NT * M * 1024, YBASE = 2 * XB, ZBASE = YBASE + NT * FRB;
    __shared__ __attribute__((aligned(16))) char lds[ZBASE + NT * FRB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int T = __builtin_amdgcn_readfirstlane(tid >> 6);     // this wave's 32-channel slice
    const int c = lane & 31, hh = lane >> 5;
    const long n0 = (long)blockIdx.x * (32 * NT);
    const int W = a.width, t_len = a.t_len;
    const float LOG2E = 1.44269504088896340736f;
    const float inv_w = uniform_ro(a.scales, 4), inv_z = uniform_ro(a.scales, 5);
    const float c0 = -inv_w * LOG2E, c1z = -2.0f * inv_w * LOG2E, c1y = -2.0f * inv_z * LOG2E, idt = 1.0f / a.dt;

    // opaque per-lane offsets (see frag_global): global fragments, the y / z areas as read, this wave's slices of them as written
    unsigned lo = lane * 16, lo_y = lane * 16 + YBASE, lo_z = lane * 16 + ZBASE;
    asm volatile("" : "+v"(lo), "+v"(lo_y), "+v"(lo_z));
    const char* const rd_y = lds + lo_y;
    const char* const rd_z = lds + lo_z;
    unsigned lo_py = lane * 16 + YBASE + T * 4096, lo_pz = lane * 16 + ZBASE + T * 4096;
    asm volatile("" : "+v"(lo_py), "+v"(lo_pz));
    char* const pub_y = lds + lo_py;
    char* const pub_z = lds + lo_pz;

    // this wave's fragment streams (wave-uniform bases): gate g -> rec + ((g KT + T) 2 KT) 2 x 64
    const half8* wg[4];
    const half8* wxg[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        wg[g] = a.rec + (size_t)((g * KT + T) * 2 * KT) * 128;
        wxg[g] = a.wxh + (size_t)((g * KT + T) * 2) * 64;
    }
    LemWideRing ring;
    lemw_ring_start(ring, wg[0], wg[1], lo);

    f32x16 y[NT], z[NT];
#pragma unroll
    for (int X = 0; X < NT; ++X) {
        const long n = n0 + 32 * X + c;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int ch = 32 * T + acc_row(r, hh);
            const bool in = n < a.n_nodes && ch < W;
            y[X][r] = in && a.y0 ? a.y0[(size_t)n * W + ch] : 0.f;
            z[X][r] = in && a.z0 ? a.z0[(size_t)n * W + ch] : 0.f;
        }
        lemw_publish(y[X], pub_y + X * FRB);
        lemw_publish(z[X], pub_z + X * FRB);
    }
    lemw_build_inputs<KT, M>(a, n0, 0, reinterpret_cast<half8*>(lds), tid);
    __syncthreads();

    for (int t = 0; t < t_len; ++t) {
        const char* bx = lds + (t & 1) * XB + lane * 16;
        f32x16 acc0[NT], acc1[NT];
        // (the lane offset is made opaque again in every phase: a fragment address formed from it cannot leave the time loop as an invariant)
        unsigned lo1 = lo, lo2 = lo;
        asm volatile("" : "+v"(lo1));
        // phase 1: g2, g3 from y -> z
        lemw_gemm2<KT, M, true>(ring, wg[0], wg[1], wxg[0], wxg[1], bx, rd_y, rd_y, lo1, acc0, acc1);
        asm volatile("" : "+v"(lo2));
        lemw_ring_start(ring, wg[2], wg[3], lo2);
#pragma unroll
        for (int X = 0; X < NT; ++X) lemw_update_publish(acc0[X], acc1[X], c0, c1z, idt, z[X], pub_z + X * FRB);
        __syncthreads();
        if (t + 1 < t_len) lemw_build_inputs<KT, M>(a, n0, t + 1, reinterpret_cast<half8*>(lds + ((t + 1) & 1) * XB), tid);
        // phase 2: g1 from y, lin from the new z -> y
        lemw_gemm2<KT, M, false>(ring, wg[2], wg[3], wxg[2], wxg[3], bx, rd_y, rd_z, lo2, acc0, acc1);
        lemw_ring_start(ring, wg[0], wg[1], lo2);
        __syncthreads();                // every wave has read y(t)
#pragma unroll
        for (int X = 0; X < NT; ++X) lemw_update_publish(acc0[X], acc1[X], c0, c1y, idt, y[X], pub_y + X * FRB);
        __syncthreads();
    }

#pragma unroll
    for (int X = 0; X < NT; ++X) {
        const long n = n0 + 32 * X + c;
        if (n < a.n_nodes) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ch = 32 * T + acc_row(r, hh);
                if (ch < W) {
                    a.y_out[(size_t)n * W + ch] = y[X][r];
                    if (a.z_out) a.z_out[(size_t)n * W + ch] = z[X][r];
                }
            }
        }
    }
}

}  // namespace msmp

using namespace msmp;

static bool lem_wide_shape_ok(const char* who, int ninp, int width) {
    if (!wide_width_ok(who, width)) return false;
    if (ninp < 1 || ninp > LEM_MAX_INP) {
        set_error("%s: ninp=%d outside 1..%d", who, ninp, LEM_MAX_INP);
        return false;
    }
    return true;
}

extern "C" int64_t msmp_packed_lem_wide_floats(int ninp, int width) {
    if (!lem_wide_shape_ok("msmp_packed_lem_wide_floats", ninp, width)) return 0;
    return lem_wide_layout((width + 31) / 32).total;
}

extern "C" int msmp_pack_lem_wide_f32(const float* weights, const float* weights_lin_z, const float* bias, const float* bias_lin_z,
                                      int ninp, int width, float* packed_out, msmp_stream_t stream) {
    if (!lem_wide_shape_ok("msmp_pack_lem_wide_f32", ninp, width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(weights && weights_lin_z && bias && bias_lin_z && packed_out, MSMP_ERR_ARG, "msmp_pack_lem_wide_f32: null pointer");
    LemWidePackArgs a{weights, weights_lin_z, bias, bias_lin_z, ninp, width, (width + 31) / 32, packed_out};
    hipLaunchKernelGGL(pack_lem_wide_scale_kernel, dim3(2), dim3(256), 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(pack_lem_wide_kernel, dim3(256), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("pack_lem_wide_kernel");
}

extern "C" int msmp_lem_encoder_wide_f32(const float* xin, int64_t n_nodes, int t_len, int ninp, int width, float dt, const float* packed,
                                         const float* y0, const float* z0, float* y_out, float* z_out, msmp_stream_t stream) {
    if (!lem_wide_shape_ok("msmp_lem_encoder_wide_f32", ninp, width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(t_len >= 1, MSMP_ERR_ARG, "msmp_lem_encoder_wide_f32: t_len=%d < 1", t_len);
    MSMP_REQUIRE(n_nodes >= 0 && n_nodes < (1L << 31), MSMP_ERR_ARG, "msmp_lem_encoder_wide_f32: bad n_nodes");
    MSMP_REQUIRE(xin && packed && y_out, MSMP_ERR_ARG, "msmp_lem_encoder_wide_f32: null pointer");
    MSMP_REQUIRE((y0 == nullptr) == (z0 == nullptr), MSMP_ERR_ARG, "msmp_lem_encoder_wide_f32: give both initial states or none");
    if (n_nodes == 0) return MSMP_OK;
    const int kt = (width + 31) / 32;
    const LemWideLayout L = lem_wide_layout(kt);
    LemWideArgs a{xin, (long)n_nodes, t_len, ninp, msmp_lem_input_stride(ninp), width, dt, packed + L.scales,
                  reinterpret_cast<const half8*>(packed + L.rec), reinterpret_cast<const half8*>(packed + L.wxh), y0, z0, y_out, z_out,
                  status_ptr()};
    const unsigned grid = (unsigned)((n_nodes + 32 * LEMW_NT - 1) / (32 * LEMW_NT));
    hipStream_t st = (hipStream_t)stream;
    timing_begin(MSMP_K_LEM, st);
    dispatch_kt(kt, [&](auto K) {
        constexpr int KT = decltype(K)::value;
        if ((3 * ninp + 2 + 15) / 16 == 1) hipLaunchKernelGGL((lem_wide_kernel<KT, 1>), dim3(grid), dim3(64 * KT), 0, st, a);
        else hipLaunchKernelGGL((lem_wide_kernel<KT, 2>), dim3(grid), dim3(64 * KT), 0, st, a);
    });
    timing_end(MSMP_K_LEM, st);
    return check_launch("lem_wide_kernel");
}
