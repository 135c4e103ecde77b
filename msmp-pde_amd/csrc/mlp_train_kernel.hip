// The Swish MLPs around the encoder and decoder for TRAINING (embedding_mlp, lemoutput_mlp, lstmoutput_mlp, double_mlp of the solver classes:
// experiments/models_gnn.py nn.Sequential(nn.Linear, Swish(), nn.Linear, Swish()) and nn.Sequential(nn.Linear(W, 2 W), Swish(), nn.Unflatten)):
// forward with the pre-activations saved, and the backward down to dx and the parameter gradients, as one kernel launch each.
//   two-layer form            out = Swish(W2 Swish(W1 x + b1) + b2)             W1 [W, K], W2 [W, W]
//   one-layer form, `heads`   out[:, h W : (h + 1) W] = Swish(W1[h W : (h + 1) W] x + b1[h W : (h + 1) W])       W1 [heads W, K], heads 1 | 2
// at 1 <= K <= 256 input features and hidden width 1 <= W <= 256, parameters in nn.Linear's layout (weight [out, in], bias [out]), rows
// row-major fp32 with explicit row strides of which only the first K (W, heads W) floats are read or written.
//   msmp_mlp_train_fwd_f32   out and saved = the pre-activations z1 (, z2)
//   msmp_mlp_train_bwd_f32   dz2 = g dswish(z2);  da1 = W2^T dz2;  dz1 = da1 dswish(z1);  dx = W1^T dz1 (optional: summed over the heads in head order);
//                            then dW2, db2 = (dz2, a1 = Swish(z1)) and dW1, db1 = (dz1, x) as msmp_grad_weights_f32 jobs of 128 columns of dz each
//
// The scheme is recurrent_train.h's with T = 1 (its pieces are in train_frags.h): one 32-row tile per workgroup, KT = ceil(W / 32) waves,
// wave ct owns channel tile ct in accumulator layout (one row per lane); the B operand of a GEMM (x, a1; dz2, dz1) is PUBLISHED in LDS as bf16
// hi / mid / lo fragments in acc order in ONE area of 6 KT KB reused between barriers, and every wave multiplies its own 32 rows of the weight
// block -- bf16x3 A fragments streamed from the L2-resident blob through buffer loads, one k-tile ahead -- with the published fragments: six
// v_mfma_f32_32x32x16_bf16 per K = 16 step, fp32-exact products.  No fp16 anywhere: no input range, the range status is neither read nor
// raised.  What T = 1 and K != W add:
//   * x has KK = ceil(K / 32) k-tiles, the area KT: x is published in chunks of KT k-tiles (wave ct publishes k-tile c0 + ct), one chunk
//     between two barriers, so K <= Wp (every solver class) is one chunk;
//   * dx has KK channel tiles, the workgroup KT waves: wave ct accumulates tiles ct, ct + KT, ... (at most ceil(8 / KT)) in registers,
//     over the heads in head order.
// Barriers per launch (K <= Wp): forward 2 per one-layer head, 3 two-layer; backward 2 per one-layer head with dx (0 without), 2 two-layer
// without dx, 4 with.
// Channels W .. Wp - 1 carry zero weights and zero bias: their z is an exact 0 (saved as such), so are a1, dz2, da1 and dz1; they are never
// written to out.  A row's arithmetic depends on nothing but that row.
//
// Memory layouts (all fp32):
//   saved  [layers heads][N][Wp]    two-layer: z1, z2; one-layer: z of head h; every element is written
//   dz1    [N][ldz1]                ldz1 = 128 ceil(heads W / 128): head h at columns h W ..; columns heads W .. ldz1 - 1 are written as 0
//   dz2, a1 [N][ldz]                ldz = 128 ceil(W / 128), likewise (two-layer form only)
// which is what a weight-gradient job reads: A = 128 columns of dz (row stride ldz), B = a1 or x.
#include "grad_weights.h"
#include "train_frags.h"

namespace msmp {

// the blob (floats), kt = ceil(W / 32), kk = ceil(K / 32), k-tile = [s 2][plane 3: hi, mid, lo][lane 64][8 bf16] in acc order (split_k_acc):
//   w1f  [head][ct kt][kc kk]   rows h W + 32 ct .. of W1, columns 32 kc ..                                   forward, layer 1 |
//   w2f  [ct kt][kc kt]         rows 32 ct .. of W2, columns 32 kc ..                 (two-layer form)        forward, layer 2 |
//   w2t  [ct kt][kc kt]         fragment row 32 ct + m, column 32 kc + k = W2[32 kc + k][32 ct + m]            da1 = W2^T dz2 |
//   w1t  [head][ot kk][kc kt]   fragment row 32 ot + m, column 32 kc + k = W1[h W + 32 kc + k][32 ot + m]      dx = W1^T dz1 |
//   bias [layers heads][Wp]
// zero outside the matrices.  A wave's stream of one GEMM is contiguous.
struct MlpTrainLayout {
    int kt, kk;
    int64_t w1f, w2f, w2t, w1t, bias, total;
};
__host__ __device__ inline MlpTrainLayout mlp_train_layout(int layers, int heads, int k_in, int width) {
    MlpTrainLayout L;
    L.kt = (width + 31) / 32;
    L.kk = (k_in + 31) / 32;
    const int64_t t1 = (int64_t)heads * L.kt * L.kk * LWT_KTILE_FLOATS, t2 = layers == 2 ? (int64_t)L.kt * L.kt * LWT_KTILE_FLOATS : 0;
    L.w1f = 0;
    L.w2f = L.w1f + t1;
    L.w2t = L.w2f + t2;
    L.w1t = L.w2t + t2;
    L.bias = L.w1t + t1;
    L.total = L.bias + (int64_t)layers * heads * 32 * L.kt;
    return L;
}

// one fragment section of the blob: tiles_r x tiles_k k-tiles of rows row0 .. row0 + n_out - 1 of w [., n_in] (transposed: of their transpose)
struct MlpPackSeg {
    const float* w;
    int n_in, n_out, row0, tiles_r, tiles_k, transposed;
    int64_t dst, first;         // offset in the blob (floats); first thread index of the section
};
constexpr int MT_MAX_SEGS = 4;
struct MlpTrainPackArgs {
    MlpPackSeg seg[MT_MAX_SEGS];
    int n_seg, n_bias, width, wp;
    int64_t n_frag, bias_dst;
    const float* bias[2];       // per bias row of Wp: its first element
    float* out;
};

// one thread per (section, row tile, k-tile, s, lane)
__global__ __launch_bounds__(256) void pack_mlp_train_kernel(MlpTrainPackArgs a) {
    const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p0 = tid0; p0 < a.n_frag; p0 += stride) {
        int si = 0;
#pragma unroll
        for (int i = 1; i < MT_MAX_SEGS; ++i)
            if (i < a.n_seg && p0 >= a.seg[i].first) si = i;
        const MlpPackSeg& sg = a.seg[si];
        const int64_t p = p0 - sg.first;
        const int lane = (int)(p & 63), s = (int)(p >> 6) & 1;
        const int64_t q = p >> 7;
        const int kc = (int)(q % sg.tiles_k), rt = (int)(q / sg.tiles_k);
        const int row = 32 * rt + (lane & 31);
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int k = 32 * kc + split_k_acc(s, lane >> 5, j);
            // fragment (row, k) is w[row0 + row][k], transposed w[row0 + k][row]: ONE load from a selected element (see pack_recurrent_train_kernel)
            const int o = sg.transposed ? k : row, i = sg.transposed ? row : k;
            const bool in = o < sg.n_out && i < sg.n_in;
            const float w = sg.w[in ? (size_t)(sg.row0 + o) * sg.n_in + i : 0];
            v[j] = in ? w : 0.f;
        }
        lwt_store_b3(a.out + sg.dst, p >> 6, lane, v);
    }
    for (int64_t p = tid0; p < (int64_t)a.n_bias * a.wp; p += stride) {
        const int ch = (int)(p % a.wp), r = (int)(p / a.wp);
        const float* b = a.bias[r];
        const float v = b[ch < a.width ? ch : 0];
        a.out[a.bias_dst + p] = ch < a.width ? v : 0.f;
    }
}

__device__ __forceinline__ __amdgpu_buffer_rsrc_t mt_stream(const float* first_tile, int n_tiles) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(first_tile), 0, n_tiles * LWT_KTILE_FLOATS * 4, 0x00027000);
}
// acc += stream[k-tiles i0 .. i0 + nk - 1] * published[k-tiles 0 .. nk - 1].  `w` holds k-tile i0 on entry (requested before the barrier in
// front of the GEMM) and k-tile i0 + nk on return where the stream has one: the next k-tile is requested before each one's MFMAs.
__device__ __forceinline__ void mt_gemm(LwtFrag& w, __amdgpu_buffer_rsrc_t stream, int i0, int nk, int n_tiles, const u32x4* xf, int lane, unsigned loff,
                                        f32x16& acc) {
    for (int kc = 0; kc < nk; ++kc) {
        LwtFrag nxt;
        const int i = i0 + kc + 1;
        lwt_frag_load(nxt, stream, i < n_tiles ? i : i - 1, loff);
        lwt_mma(w, xf, kc, lane, acc);
        __builtin_amdgcn_sched_barrier(0);       // one k-tile of weight fragments ahead, not all of them
        w = nxt;
    }
}

struct MlpTrainArgs {
    const float* x;         // [N, ldx], K used
    long n_rows;
    int ldx, k_in, width, heads, kk;
    const float *w1f, *w2f, *bias;
    float* saved;           // [layers heads][N][Wp]
    float* out;             // [N, ld_out], heads W used
    int ld_out;
};

template <int KT, int LAYERS>
__global__ __launch_bounds__(64 * KT) void mlp_train_fwd_kernel(MlpTrainArgs a) {
    constexpr int WP = 32 * KT;
    __shared__ u32x4 xf[KT * LWT_KTILE_U4];                          // 6 KT KB: a chunk of x, then a1
    const int tid = threadIdx.x, lane = tid & 63;
    const int ct = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5, W = a.width, K = a.k_in, kk = a.kk;
    const int heads = LAYERS == 2 ? 1 : a.heads;
    const size_t plane = (size_t)a.n_rows * WP;
    const long n = (long)blockIdx.x * 32 + c;
    const bool live = n < a.n_rows;
    const long nc = live ? n : a.n_rows - 1;
    const float* xrow = a.x + (size_t)nc * a.ldx;
    float* srow = a.saved + (size_t)nc * WP + 4 * hh;
    unsigned loff = 16u * lane;
    asm volatile("" : "+v"(loff));

    for (int h = 0; h < heads; ++h) {
        f32x16 acc;
        lwt_tile_load(a.bias + h * WP + 4 * hh, ct, acc);
        const __amdgpu_buffer_rsrc_t s1 = mt_stream(a.w1f + (size_t)(h * KT + ct) * kk * LWT_KTILE_FLOATS, kk);
        LwtFrag w;
        lwt_frag_load(w, s1, 0, loff);
        for (int c0 = 0; c0 < kk; c0 += KT) {                        // the area is free: every GEMM below ends with a barrier
            if (c0 + ct < kk) {
                f32x16 v;
                lwt_dense_load(xrow, c0 + ct, hh, K, v);
                lwt_publish(xf, ct, lane, v);
            }
            __syncthreads();
            mt_gemm(w, s1, c0, min(KT, kk - c0), kk, xf, lane, loff, acc);
            __syncthreads();
        }
        if (live) lwt_tile_store(srow + (size_t)h * plane, ct, acc);             // z1 (one-layer: z of head h)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = swishf(acc[r]);
        if constexpr (LAYERS == 2) {
            lwt_publish(xf, ct, lane, acc);
            const __amdgpu_buffer_rsrc_t s2 = mt_stream(a.w2f + (size_t)ct * KT * LWT_KTILE_FLOATS, KT);
            lwt_frag_load(w, s2, 0, loff);
            lwt_tile_load(a.bias + WP + 4 * hh, ct, acc);
            __syncthreads();
            mt_gemm(w, s2, 0, KT, KT, xf, lane, loff, acc);
            if (live) lwt_tile_store(srow + plane, ct, acc);                     // z2
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[r] = swishf(acc[r]);
        }
        if (live) lwt_dense_store(a.out + (size_t)n * a.ld_out + h * W, ct, hh, W, acc);
    }
}

struct MlpTrainBwdArgs {
    const float* gout;      // [N, ld_g], heads W used
    const float* saved;
    long n_rows;
    int ld_g, k_in, width, heads, kk, ldz;
    const float *w2t, *w1t;
    float *dz2, *a1, *dz1;  // [N, ldz]; dz2 and a1 in the two-layer form only
    float* dx;              // [N, ld_dx], K used; NULL: not computed
    int ld_dx;
};

template <int KT, int LAYERS>
__global__ __launch_bounds__(64 * KT) void mlp_train_bwd_kernel(MlpTrainBwdArgs a) {
    constexpr int WP = 32 * KT, NT = (8 + KT - 1) / KT;              // dx tiles of a wave
    __shared__ u32x4 xf[KT * LWT_KTILE_U4];                          // 6 KT KB: dz2, then dz1
    const int tid = threadIdx.x, lane = tid & 63;
    const int ct = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 31, hh = lane >> 5, W = a.width, K = a.k_in, kk = a.kk, ldz = a.ldz;
    const int heads = LAYERS == 2 ? 1 : a.heads;
    const size_t plane = (size_t)a.n_rows * WP;
    const long n = (long)blockIdx.x * 32 + c;
    const bool live = n < a.n_rows;
    const long nc = live ? n : a.n_rows - 1;
    const float* srow = a.saved + (size_t)nc * WP + 4 * hh;
    float* zrow = a.dz1 + (size_t)nc * ldz;
    unsigned loff = 16u * lane;
    asm volatile("" : "+v"(loff));
    f32x16 dxa[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r) dxa[j][r] = 0.f;

    for (int h = 0; h < heads; ++h) {
        f32x16 d, z;
        lwt_dense_load(a.gout + (size_t)nc * a.ld_g + h * W, ct, hh, W, d);
        lwt_tile_load(srow + (size_t)(LAYERS == 2 ? 1 : h) * plane, ct, z);
#pragma unroll
        for (int r = 0; r < 16; ++r) d[r] *= dswish(z[r]);
        if constexpr (LAYERS == 2) {
            if (live) lwt_dense_store(a.dz2 + (size_t)nc * ldz, ct, hh, W, d);
            lwt_publish(xf, ct, lane, d);
            const __amdgpu_buffer_rsrc_t s2 = mt_stream(a.w2t + (size_t)ct * KT * LWT_KTILE_FLOATS, KT);
            LwtFrag w;
            lwt_frag_load(w, s2, 0, loff);
            f32x16 da;
#pragma unroll
            for (int r = 0; r < 16; ++r) da[r] = 0.f;
            __syncthreads();
            mt_gemm(w, s2, 0, KT, KT, xf, lane, loff, da);                       // da1 = W2^T dz2
            __syncthreads();                                                     // every wave has read the last fragment of dz2
            lwt_tile_load(srow, ct, z);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                d[r] = da[r] * dswish(z[r]);
                z[r] = swishf(z[r]);
            }
            if (live) lwt_dense_store(a.a1 + (size_t)nc * ldz, ct, hh, W, z);
        }
        if (live) lwt_dense_store(zrow + h * W, ct, hh, W, d);
        if (a.dx) {
            lwt_publish(xf, ct, lane, d);                                        // the area is free: first use, or behind a barrier
            __syncthreads();
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int ot = ct + j * KT;
                if (ot < kk) {
                    const __amdgpu_buffer_rsrc_t s1 = mt_stream(a.w1t + (size_t)(h * kk + ot) * KT * LWT_KTILE_FLOATS, KT);
                    LwtFrag w;
                    lwt_frag_load(w, s1, 0, loff);
                    mt_gemm(w, s1, 0, KT, KT, xf, lane, loff, dxa[j]);           // dx += W1[head h]^T dz1
                }
            }
            __syncthreads();
        }
    }
    if (!live) return;
    // columns heads W .. ldz - 1: zeros (the weight-gradient jobs read whole 128-column blocks)
    for (int col = heads * W + 2 * ct + hh; col < ldz; col += 2 * KT) {
        zrow[col] = 0.f;
        if constexpr (LAYERS == 2) {
            a.dz2[(size_t)nc * ldz + col] = 0.f;
            a.a1[(size_t)nc * ldz + col] = 0.f;
        }
    }
    if (a.dx) {
#pragma unroll
        for (int j = 0; j < NT; ++j)
            if (ct + j * KT < kk) lwt_dense_store(a.dx + (size_t)n * a.ld_dx, ct + j * KT, hh, K, dxa[j]);
    }
}

// the first rows of a part-filled last 128-row group of a weight gradient, from the job's full block to the parameter's gradient
struct MlpRaggedArgs {
    const float* src[4];
    float* dst[4];
    int count[4], n;
};
__global__ __launch_bounds__(256) void mlp_train_ragged_kernel(MlpRaggedArgs a) {
    const int i = blockIdx.y;
    if (i >= a.n) return;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < a.count[i]; p += gridDim.x * blockDim.x) a.dst[i][p] = a.src[i][p];
}

struct MlpBwdPlan {
    int ldz1, ldz, g1, g2;              // row strides and 128-column groups of dz1 / dz2
    size_t dz1, dz2, a1, rag_w[2], rag_b[2], gw, bytes;
    int64_t gw_floats;
    int n_jobs;
};
static bool mlp_bwd_plan(int64_t n, int layers, int heads, int k_in, int width, MlpBwdPlan& p) {
    size_t off = 0;
    auto take = [&](size_t floats) { const size_t r = off; off += (floats * sizeof(float) + 255) & ~(size_t)255; return r; };
    p.g1 = (heads * width + 127) / 128; p.ldz1 = 128 * p.g1;
    p.g2 = layers == 2 ? (width + 127) / 128 : 0; p.ldz = 128 * p.g2;
    p.dz1 = take((size_t)n * p.ldz1);
    p.dz2 = take((size_t)n * p.ldz);
    p.a1 = take((size_t)n * p.ldz);
    p.rag_w[0] = take((size_t)128 * k_in); p.rag_b[0] = take(128);
    p.rag_w[1] = take((size_t)128 * width); p.rag_b[1] = take(128);
    int64_t rows[GW_MAX_JOBS];
    int k2[GW_MAX_JOBS];
    p.n_jobs = 0;
    for (int g = 0; g < p.g2; ++g, ++p.n_jobs) { rows[p.n_jobs] = n; k2[p.n_jobs] = width; }
    for (int g = 0; g < p.g1; ++g, ++p.n_jobs) { rows[p.n_jobs] = n; k2[p.n_jobs] = k_in; }
    p.gw_floats = msmp_grad_weights_workspace_floats(p.n_jobs, rows, k2);
    if (p.gw_floats < 0) return false;
    p.gw = take((size_t)p.gw_floats);
    p.bytes = off + 256;                // the base is aligned up to 256 bytes
    return true;
}

}  // namespace msmp

using namespace msmp;

static bool mlp_train_shape_ok(const char* who, int layers, int heads, int k_in, int width) {
    if (!wide_width_ok(who, width)) return false;
    if (k_in < 1 || k_in > WIDE_MAX_W) {
        set_error("%s: k_in=%d outside 1..%d", who, k_in, WIDE_MAX_W);
        return false;
    }
    if (layers < 1 || layers > 2 || heads < 1 || heads > 2 || (layers == 2 && heads != 1)) {
        set_error("%s: layers=%d heads=%d: one layer of 1 or 2 heads, or two layers of one", who, layers, heads);
        return false;
    }
    return true;
}
static bool mlp_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static bool mlp_rows_ok(int64_t n_rows) { return n_rows >= 1 && n_rows < (1L << 31); }

extern "C" int64_t msmp_packed_mlp_train_floats(int layers, int heads, int k_in, int width) {
    if (!mlp_train_shape_ok("msmp_packed_mlp_train_floats", layers, heads, k_in, width)) return 0;
    return mlp_train_layout(layers, heads, k_in, width).total;
}

extern "C" int64_t msmp_mlp_train_saved_floats(int64_t n_rows, int layers, int heads, int width) {
    if (!mlp_train_shape_ok("msmp_mlp_train_saved_floats", layers, heads, 1, width)) return 0;
    if (!mlp_rows_ok(n_rows)) {
        set_error("msmp_mlp_train_saved_floats: bad n_rows");
        return 0;
    }
    return (int64_t)layers * heads * n_rows * (32 * ((width + 31) / 32));
}

extern "C" size_t msmp_mlp_train_bwd_workspace_bytes(int64_t n_rows, int layers, int heads, int k_in, int width) {
    if (!mlp_train_shape_ok("msmp_mlp_train_bwd_workspace_bytes", layers, heads, k_in, width)) return 0;
    MlpBwdPlan p;
    if (!mlp_rows_ok(n_rows) || !mlp_bwd_plan(n_rows, layers, heads, k_in, width, p)) {
        set_error("msmp_mlp_train_bwd_workspace_bytes: bad n_rows");
        return 0;
    }
    return p.bytes;
}

extern "C" int msmp_pack_mlp_train_f32(const float* w1, const float* b1, const float* w2, const float* b2, int layers, int heads, int k_in, int width,
                                       float* packed_out, msmp_stream_t stream) {
    const char* who = "msmp_pack_mlp_train_f32";
    if (!mlp_train_shape_ok(who, layers, heads, k_in, width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(w1 && b1 && packed_out && (layers == 1 || (w2 && b2)), MSMP_ERR_ARG, "%s: null pointer", who);
    MSMP_REQUIRE(mlp_aligned16(packed_out), MSMP_ERR_ARG, "%s: packed_out is not 16-byte aligned", who);
    const MlpTrainLayout L = mlp_train_layout(layers, heads, k_in, width);
    MlpTrainPackArgs a;
    a.n_seg = 0;
    a.n_frag = 0;
    auto add = [&](const float* w, int n_in, int row0, int tr, int tk, int transposed, int64_t dst) {
        a.seg[a.n_seg++] = MlpPackSeg{w, n_in, width, row0, tr, tk, transposed, dst, a.n_frag};
        a.n_frag += (int64_t)tr * tk * 128;
    };
    const int64_t t1 = (int64_t)L.kt * L.kk * LWT_KTILE_FLOATS;
    for (int h = 0; h < heads; ++h) add(w1, k_in, h * width, L.kt, L.kk, 0, L.w1f + h * t1);
    if (layers == 2) {
        add(w2, width, 0, L.kt, L.kt, 0, L.w2f);
        add(w2, width, 0, L.kt, L.kt, 1, L.w2t);
    }
    for (int h = 0; h < heads; ++h) add(w1, k_in, h * width, L.kk, L.kt, 1, L.w1t + h * t1);
    for (int i = a.n_seg; i < MT_MAX_SEGS; ++i) a.seg[i] = a.seg[0];
    a.n_bias = layers * heads; a.width = width; a.wp = 32 * L.kt; a.bias_dst = L.bias;
    a.bias[0] = b1;
    a.bias[1] = layers == 2 ? b2 : b1 + width;
    a.out = packed_out;
    hipLaunchKernelGGL(pack_mlp_train_kernel, dim3(grid_for(a.n_frag)), dim3(256), 0, (hipStream_t)stream, a);
    return check_launch("pack_mlp_train_kernel");
}

extern "C" int msmp_mlp_train_fwd_f32(const float* x, int ldx, int64_t n_rows, int layers, int heads, int k_in, int width, const float* packed,
                                      float* saved, float* out, int ld_out, msmp_stream_t stream) {
    const char* who = "msmp_mlp_train_fwd_f32";
    if (!mlp_train_shape_ok(who, layers, heads, k_in, width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(x && packed && saved && out, MSMP_ERR_ARG, "%s: null pointer", who);
    MSMP_REQUIRE(mlp_rows_ok(n_rows), MSMP_ERR_ARG, "%s: bad n_rows", who);
    MSMP_REQUIRE(ldx >= k_in && ld_out >= heads * width, MSMP_ERR_ARG, "%s: ldx=%d < k_in or ld_out=%d < heads * width", who, ldx, ld_out);
    MSMP_REQUIRE(mlp_aligned16(packed) && mlp_aligned16(saved), MSMP_ERR_ARG, "%s: packed / saved not 16-byte aligned", who);
    const MlpTrainLayout L = mlp_train_layout(layers, heads, k_in, width);
    MlpTrainArgs a{x, (long)n_rows, ldx, k_in, width, heads, L.kk, packed + L.w1f, packed + L.w2f, packed + L.bias, saved, out, ld_out};
    const unsigned grid = (unsigned)((n_rows + 31) / 32);
    hipStream_t st = (hipStream_t)stream;
    dispatch_kt(L.kt, [&](auto Kc) {
        constexpr int KT = decltype(Kc)::value;
        if (layers == 2) hipLaunchKernelGGL((mlp_train_fwd_kernel<KT, 2>), dim3(grid), dim3(64 * KT), 0, st, a);
        else hipLaunchKernelGGL((mlp_train_fwd_kernel<KT, 1>), dim3(grid), dim3(64 * KT), 0, st, a);
    });
    return check_launch("mlp_train_fwd_kernel");
}

extern "C" int msmp_mlp_train_bwd_f32(const float* grad_out, int ld_grad, const float* x, int ldx, const float* saved, int64_t n_rows, int layers,
                                      int heads, int k_in, int width, const float* packed, float* dx, int ld_dx, float* dw1, float* db1, float* dw2,
                                      float* db2, void* workspace, size_t workspace_bytes, msmp_stream_t stream) {
    const char* who = "msmp_mlp_train_bwd_f32";
    if (!mlp_train_shape_ok(who, layers, heads, k_in, width)) return MSMP_ERR_UNSUPPORTED;
    MSMP_REQUIRE(grad_out && x && saved && packed && dw1 && db1 && workspace && (layers == 1 || (dw2 && db2)), MSMP_ERR_ARG, "%s: null pointer", who);
    MSMP_REQUIRE(mlp_rows_ok(n_rows), MSMP_ERR_ARG, "%s: bad n_rows", who);
    MSMP_REQUIRE(ldx >= k_in && ld_grad >= heads * width && (!dx || ld_dx >= k_in), MSMP_ERR_ARG, "%s: a row stride is shorter than its row", who);
    MSMP_REQUIRE(mlp_aligned16(packed) && mlp_aligned16(saved), MSMP_ERR_ARG, "%s: packed / saved not 16-byte aligned", who);
    MlpBwdPlan p;
    MSMP_REQUIRE(mlp_bwd_plan(n_rows, layers, heads, k_in, width, p), MSMP_ERR_UNSUPPORTED, "%s: sizes outside the weight-gradient kernel", who);
    MSMP_REQUIRE(workspace_bytes >= p.bytes, MSMP_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, p.bytes);
    char* base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    auto at = [&](size_t off) { return reinterpret_cast<float*>(base + off); };
    const MlpTrainLayout L = mlp_train_layout(layers, heads, k_in, width);
    MlpTrainBwdArgs a{grad_out, saved, (long)n_rows, ld_grad, k_in, width, heads, L.kk, p.ldz1, packed + L.w2t, packed + L.w1t,
                      at(p.dz2), at(p.a1), at(p.dz1), dx, ld_dx};
    const unsigned grid = (unsigned)((n_rows + 31) / 32);
    hipStream_t st = (hipStream_t)stream;
    dispatch_kt(L.kt, [&](auto Kc) {
        constexpr int KT = decltype(Kc)::value;
        if (layers == 2) hipLaunchKernelGGL((mlp_train_bwd_kernel<KT, 2>), dim3(grid), dim3(64 * KT), 0, st, a);
        else hipLaunchKernelGGL((mlp_train_bwd_kernel<KT, 1>), dim3(grid), dim3(64 * KT), 0, st, a);
    });
    const int rc = check_launch("mlp_train_bwd_kernel");
    if (rc) return rc;

    // dW2, db2 = (dz2, a1); dW1, db1 = (dz1, x): one job per 128 columns of dz.  A job writes 128 rows of a gradient: the part-filled last
    // group of a layer goes to a block of the workspace, of which mlp_train_ragged_kernel copies the rows that exist.
    const float *ja[GW_MAX_JOBS], *jb[GW_MAX_JOBS];
    float *jw[GW_MAX_JOBS], *jbias[GW_MAX_JOBS];
    int64_t rows[GW_MAX_JOBS];
    int lda[GW_MAX_JOBS], ldb[GW_MAX_JOBS], k2[GW_MAX_JOBS], j = 0;
    MlpRaggedArgs rg;
    rg.n = 0;
    auto layer_jobs = [&](int which, const float* dz, int ldz, int groups, int n_out, const float* b, int ld_b, int k, float* dw, float* db) {
        for (int g = 0; g < groups; ++g, ++j) {
            const bool ragged = 128 * (g + 1) > n_out;
            ja[j] = dz + 128 * g; jb[j] = b; rows[j] = n_rows; lda[j] = ldz; ldb[j] = ld_b; k2[j] = k;
            jw[j] = ragged ? at(p.rag_w[which]) : dw + (size_t)128 * g * k;
            jbias[j] = ragged ? at(p.rag_b[which]) : db + 128 * g;
            if (ragged) {
                const int left = n_out - 128 * g;
                rg.src[rg.n] = jw[j]; rg.dst[rg.n] = dw + (size_t)128 * g * k; rg.count[rg.n++] = left * k;
                rg.src[rg.n] = jbias[j]; rg.dst[rg.n] = db + 128 * g; rg.count[rg.n++] = left;
            }
        }
    };
    if (layers == 2) layer_jobs(1, at(p.dz2), p.ldz, p.g2, width, at(p.a1), p.ldz, width, dw2, db2);
    layer_jobs(0, at(p.dz1), p.ldz1, p.g1, heads * width, x, ldx, k_in, dw1, db1);
    const int rc2 = launch_grad_weights(j, ja, jb, rows, lda, ldb, k2, jw, jbias, at(p.gw), p.gw_floats, st);
    if (rc2) return rc2;
    if (rg.n) {
        for (int i = rg.n; i < 4; ++i) { rg.src[i] = rg.src[0]; rg.dst[i] = rg.dst[0]; rg.count[i] = 0; }
        hipLaunchKernelGGL(mlp_train_ragged_kernel, dim3(32, (unsigned)rg.n), dim3(256), 0, st, rg);
        return check_launch("mlp_train_ragged_kernel");
    }
    return MSMP_OK;
}
