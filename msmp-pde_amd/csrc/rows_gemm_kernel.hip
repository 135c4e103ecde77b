// The fp32-exact bf16x3 row GEMM (interface: rows_gemm.h).  Callers: both layer backwards (layer_bwd_kernel.hip, wide_layer_bwd_kernel.hip)
// and, through the msmp_linear_f32 / msmp_linear_swish_f32 entries at the end of this file, the inference forward of the GLU classes and
// of the 2-D classes' double_mlp.
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
#include "rows_gemm.h"

namespace msmp {

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

void add_pack(RgPackArgs& a, int& blocks, const float* w, int ldw, int K, int col0, int transposed, u32x4* out) {
    RgPackJob& j = a.job[a.n_jobs++];
    j.w = w; j.out = out; j.ldw = ldw; j.K = K; j.n_chunks = (K + 31) / 32; j.col0 = col0; j.transposed = transposed; j.first_block = blocks;
    j.n_rows = 0x7fffffff;
    blocks += (j.n_chunks * 512 + 255) / 256;
}
int launch_rg_pack(RgPackArgs& a, int blocks, hipStream_t st) {
    for (int i = a.n_jobs; i < RG_MAX_PACK; ++i) a.job[i] = a.job[0];
    hipLaunchKernelGGL(rg_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    return check_launch("rg_pack_kernel");
}

}  // namespace msmp

using namespace msmp;

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
    RC(launch_rg_pack(pa, blocks, st));
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
    RC(launch_rg_pack(pa, blocks, st));
    hipLaunchKernelGGL(linear_pad_bias_kernel, dim3((unsigned)((128 * groups + 255) / 256)), dim3(256), 0, st, mode == 2 ? nullptr : bias, n_out, 128 * groups, bpad);
    RC(check_launch("linear_pad_bias_kernel"));
    const int epi = mode == 0 ? 1 : (mode == 1 ? 4 : 5);
    for (int g = 0; g < groups; ++g)
        RC(rows_gemm(epi, x, ldx, (long)rows, k, fp + (size_t)g * chunks * RG_CHUNK_U4, bpad + 128 * g, nullptr, out + 128 * g, ld_out, nullptr, st));
    return MSMP_OK;
}
