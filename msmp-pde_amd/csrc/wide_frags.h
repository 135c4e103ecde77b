// The fragment toolkit of the width-generic kernels (lem_wide_kernel.hip, wide_message_kernel.hip, wide_node_tail_kernel.hip).  They share
// one scheme: a wave per 32-channel slice (KT = Wp / 32 waves, Wp = 32 ceil(W / 32) <= 256), operands as fp16 hi / lo fragments laid
// out [k-step][plane 2: hi, lo][column block NB][lane 64] half8 (1 KB per fragment, lane-linear: one conflict-free 16-byte access per
// lane), three v_mfma_f32_32x32x16_f16 per K = 16 step into one fp32 accumulator (mfma_tiles.h), weights pre-multiplied at pack time by
// a power of two 2^s with max |.| 2^s in [16, 32).  What differs between the kernels (tile maps, phases, which operand streams and
// which stays) is in their own files.
#pragma once
#include <type_traits>

#include "mfma_tiles.h"

namespace msmp {

constexpr int WIDE_MAX_W = 256;

// ---- pack time: the scale and the A fragments ---------------------------------------------------------------------------------

// max |p[0 .. n - 1]| over this block's 256 threads, this thread's part
__device__ __forceinline__ float abs_max_part(const float* p, int n) {
    float m = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) m = fmaxf(m, fabsf(p[i]));
    return m;
}

// the shift s with mx 2^s in [16, 32), mx the maximum of `m` over the block's 256 threads (0 for mx = 0); valid in every thread
__device__ __forceinline__ int block_scale_shift(float m) {
    __shared__ float red[256];
    red[threadIdx.x] = m;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + off]);
        __syncthreads();
    }
    const float mx = red[0];
    int e = 0;
    if (mx > 0.f && mx < 3.0e38f) (void)frexpf(mx, &e);
    return mx > 0.f ? 5 - e : 0;
}

// scale group i of a blob's scales[8]: 2^s at [i], 2^-(s + extra) at [4 + i] (extra: a power of two that the kernel's other operand
// carries), zeros in the unused slots [2 + i] and [6 + i]
__device__ __forceinline__ void store_scale_group(float* scales, int i, int sft, int extra) {
    scales[i] = ldexpf(1.0f, sft);
    scales[4 + i] = ldexpf(1.0f, -sft - extra);
    scales[2 + i] = 0.f;
    scales[6 + i] = 0.f;
}

// n_frags A fragments as [fragment][plane 2: hi, lo][lane 64][8 halfs] (grid-stride): value(fragment, lane, j) is the SCALED weight of
// that element, 0 outside the matrix; lane (c, hh) = (lane & 31, lane >> 5) holds row c of the fragment's slice and the k of
// split_k_natural / split_k_acc (hh, j) of its k-step
template <class F>
__device__ __forceinline__ void pack_split_fragments(_Float16* out, int64_t n_frags, F value) {
    const int64_t tid0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = tid0; p < n_frags * 1024; p += stride) {
        const int j = (int)(p & 7), lane = (int)(p >> 3) & 63, plane = (int)(p >> 9) & 1;
        const float w = value((int)(p >> 10), lane, j);
        const _Float16 hi = (_Float16)w;
        out[p] = plane == 0 ? hi : (_Float16)(w - (float)hi);
    }
}

// ---- fragment access -------------------------------------------------------------------------------------------------------

// Every global fragment address is  a wave-uniform base  +  ONE opaque per-lane byte offset (lane * 16, kept in a register the compiler
// cannot see through: asm volatile("" : "+v"(lo)))  +  a compile-time constant: left to itself the compiler keeps the ~100 distinct
// fragment addresses of an unrolled step as loop invariants in vector registers and spills them (the finding behind lem_ws3_gemm2 of
// lem_kernel.hip).
__device__ __forceinline__ half8 frag_global(const half8* base, int frag, unsigned lo) {
    return *reinterpret_cast<const half8*>(reinterpret_cast<const char*>(base + frag * 64) + lo);
}
// fragment `frag` of an LDS area; lane_base: the area + lane * 16
__device__ __forceinline__ half8 frag_lds(const char* lane_base, int frag) {
    return *reinterpret_cast<const half8*>(lane_base + frag * 1024);
}

// ---- the GEMM step ---------------------------------------------------------------------------------------------------------

// acc += (ah + al)(bh + bl) without the lo * lo term: three back-to-back MFMAs, small products first (the order of mma_chunk_split)
__device__ __forceinline__ void split_mfma3(const half8& ah, const half8& al, const half8& bh, const half8& bl, f32x16& acc) {
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
}

// acc[nb][r] = the scaled bias of row acc_row(r, hh) of the wave's slice, for every column; bias_slice = bias + 32 T + 4 hh
template <int NB>
__device__ __forceinline__ void acc_bias_init(const float* bias_slice, f32x16 (&acc)[NB]) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(bias_slice + 8 * q);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int nb = 0; nb < NB; ++nb) acc[nb][4 * q + m] = bv[m];
    }
}

// ---- staging B fragments ---------------------------------------------------------------------------------------------------

// 8 consecutive k of one column, split, -> the hi / lo fragments (k-step s, block blk) of an area with NB column blocks; lane_base:
// the area + lane * 16.  NODE: node rows, scaled by 2^8 and saturated (split8_node); otherwise activations of order one (split8).
template <int NB, bool NODE = false>
__device__ __forceinline__ void publish_split(const float (&v)[8], char* lane_base, int s, int blk) {
    half8 hi, lo;
    if constexpr (NODE) split8_node(v, hi, lo);
    else split8(v, hi, lo);
    *reinterpret_cast<half8*>(lane_base + ((2 * s + 0) * NB + blk) * 1024) = hi;
    *reinterpret_cast<half8*>(lane_base + ((2 * s + 1) * NB + blk) * 1024) = lo;
}

// `worst` collects the largest |x| as an integer (the bit patterns of non-negative floats order like their values, NaN above Inf) and is
// compared against NODE_RANGE once, at the end of the kernel: the predicate of out_of_range at two integer operations per value
__device__ __forceinline__ void track_abs_max(unsigned& worst, float x) { worst = max(worst, __float_as_uint(x) & 0x7fffffffu); }
__device__ __forceinline__ bool node_range_exceeded(unsigned worst) { return worst > __float_as_uint(NODE_RANGE); }

// ---- host side ---------------------------------------------------------------------------------------------------------------

inline bool wide_width_ok(const char* who, int width, int max_width = WIDE_MAX_W) {
    if (width < 1 || width > max_width) {
        set_error("%s: width=%d outside 1..%d", who, width, max_width);
        return false;
    }
    return true;
}

// f(std::integral_constant<int, KT>) for KT = kt in 1 .. 8 (8 for anything above)
template <int KT = 1, class F>
inline void dispatch_kt(int kt, F&& f) {
    if constexpr (KT < 8)
        if (kt != KT) return dispatch_kt<KT + 1>(kt, f);
    f(std::integral_constant<int, KT>{});
}

inline int device_cus() {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    return cus;
}

// the grid of a persistent kernel of 64 KT threads and lds_bytes of LDS: as many workgroups as are resident at once (160 KB of LDS per
// CU; two waves per SIMD at up to 256 registers, i.e. 8 waves per CU)
inline long resident_workgroups(int cus, int lds_bytes, int kt) {
    const int by_lds = 160 * 1024 / lds_bytes, by_waves = 8 / kt;
    const int per_cu = by_lds < by_waves ? by_lds : by_waves;
    return (long)cus * (per_cu < 1 ? 1 : per_cu);
}

}  // namespace msmp
