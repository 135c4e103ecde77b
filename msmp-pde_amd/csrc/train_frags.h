// The bf16x3 fragment pieces of the TRAINING kernels that run one 32-row tile per workgroup with a wave per 32-channel slice
// (the recurrent pairs through recurrent_train.h, whose head describes the scheme, and mlp_train_kernel.hip): accumulator tiles <-> rows, the
// publish of a B operand as bf16 hi / mid / lo fragments in "acc order", the streamed weight A fragments and the six-MFMA product.
#pragma once
#include "wide_frags.h"

namespace msmp {

constexpr int LWT_KTILE_U4 = 2 * 3 * 64;                  // one k-tile of a fragment stream or of a published tensor: [s 2][plane 3][lane 64] u32x4, 6 KB
constexpr int LWT_KTILE_FLOATS = LWT_KTILE_U4 * 4;

__device__ __forceinline__ void lwt_store_b3(float* base, int64_t frag /* (stream, s) */, int lane, const float (&v)[8]) {
    const Bf3 f = split_bf16x3(v);
    u32x4* dst = reinterpret_cast<u32x4*>(base) + frag * 3 * 64 + lane;
    dst[0] = __builtin_bit_cast(u32x4, f.hi);
    dst[64] = __builtin_bit_cast(u32x4, f.mid);
    dst[128] = __builtin_bit_cast(u32x4, f.lo);
}

// one tile of a 16-byte aligned row <-> accumulator registers: register 4 q + m is channel 32 ct + 8 q + 4 hh + m (row_hh = row + 4 hh)
__device__ __forceinline__ void lwt_tile_load(const float* row_hh, int ct, f32x16& v) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 p = *reinterpret_cast<const f32x4*>(row_hh + 32 * ct + 8 * q);
#pragma unroll
        for (int m = 0; m < 4; ++m) v[4 * q + m] = p[m];
    }
}
__device__ __forceinline__ void lwt_tile_store(float* row_hh, int ct, const f32x16& v) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x4 p;
#pragma unroll
        for (int m = 0; m < 4; ++m) p[m] = v[4 * q + m];
        *reinterpret_cast<f32x4*>(row_hh + 32 * ct + 8 * q) = p;
    }
}
// the same against a DENSE row of W floats (states, dL/dy_T: any alignment); channels >= W read as 0 and are not written
__device__ __forceinline__ void lwt_dense_load(const float* row, int ct, int hh, int W, f32x16& v) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ch = 32 * ct + acc_row(r, hh);
        v[r] = ch < W ? row[ch] : 0.f;
    }
}
__device__ __forceinline__ void lwt_dense_store(float* row, int ct, int hh, int W, const f32x16& v) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int ch = 32 * ct + acc_row(r, hh);
        if (ch < W) row[ch] = v[r];
    }
}

__device__ __forceinline__ void lwt_publish(u32x4* xf, int ct, int lane, const f32x16& v) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        float t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = v[8 * s + j];
        const Bf3 f = split_bf16x3(t);
        u32x4* dst = xf + (size_t)((ct * 2 + s) * 3) * 64 + lane;
        dst[0] = __builtin_bit_cast(u32x4, f.hi);
        dst[64] = __builtin_bit_cast(u32x4, f.mid);
        dst[128] = __builtin_bit_cast(u32x4, f.lo);
    }
}

struct LwtFrag {
    u32x4 f[2][3];       // [s][plane] of this wave's 32 rows of one k-tile
};
// k-tile i of this wave's stream through BUFFER loads: the descriptor holds the wave's stream base (scalar), the fragment is a scalar offset
// and the lane one 32-bit vector offset.  With global loads the compiler forms a per-lane 64-bit address for each of the 96 fragments of a
// LEM time step, hoists them out of the t loop as invariants and spills them (49 scratch stores at the head of the first edition).
__device__ __forceinline__ void lwt_frag_load(LwtFrag& w, __amdgpu_buffer_rsrc_t stream, int i, unsigned loff) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl) w.f[s][pl] = __builtin_amdgcn_raw_buffer_load_b128(stream, loff, ((i * 2 + s) * 3 + pl) * 1024, 0);
}
// acc (tile ct) += W[32 ct .., k-tile kc] * published[k-tile kc]
__device__ __forceinline__ void lwt_mma(const LwtFrag& w, const u32x4* xf, int kc, int lane, f32x16& acc) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const bf16x8 wh = __builtin_bit_cast(bf16x8, w.f[s][0]), wm = __builtin_bit_cast(bf16x8, w.f[s][1]), wl = __builtin_bit_cast(bf16x8, w.f[s][2]);
        const u32x4* b = xf + (size_t)((kc * 2 + s) * 3) * 64 + lane;
        const bf16x8 bh = __builtin_bit_cast(bf16x8, b[0]), bm = __builtin_bit_cast(bf16x8, b[64]), bl = __builtin_bit_cast(bf16x8, b[128]);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wl, bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, bl, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wm, bm, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wm, bh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, bm, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(wh, bh, acc, 0, 0, 0);
    }
}

}  // namespace msmp
