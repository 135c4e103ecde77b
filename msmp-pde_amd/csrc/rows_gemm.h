// The fp32-exact bf16x3 row GEMM and its weight-split launch (rows_gemm_kernel.hip) for the two layer backwards; library-internal.
#pragma once
#include "mfma_tiles.h"

namespace msmp {
// weights as pre-split bf16x3 fragments, 24-KB chunks of 32 k
constexpr int RG_CHUNK_U4 = 2 * 4 * 3 * 64;            // 16-byte fragments per 32-k chunk: [s][T][plane][lane]
constexpr int RG_CHUNK_FLOATS = RG_CHUNK_U4 * 4;       // 24 KB
struct RgPackJob {
    const float* w;      // row-major, row stride ldw
    u32x4* out;          // n_chunks * RG_CHUNK_U4 fragments
    int ldw, K, n_chunks, col0, transposed, n_rows;     // rows (output channels) >= n_rows read as zero (forward form; msmp_linear_f32's last group)
    // transposed = 0: W_eff[o][k] = w[(col0 + o) * ldw + k]   (forward form: rows of w are output channels)
    // transposed = 1: W_eff[o][k] = w[k * ldw + col0 + o]     (data-gradient form: the reduction runs over w's rows)
    int first_block;
};
constexpr int RG_MAX_PACK = 24;
struct RgPackArgs {
    RgPackJob job[RG_MAX_PACK];
    int n_jobs;
};

// one more 128-channel group of a weight matrix in `a` (see RgPackJob); blocks: running workgroup count of the split launch
void add_pack(RgPackArgs& a, int& blocks, const float* w, int ldw, int K, int col0, int transposed, u32x4* out);
// the split launch for the jobs collected by add_pack (rg_pack_kernel)
int launch_rg_pack(RgPackArgs& a, int blocks, hipStream_t st);
// OUT[rows, 128] = epilogue(X[rows, K] W_eff^T); the epilogues are listed at rows_gemm_kernel.  EPI 1, 3 and 5 take any output row stride
// ld0; EPI 0 and 2 read / write their second tensor at row stride 128.
int rows_gemm(int epi, const float* x, int ldx, long rows, int K, const u32x4* wfrag, const float* bias, const float* aux, float* out0,
              int ld0, float* out1, hipStream_t st);
}  // namespace msmp
