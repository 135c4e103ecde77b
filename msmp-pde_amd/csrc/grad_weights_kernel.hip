// The weight-gradient kernel pair behind msmp_grad_weights_f32 / _cat_f32 and, through grad_weights.h, behind both layer backwards.
// ----------------------------------------------------------------------------------------------
// Weight gradients:  dW[m][n] = sum_r A[r][m] B[r][n]  and  db[m] = sum_r A[r][m]  for up to GW_MAX_JOBS (A, B) pairs in one call
// (A [R,128] (row stride lda) = gradient of a pre-activation, B [R, >= k2] = the input of that linear layer, R = E or N rows).
// These GEMMs are 128 x k2 outputs with a reduction over R >> 1000 rows: the library runs them on 36 workgroups
// (63 us each at R = 9 408); here the rows are split over workgroups (<= 512 splits per pair; fp32 products from six bf16 MFMAs,
// see split_bf16x3; the bias column as a virtual all-ones column k2 of B), and a second kernel sums the partials in a fixed order
// (deterministic).
// ----------------------------------------------------------------------------------------------
#include "grad_weights.h"
#include "mfma_tiles.h"

namespace msmp {

constexpr int GW_MAX_UNITS = 2 * GW_MAX_JOBS;       // a job of more than 160 columns is two column groups
struct GradWeightJob {
    const float* a;      // [rows, lda], columns 0..127 used
    const float* b;      // [rows, ldb], columns 0..k2-1 used (0..ksplit-1 when b2 is given)
    const float* b2;     // optional second matrix [rows, ldb2]: column c >= ksplit of the virtual B = [b | b2] is b2's column c - ksplit
    float* out_w;        // [128, k2]
    float* out_b;        // [128]
    float* partial;      // [splits][128][ldp]
    int rows, lda, ldb, k2, ldp, rows_per_split, splits, first_block;
    int c0;              // first column of B of this unit's group (0 or 160)
    int ldb2, ksplit;
};
struct GradWeightArgs {
    GradWeightJob job[GW_MAX_JOBS];       // the reduction's view: one entry per job
    GradWeightJob unit[GW_MAX_UNITS];     // the product kernel's view: one entry per (job, column group)
    int n_jobs, n_units;
};

// One workgroup = one row split of one job's column group (<= 5 output tiles = 160 columns of B; jobs with more columns are cut
// into groups so that the accumulators (80 registers) leave room for TWO 16-row blocks of operands in flight (96 registers): the
// loop is bound by load latency otherwise (measured: a 9-tile body with one block in flight ran 2.6x SLOWER than the fp32-MFMA
// kernel it replaced, ten dependent memory round trips per block).
constexpr int GW_NT = 5;
constexpr int GW_FRAG_U4 = GW_NT * 3 * 64;           // 16-byte fragments of one 16-row block of B: [tile][plane][lane] = 15 KB

// One 16-row block: lane (m, kk) of wave w loads rows rbase .. rbase + 7 of column 32 w + m of A (its own MFMA operand) and of
// column c0 + 32 w + m of B (tile w); tile 4 of the group is loaded by the wave whose turn it is (block index mod 4).  Every load is
// a 128-byte row segment across 32 lanes.  B is converted ONCE per workgroup and shared through LDS as bf16x3 fragments: with every
// wave loading and converting all five tiles itself (first round-2 edition) the B rows crossed the L1 four times and the
// conversion was 85 % of the vector work.
struct GwRegs {
    float a[8], b[8], b4[8];
};
template <bool FULL>
__device__ __forceinline__ void gw_load(const GradWeightJob& j, const float* acol, const float* bcol, int bld, const float* bcol4, int bld4, bool mine4,
                                        int rbase, int rlim, GwRegs& r) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const size_t row = FULL ? rbase + i : rbase + min(i, max(rlim - 1, 0));
        const bool in = FULL || i < rlim;
        const float va = acol[row * j.lda], vb = bcol[row * bld];
        r.a[i] = in ? va : 0.f;
        r.b[i] = in ? vb : 0.f;
    }
    if (mine4) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const size_t row = FULL ? rbase + i : rbase + min(i, max(rlim - 1, 0));
            const float v = bcol4[row * bld4];
            r.b4[i] = FULL || i < rlim ? v : 0.f;
        }
    } else {
        // defined on both paths: left untouched here, r.b4 is merged with its old value behind the branch by copies that wait for the
        // loads above (vmcnt(0) with the whole block's loads the youngest in flight: the prefetch was waited for where it was issued)
#pragma unroll
        for (int i = 0; i < 8; ++i) r.b4[i] = 0.f;
    }
}
__device__ __forceinline__ void gw_publish(const float (&b)[8], float keep, float ones, u32x4* frag_tile, int lane) {
    float bv[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) bv[i] = fmaf(b[i], keep, ones);          // column past k2: 0; the bias column k2: 1
    const Bf3 b3 = split_bf16x3(bv);
    frag_tile[lane] = __builtin_bit_cast(u32x4, b3.hi);
    frag_tile[64 + lane] = __builtin_bit_cast(u32x4, b3.mid);
    frag_tile[128 + lane] = __builtin_bit_cast(u32x4, b3.lo);
}
__device__ __forceinline__ void gw_mma(const Bf3& a3, const u32x4* frags, int lane, f32x16 (&acc)[GW_NT]) {
#pragma unroll
    for (int t = 0; t < GW_NT; ++t) {
        const u32x4* f = frags + (size_t)t * 3 * 64 + lane;
        const bf16x8 bh = __builtin_bit_cast(bf16x8, f[0]), bm = __builtin_bit_cast(bf16x8, f[64]), bl = __builtin_bit_cast(bf16x8, f[128]);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3.lo, bh, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3.hi, bl, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3.mid, bm, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3.mid, bh, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3.hi, bm, acc[t], 0, 0, 0);
        acc[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a3.hi, bh, acc[t], 0, 0, 0);
    }
}

// Phase profile (build with MSMP_PROF=gw; scripts/prof_gw.py): cycle sums of wave 0 of every 8th workgroup with at least 100 blocks
#if MSMP_PROF_GW
__device__ unsigned long long g_prof_gw[8];
#define GWP_DECL long long gp[5] = {0, 0, 0, 0, 0}; long long gt = __builtin_readcyclecounter();
#define GWP(i) do { const long long t_ = __builtin_readcyclecounter(); gp[i] += t_ - gt; gt = t_; } while (0)
#define GWP_FLUSH if (wave == 0 && lane == 0 && n_blocks >= 100 && (split & 7) == 0) { for (int i_ = 0; i_ < 5; ++i_) atomicAdd(&g_prof_gw[i_], (unsigned long long)gp[i_]); atomicAdd(&g_prof_gw[6], (unsigned long long)n_blocks); atomicAdd(&g_prof_gw[7], 1ull); }
#else
#define GWP_DECL
#define GWP(i)
#define GWP_FLUSH
#endif
__device__ __forceinline__ void grad_weight_body(const GradWeightJob& j, int split, int wave, int lane, u32x4* frags /* LDS [2][GW_FRAG_U4] */) {
    const int m = lane & 31, kk = lane >> 5;
    f32x16 acc[GW_NT];
#pragma unroll
    for (int t = 0; t < GW_NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;
    const int r0 = split * j.rows_per_split, r1 = min(r0 + j.rows_per_split, j.rows);
    const float* acol = j.a + 32 * wave + m;
    auto colptr = [&](int t, float& keep, float& ones, int& ld) {
        const int c = j.c0 + 32 * t + m;
        keep = c < j.k2 ? 1.0f : 0.f;
        ones = c == j.k2 ? 1.0f : 0.f;
        const bool second = j.b2 != nullptr && c >= j.ksplit && c < j.k2;      // the virtual concatenation [b | b2]
        ld = second ? j.ldb2 : j.ldb;
        return second ? j.b2 + (c - j.ksplit) : j.b + (c < j.k2 ? c : 0);
    };
    float keep, ones, keep4, ones4;
    int bld, bld4;
    const float* bcol = colptr(wave, keep, ones, bld);
    const float* bcol4 = colptr(4, keep4, ones4, bld4);
    const int n_blocks = (r1 - r0 + 15) / 16;            // the last one may be ragged: it takes the predicated loads
    const int n_full = (r1 - r0) / 16;
    GwRegs cur, nxt;
    auto load_block = [&](int blk, GwRegs& dst) {
        const int rb = r0 + 16 * blk + 8 * kk;
        if (blk < n_full) gw_load<true>(j, acol, bcol, bld, bcol4, bld4, (blk & 3) == wave, rb, 8, dst);
        else gw_load<false>(j, acol, bcol, bld, bcol4, bld4, (blk & 3) == wave, min(rb, r1 - 1), r1 - rb, dst);
    };
    GWP_DECL
    if (n_blocks > 0) load_block(0, cur);
    // The first block's values are pinned in registers HERE (an empty asm that "modifies" them: the loads must have landed).  Without it
    // the loop header inherits "loads pending on cur" from this prologue, and the wait the compiler places at the top of the loop for the
    // first trip (vmcnt(14) ... vmcnt(0) through the publish phase) is executed on EVERY trip -- where the youngest loads are the next
    // block's prefetch, issued a few instructions earlier: every block waited for its own prefetch (round 4 phase profile: 2 640 of
    // 5 000 cycles per block).
#pragma unroll
    for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(cur.a[i]), "+v"(cur.b[i]), "+v"(cur.b4[i]));
    __builtin_amdgcn_sched_barrier(0);
    for (int blk = 0; blk < n_blocks; ++blk) {
        if (blk + 1 < n_blocks) load_block(blk + 1, nxt);
        __builtin_amdgcn_sched_barrier(0);               // all loads of the next block are requested before this block's work
        GWP(0);
        u32x4* fb = frags + (size_t)(blk & 1) * GW_FRAG_U4;
        gw_publish(cur.b, keep, ones, fb + (size_t)wave * 3 * 64, lane);
        if ((blk & 3) == wave) gw_publish(cur.b4, keep4, ones4, fb + (size_t)4 * 3 * 64, lane);
        const Bf3 a3 = split_bf16x3(cur.a);
        GWP(1);
        __syncthreads();                                 // fragments of this block visible; the other buffer is free for the next block
        GWP(2);
        gw_mma(a3, fb, lane, acc);
        __builtin_amdgcn_sched_barrier(0);
        GWP(3);
#pragma unroll
        for (int i = 0; i < 8; ++i) { cur.a[i] = nxt.a[i]; cur.b[i] = nxt.b[i]; cur.b4[i] = nxt.b4[i]; }
    }
    GWP(4);
    GWP_FLUSH
    float* p = j.partial + (size_t)split * H * j.ldp + j.c0;
#pragma unroll
    for (int t = 0; t < GW_NT; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (j.c0 + 32 * t < j.ldp) p[(size_t)(32 * wave + acc_row(r, kk)) * j.ldp + 32 * t + m] = acc[t][r];
}

__global__ __launch_bounds__(256, 3) void grad_weight_kernel(GradWeightArgs a) {
    int ji = 0;
#pragma unroll
    for (int i = 1; i < GW_MAX_UNITS; ++i)
        if (i < a.n_units && (int)blockIdx.x >= a.unit[i].first_block) ji = i;
    const GradWeightJob& j = a.unit[ji];
    __shared__ u32x4 frags[2 * GW_FRAG_U4];              // 30 KB
    grad_weight_body(j, blockIdx.x - j.first_block, threadIdx.x >> 6, threadIdx.x & 63, frags);
}

// out[row][col] = sum over splits, in split order; grid.y = job
__global__ __launch_bounds__(256) void grad_weight_reduce_kernel(GradWeightArgs a) {
    const GradWeightJob& j = a.job[blockIdx.y];
    const int w = j.k2 + 1, ldp = j.ldp, total = H * w;
    for (int p = blockIdx.x * blockDim.x + threadIdx.x; p < total; p += gridDim.x * blockDim.x) {
        const int row = p / w, c = p - row * w;
        const float* src = j.partial + (size_t)row * ldp + c;
        float s = 0.f;
        for (int k = 0; k < j.splits; ++k) s += src[(size_t)k * H * ldp];
        if (c < j.k2) j.out_w[(size_t)row * j.k2 + c] = s;
        else j.out_b[row] = s;
    }
}

static int gw_tiles(int k2) { const int t = (k2 + 1 + 31) / 32; return t <= 5 ? 5 : t <= 9 ? 9 : t <= 10 ? 10 : -1; }
// rows per workgroup: 128, more once a pair would exceed its split limit (the partial products, splits x 128 x 32 nt floats, are
// written and re-read by the reduction).  Round 1 measured limits 128 / 256 / 512 with the fp32 kernel (E2 MSMP-PDE): batch 16
// 7.1 / 7.0 / 6.3 ms (the LEM pairs have 40 000 rows), batch 128 15.0 / 14.9 / 14.9, batch 512 51.1 / 49.7 / 48.9.
static int gw_rows_per_split(int64_t rows) {
    // small jobs keep up to 512 splits (they need the parallelism); large ones 128 (measured at batch 512, ms per iteration, cap
    // 512 / 256 / 128 / 64: 24.0 / 23.7 / 23.7 / 25.2: fewer partials to write and re-read until the splits no longer fill the chip)
    const int64_t lim = rows > 32768 ? 128 : 512;
    int64_t rps = 128;
    if ((rows + rps - 1) / rps > lim) rps = ((rows + lim - 1) / lim + 15) / 16 * 16;
    return (int)rps;
}

}  // namespace msmp

using namespace msmp;

#if MSMP_PROF_GW
extern "C" __attribute__((visibility("default"))) int msmp_debug_prof_gw(unsigned long long* out8, int reset) {
    if (reset) { unsigned long long z[8] = {0}; return (int)hipMemcpyToSymbol(HIP_SYMBOL(msmp::g_prof_gw), z, sizeof(z)); }
    return (int)hipMemcpyFromSymbol(out8, HIP_SYMBOL(msmp::g_prof_gw), 8 * sizeof(unsigned long long));
}
#endif
extern "C" int64_t msmp_grad_weights_workspace_floats(int n_jobs, const int64_t* rows, const int* k2) {
    if (n_jobs < 1 || n_jobs > GW_MAX_JOBS || !rows || !k2) return -1;
    int64_t total = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const int nt = gw_tiles(k2[i]);
        if (nt < 0 || rows[i] < 1) return -1;
        const int rps = gw_rows_per_split(rows[i]);
        total += ((rows[i] + rps - 1) / rps) * H * 32 * nt;
    }
    return total;
}

namespace msmp {
// launches of msmp_grad_weights_f32 on validated arguments (also used by the two layer backwards: grad_weights.h)
int launch_grad_weights(int n_jobs, const float* const* a, const float* const* b, const int64_t* rows, const int* lda,
                        const int* ldb, const int* k2, float* const* out_w, float* const* out_b, float* workspace,
                        int64_t workspace_floats, hipStream_t stream, const float* const* b2, const int* ldb2, const int* ksplit) {
    GradWeightArgs args;
    args.n_jobs = n_jobs;
    int64_t used = 0;
    int blocks = 0, max_w = 0, nu = 0;
    for (int i = 0; i < n_jobs; ++i) {
        MSMP_REQUIRE(a[i] && b[i] && out_w[i] && out_b[i], MSMP_ERR_ARG, "msmp_grad_weights_f32: null pointer in job %d", i);
        MSMP_REQUIRE(rows[i] >= 1 && rows[i] < (1L << 31) && k2[i] >= 1 && (ldb[i] >= k2[i] || (b2 && b2[i])) && lda[i] >= H, MSMP_ERR_ARG, "msmp_grad_weights_f32: bad sizes in job %d", i);
        const int nt = gw_tiles(k2[i]);
        MSMP_REQUIRE(nt > 0, MSMP_ERR_UNSUPPORTED, "msmp_grad_weights_f32: k2=%d > 319", k2[i]);
        GradWeightJob& j = args.job[i];
        j.a = a[i]; j.b = b[i]; j.out_w = out_w[i]; j.out_b = out_b[i]; j.partial = workspace + used;
        j.b2 = b2 ? b2[i] : nullptr; j.ldb2 = j.b2 ? ldb2[i] : 0; j.ksplit = j.b2 ? ksplit[i] : 0;
        MSMP_REQUIRE(!j.b2 || (j.ksplit >= 1 && j.ksplit < k2[i] && j.ldb2 >= k2[i] - j.ksplit && ldb[i] >= j.ksplit), MSMP_ERR_ARG, "msmp_grad_weights_f32: bad split of job %d", i);
        j.rows = (int)rows[i]; j.lda = lda[i]; j.ldb = ldb[i]; j.k2 = k2[i]; j.ldp = 32 * nt;
        j.rows_per_split = gw_rows_per_split(rows[i]);
        j.splits = (j.rows + j.rows_per_split - 1) / j.rows_per_split;
        j.first_block = 0; j.c0 = 0;
        for (int c0 = 0; c0 < 32 * nt; c0 += 32 * GW_NT) {
            GradWeightJob& u = args.unit[nu++];
            u = j; u.c0 = c0; u.first_block = blocks;
            blocks += j.splits;
        }
        used += (int64_t)j.splits * H * 32 * nt;
        max_w = k2[i] + 1 > max_w ? k2[i] + 1 : max_w;
    }
    args.n_units = nu;
    for (int i = n_jobs; i < GW_MAX_JOBS; ++i) args.job[i] = args.job[0];
    for (int i = nu; i < GW_MAX_UNITS; ++i) args.unit[i] = args.unit[0];
    MSMP_REQUIRE(used <= workspace_floats, MSMP_ERR_WORKSPACE, "msmp_grad_weights_f32: workspace of %ld floats, need %ld", (long)workspace_floats, (long)used);
    hipLaunchKernelGGL(grad_weight_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, args);
    hipLaunchKernelGGL(grad_weight_reduce_kernel, dim3((unsigned)((H * max_w + 255) / 256), (unsigned)n_jobs), dim3(256), 0, stream, args);
    return check_launch("grad_weight_kernel");
}
}  // namespace msmp

extern "C" int msmp_grad_weights_f32(int n_jobs, const float* const* a, const float* const* b, const int64_t* rows, const int* lda,
                                     const int* ldb, const int* k2, float* const* out_w, float* const* out_b, float* workspace,
                                     int64_t workspace_floats, msmp_stream_t stream) {
    MSMP_REQUIRE(n_jobs >= 1 && n_jobs <= GW_MAX_JOBS, MSMP_ERR_ARG, "msmp_grad_weights_f32: n_jobs=%d not in 1..%d", n_jobs, GW_MAX_JOBS);
    MSMP_REQUIRE(a && b && rows && lda && ldb && k2 && out_w && out_b && workspace, MSMP_ERR_ARG, "msmp_grad_weights_f32: null pointer");
    return launch_grad_weights(n_jobs, a, b, rows, lda, ldb, k2, out_w, out_b, workspace, workspace_floats, (hipStream_t)stream);
}

extern "C" int msmp_grad_weights_cat_f32(int n_jobs, const float* const* a, const float* const* b, const float* const* b2, const int64_t* rows,
                                         const int* lda, const int* ldb, const int* ldb2, const int* ksplit, const int* k2, float* const* out_w,
                                         float* const* out_b, float* workspace, int64_t workspace_floats, msmp_stream_t stream) {
    MSMP_REQUIRE(n_jobs >= 1 && n_jobs <= GW_MAX_JOBS, MSMP_ERR_ARG, "msmp_grad_weights_cat_f32: n_jobs=%d not in 1..%d", n_jobs, GW_MAX_JOBS);
    MSMP_REQUIRE(a && b && b2 && rows && lda && ldb && ldb2 && ksplit && k2 && out_w && out_b && workspace, MSMP_ERR_ARG, "msmp_grad_weights_cat_f32: null pointer");
    return launch_grad_weights(n_jobs, a, b, rows, lda, ldb, k2, out_w, out_b, workspace, workspace_floats, (hipStream_t)stream, b2, ldb2, ksplit);
}
