// The pieces of a training step around the gradients (reductions.py, optim.py, train.py): deterministic reductions, fused AdamW in its
// eager, capturable and guarded forms, the finite check of the gradients and the range-status poison.  No MFMA, nothing shared with the
// layer kernels.
#include "msmp_common.h"

using namespace msmp;

// ------------------------------------------------------------------------------------------------------------------------
// Deterministic reductions for the pieces of a training iteration that stay in PyTorch (encoder / decoder bias gradients, the loss
// sum, experiments/train_helper.py:125-141): two launches each, partial sums in a caller's workspace, fixed order, no atomics and
// no zero-initialised semaphore -- a library reduction's hipMemsetAsync becomes a memset NODE in a captured training step and was
// seen to replay out of order.
// ------------------------------------------------------------------------------------------------------------------------
namespace msmp {
constexpr int RED_BLOCKS = 128;
// partial[b][c] = sum of x[r][c] over the rows of block b
__global__ __launch_bounds__(256) void colsum_partial_kernel(const float* __restrict__ x, long rows, int cols, float* __restrict__ partial) {
    const long per = (rows + gridDim.x - 1) / gridDim.x;
    const long r0 = (long)blockIdx.x * per, r1 = min(r0 + per, rows);
    for (int c = threadIdx.x; c < cols; c += 256) {
        float s = 0.f;
        for (long r = r0; r < r1; ++r) s += x[(size_t)r * cols + c];
        partial[(size_t)blockIdx.x * cols + c] = s;
    }
}
__device__ __forceinline__ float block_sum_256(float v, float* red) {       // fixed tree, every thread returns the total
    red[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}
// out[j] = sum over blocks and over the `group` consecutive columns of output j: one workgroup per output, element (b, g) of the
// blocks x group set at thread (b group + g) % 256 -- fixed order, then the fixed tree
__global__ __launch_bounds__(256) void colsum_final_kernel(const float* __restrict__ partial, int blocks, int cols, int group, float* __restrict__ out) {
    __shared__ float red[256];
    const int j = blockIdx.x;
    float s = 0.f;
    for (int i = threadIdx.x; i < blocks * group; i += 256) s += partial[(size_t)(i / group) * cols + j * group + i % group];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) out[j] = s;
}
__global__ __launch_bounds__(256) void sqerr_partial_kernel(const float* __restrict__ a, const float* __restrict__ b, long n, float* __restrict__ partial) {
    __shared__ float red[256];
    float s = 0.f;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const float d = a[i] - b[i];
        s = fmaf(d, d, s);
    }
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void sum_final_kernel(const float* __restrict__ partial, int n, float* __restrict__ out) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    s = block_sum_256(s, red);
    if (threadIdx.x == 0) out[0] = s;
}
}  // namespace msmp

extern "C" size_t msmp_reduce_workspace_bytes(int cols) { return (size_t)RED_BLOCKS * (size_t)(cols > 1 ? cols : 1) * sizeof(float); }

extern "C" int msmp_colsum_f32(const float* x, int64_t rows, int cols, int group, float* out, void* workspace, size_t workspace_bytes,
                               msmp_stream_t stream) {
    MSMP_REQUIRE(x && out && workspace, MSMP_ERR_ARG, "msmp_colsum_f32: null pointer");
    MSMP_REQUIRE(rows >= 0 && cols >= 1 && group >= 1 && cols % group == 0, MSMP_ERR_ARG, "msmp_colsum_f32: bad sizes");
    MSMP_REQUIRE(workspace_bytes >= msmp_reduce_workspace_bytes(cols), MSMP_ERR_WORKSPACE, "msmp_colsum_f32: workspace %zu < %zu", workspace_bytes,
                 msmp_reduce_workspace_bytes(cols));
    const int blocks = (int)(rows < RED_BLOCKS ? (rows > 0 ? rows : 1) : RED_BLOCKS);
    hipLaunchKernelGGL(colsum_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, (long)rows, cols, (float*)workspace);
    hipLaunchKernelGGL(colsum_final_kernel, dim3((unsigned)(cols / group)), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, blocks,
                       cols, group, out);
    return check_launch("colsum_kernel");
}

extern "C" int msmp_sqerr_sum_f32(const float* a, const float* b, int64_t n, float* out, void* workspace, size_t workspace_bytes,
                                  msmp_stream_t stream) {
    MSMP_REQUIRE(a && b && out && workspace, MSMP_ERR_ARG, "msmp_sqerr_sum_f32: null pointer");
    MSMP_REQUIRE(n >= 0 && workspace_bytes >= msmp_reduce_workspace_bytes(1), MSMP_ERR_ARG, "msmp_sqerr_sum_f32: bad sizes / workspace");
    hipLaunchKernelGGL(sqerr_partial_kernel, dim3(RED_BLOCKS), dim3(256), 0, (hipStream_t)stream, a, b, (long)n, (float*)workspace);
    hipLaunchKernelGGL(sum_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, RED_BLOCKS, out);
    return check_launch("sqerr_sum_kernel");
}

// ------------------------------------------------------------------------------------------------------------------------
// Fused AdamW (experiments/train.py:410: optim.AdamW(model.parameters(), lr)): every parameter tensor of the model in one or two
// launches.  A launch carries up to ADAMW_MAX_TENSORS tensor descriptors in its kernel arguments; block b works on chunk
// (b - first_block[t]) of tensor t.  Decoupled weight decay, bias-corrected moments, the same order of operations as
// torch.optim.AdamW (p *= 1 - lr wd;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  p -= lr / bc1 * m / (sqrt(v) / sqrt(bc2) + eps)).
// ------------------------------------------------------------------------------------------------------------------------
namespace msmp {
constexpr int ADAMW_MAX_TENSORS = 48;
constexpr int ADAMW_CHUNK = 4096;           // elements per block (256 threads x 4 x 4)
struct AdamWArgs {
    float* p[ADAMW_MAX_TENSORS];
    const float* g[ADAMW_MAX_TENSORS];
    float* m[ADAMW_MAX_TENSORS];
    float* v[ADAMW_MAX_TENSORS];
    int numel[ADAMW_MAX_TENSORS];
    int first_block[ADAMW_MAX_TENSORS + 1];
    int n;
    float lr, beta1, beta2, eps, decay, bc1_inv, bc2_rsqrt;      // decay = 1 - lr wd;  bc1_inv = 1 / (1 - b1^t);  bc2_rsqrt = 1 / sqrt(1 - b2^t)
    // capturable form (a hipGraph replays the same kernel arguments): step count and learning rate are read from device memory
    const long long* step_dev;
    const float* lr_dev;
    float weight_decay;
    const int* verdict_dev;     // guarded form only (msmp_adamw_guarded_f32): a non-zero word leaves every tensor alone
};

__global__ void adamw_advance_kernel(long long* step) {
    if (threadIdx.x == 0 && blockIdx.x == 0) step[0] += 1;
}

template <bool DEV, bool GUARD = false>
__global__ __launch_bounds__(256) void adamw_kernel(AdamWArgs a) {
    if (GUARD && a.verdict_dev[0] != 0) return;          // uniform over the grid: the same word for every block
    int t = 0;
    while (t + 1 < a.n && (int)blockIdx.x >= a.first_block[t + 1]) ++t;
    const int base = ((int)blockIdx.x - a.first_block[t]) * ADAMW_CHUNK;
    const int n = a.numel[t];
    float* __restrict__ p = a.p[t];
    const float* __restrict__ g = a.g[t];
    float* __restrict__ m = a.m[t];
    float* __restrict__ v = a.v[t];
    if (DEV) {          // the host entry's arithmetic, per block (two pow calls: nothing beside 4096 elements)
        const double st = (double)a.step_dev[0];
        a.lr = a.lr_dev[0];
        a.decay = 1.0f - a.lr * a.weight_decay;
        a.bc1_inv = (float)(1.0 / (1.0 - pow((double)a.beta1, st)));
        a.bc2_rsqrt = (float)(1.0 / sqrt(1.0 - pow((double)a.beta2, st)));
    }
    const float step = a.lr * a.bc1_inv;
#pragma unroll
    for (int k = 0; k < ADAMW_CHUNK / 256; ++k) {
        const int i = base + k * 256 + threadIdx.x;
        if (i < n) {
            const float gi = g[i];
            const float mi = a.beta1 * m[i] + (1.0f - a.beta1) * gi;
            const float vi = a.beta2 * v[i] + (1.0f - a.beta2) * gi * gi;
            m[i] = mi;
            v[i] = vi;
            p[i] = p[i] * a.decay - step * (mi / (sqrtf(vi) * a.bc2_rsqrt + a.eps));
        }
    }
}
}  // namespace msmp

static int adamw_launch(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                        float* const* exp_avg_sq, const int64_t* numel, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int64_t step, int64_t* step_dev, const float* lr_dev, msmp_stream_t stream,
                        const int* verdict_dev = nullptr);

extern "C" int msmp_adamw_f32(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                              float* const* exp_avg_sq, const int64_t* numel, float lr, float beta1, float beta2, float eps,
                              float weight_decay, int64_t step, msmp_stream_t stream) {
    MSMP_REQUIRE(step >= 1, MSMP_ERR_ARG, "msmp_adamw_f32: bad hyper-parameters");
    return adamw_launch(n_tensors, params, grads, exp_avg, exp_avg_sq, numel, lr, beta1, beta2, eps, weight_decay, step, nullptr, nullptr, stream);
}

extern "C" int msmp_adamw_capturable_f32(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                                         float* const* exp_avg_sq, const int64_t* numel, const float* lr_dev, float beta1, float beta2,
                                         float eps, float weight_decay, int64_t* step_dev, msmp_stream_t stream) {
    MSMP_REQUIRE(lr_dev && step_dev, MSMP_ERR_ARG, "msmp_adamw_capturable_f32: null pointer");
    hipLaunchKernelGGL(adamw_advance_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long*)step_dev);
    return adamw_launch(n_tensors, params, grads, exp_avg, exp_avg_sq, numel, 0.f, beta1, beta2, eps, weight_decay, 1, step_dev, lr_dev, stream);
}

static int adamw_launch(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                        float* const* exp_avg_sq, const int64_t* numel, float lr, float beta1, float beta2, float eps,
                        float weight_decay, int64_t step, int64_t* step_dev, const float* lr_dev, msmp_stream_t stream,
                        const int* verdict_dev) {
    MSMP_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || (params && grads && exp_avg && exp_avg_sq && numel)), MSMP_ERR_ARG, "msmp_adamw_f32: null pointer");
    MSMP_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, MSMP_ERR_ARG, "msmp_adamw_f32: bad hyper-parameters");
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    for (int t0 = 0; t0 < n_tensors; t0 += ADAMW_MAX_TENSORS) {
        AdamWArgs a;
        a.n = n_tensors - t0 < ADAMW_MAX_TENSORS ? n_tensors - t0 : ADAMW_MAX_TENSORS;
        int blocks = 0;
        for (int i = 0; i < a.n; ++i) {
            MSMP_REQUIRE(((params[t0 + i] && grads[t0 + i] && exp_avg[t0 + i] && exp_avg_sq[t0 + i]) || numel[t0 + i] == 0) && numel[t0 + i] >= 0 &&
                             numel[t0 + i] < (1L << 31),          // an empty tensor is never read or written: no block is its own
                         MSMP_ERR_ARG, "msmp_adamw_f32: bad tensor %d (null pointer or element count)", t0 + i);
            a.p[i] = params[t0 + i]; a.g[i] = grads[t0 + i]; a.m[i] = exp_avg[t0 + i]; a.v[i] = exp_avg_sq[t0 + i];
            a.numel[i] = (int)numel[t0 + i];
            a.first_block[i] = blocks;
            blocks += (int)((numel[t0 + i] + ADAMW_CHUNK - 1) / ADAMW_CHUNK);
        }
        a.first_block[a.n] = blocks;
        a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.decay = 1.0f - lr * weight_decay;
        a.bc1_inv = (float)(1.0 / bc1); a.bc2_rsqrt = (float)(1.0 / sqrt(bc2));
        a.step_dev = (const long long*)step_dev; a.lr_dev = lr_dev; a.weight_decay = weight_decay; a.verdict_dev = verdict_dev;
        if (blocks && step_dev && verdict_dev) hipLaunchKernelGGL((adamw_kernel<true, true>), dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
        else if (blocks && step_dev) hipLaunchKernelGGL(adamw_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
        else if (blocks) hipLaunchKernelGGL(adamw_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
    }
    return check_launch("adamw_kernel");
}

// ------------------------------------------------------------------------------------------------------------------------
// The guard of a training step (experiments/train_helper.py:125-141 has none: the reference has no input range to leave).  A
// non-finite loss gives non-finite gradients, and AdamW writes them into every weight and both moments; these three entries let
// the step refuse such an update without a host read-back, so a captured step stays one graph:
//   msmp_status_poison_f32    the sticky range status becomes a NaN in the loss scalar (every rank of a data-parallel step then
//                             sees it through the scalar all-reduce it makes anyway);
//   msmp_grads_finite_f32     one int32 verdict over all gradients and a few watched scalars, by the rules of the reductions
//                             above: every block overwrites its own workspace slot, a final block overwrites the verdict;
//   msmp_adamw_guarded_f32    msmp_adamw_capturable_f32 that leaves everything alone, and counts, when the verdict is not 0.
// ------------------------------------------------------------------------------------------------------------------------
namespace msmp {
constexpr int FINITE_MAX_SCALARS = 4;
struct FiniteArgs {
    const float* g[ADAMW_MAX_TENSORS];
    int numel[ADAMW_MAX_TENSORS];
    int first_block[ADAMW_MAX_TENSORS + 1];
    int n;
    int* slots;          // this launch's part of the workspace: one word per block
};
struct FiniteScalars {
    const float* s[FINITE_MAX_SCALARS];
    int n;
};

__device__ __forceinline__ int nonfinite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }      // exponent all ones: NaN, +-Inf

// slot[block] = 1 if one of the block's 4096 elements is NaN or +-Inf, else 0 (written either way: nothing is zeroed beforehand)
__global__ __launch_bounds__(256) void finite_partial_kernel(FiniteArgs a) {
    int t = 0;
    while (t + 1 < a.n && (int)blockIdx.x >= a.first_block[t + 1]) ++t;
    const int base = ((int)blockIdx.x - a.first_block[t]) * ADAMW_CHUNK;
    const int n = a.numel[t];
    const float* __restrict__ g = a.g[t];
    int bad = 0;
#pragma unroll
    for (int k = 0; k < ADAMW_CHUNK / 256; ++k) {
        const int i = base + k * 256 + threadIdx.x;
        if (i < n) bad |= nonfinite_bits(g[i]);
    }
    bad = __syncthreads_or(bad);
    if (threadIdx.x == 0) a.slots[blockIdx.x] = bad ? 1 : 0;
}

// verdict[0] = (any slot set ? GRAD : 0) | (any watched scalar non-finite ? SCALAR : 0), overwritten on every run
__global__ __launch_bounds__(256) void finite_final_kernel(const int* __restrict__ slots, int n_slots, FiniteScalars sc, int* __restrict__ verdict) {
    int bad = 0;
    for (int i = threadIdx.x; i < n_slots; i += 256) bad |= slots[i];
    bad = __syncthreads_or(bad);
    int sbad = 0;
    if ((int)threadIdx.x < sc.n) sbad = nonfinite_bits(sc.s[threadIdx.x][0]);
    sbad = __syncthreads_or(sbad);
    if (threadIdx.x == 0) verdict[0] = (bad ? MSMP_NONFINITE_GRAD : 0) | (sbad ? MSMP_NONFINITE_SCALAR : 0);
}

// the guarded form of adamw_advance_kernel: a refused step advances the other counter
__global__ void adamw_advance_guarded_kernel(long long* step, const int* verdict, long long* skipped) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        if (verdict[0] == 0) step[0] += 1;
        else skipped[0] += 1;
    }
}

// scalar[0] = NaN if the status word is raised (system scope: the word may be host memory, and the forward's kernels raised it with
// system-scope atomic ORs earlier in this stream)
__global__ __launch_bounds__(64) void status_poison_kernel(const int* status, float* scalar) {
    if (threadIdx.x == 0 && __hip_atomic_load(status, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM) != 0) scalar[0] = __uint_as_float(0x7fc00000u);
}

static int64_t finite_blocks(int n_tensors, const int64_t* numel) {
    int64_t blocks = 0;
    for (int i = 0; i < n_tensors; ++i) {
        if (numel[i] < 0 || numel[i] >= (1L << 31)) return -1;
        blocks += (numel[i] + ADAMW_CHUNK - 1) / ADAMW_CHUNK;
    }
    return blocks;
}
}  // namespace msmp

extern "C" size_t msmp_grads_finite_workspace_bytes(int n_tensors, const int64_t* numel) {
    if (n_tensors < 0 || (n_tensors > 0 && !numel)) return 0;
    const int64_t blocks = finite_blocks(n_tensors, numel);
    return blocks < 0 ? 0 : (size_t)(blocks > 0 ? blocks : 1) * sizeof(int);
}

extern "C" int msmp_grads_finite_f32(int n_tensors, const float* const* grads, const int64_t* numel, int n_scalars, const float* const* scalars,
                                     int32_t* verdict_dev, void* workspace, size_t workspace_bytes, msmp_stream_t stream) {
    MSMP_REQUIRE(n_tensors >= 0 && n_scalars >= 0 && n_scalars <= FINITE_MAX_SCALARS, MSMP_ERR_ARG,
                 "msmp_grads_finite_f32: bad counts (n_tensors=%d, n_scalars=%d not in 0..%d)", n_tensors, n_scalars, FINITE_MAX_SCALARS);
    MSMP_REQUIRE(verdict_dev && workspace && (n_tensors == 0 || (grads && numel)) && (n_scalars == 0 || scalars), MSMP_ERR_ARG,
                 "msmp_grads_finite_f32: null pointer");
    FiniteScalars sc;
    sc.n = n_scalars;
    for (int i = 0; i < FINITE_MAX_SCALARS; ++i) {
        MSMP_REQUIRE(i >= n_scalars || scalars[i], MSMP_ERR_ARG, "msmp_grads_finite_f32: null pointer (scalar %d)", i);
        sc.s[i] = i < n_scalars ? scalars[i] : nullptr;
    }
    for (int i = 0; i < n_tensors; ++i)
        MSMP_REQUIRE((grads[i] || numel[i] == 0) && numel[i] >= 0 && numel[i] < (1L << 31), MSMP_ERR_ARG,       // an empty tensor is never read
                     "msmp_grads_finite_f32: bad tensor %d (null pointer or element count)", i);
    const int64_t total = finite_blocks(n_tensors, numel);
    MSMP_REQUIRE(total < (1L << 31), MSMP_ERR_ARG, "msmp_grads_finite_f32: bad sizes (%ld chunks)", (long)total);
    MSMP_REQUIRE(workspace_bytes >= msmp_grads_finite_workspace_bytes(n_tensors, numel), MSMP_ERR_WORKSPACE, "msmp_grads_finite_f32: workspace %zu < %zu",
                 workspace_bytes, msmp_grads_finite_workspace_bytes(n_tensors, numel));
    int* slots = static_cast<int*>(workspace);
    int used = 0;
    for (int t0 = 0; t0 < n_tensors; t0 += ADAMW_MAX_TENSORS) {
        FiniteArgs a;
        a.n = n_tensors - t0 < ADAMW_MAX_TENSORS ? n_tensors - t0 : ADAMW_MAX_TENSORS;
        int blocks = 0;
        for (int i = 0; i < a.n; ++i) {
            a.g[i] = grads[t0 + i];
            a.numel[i] = (int)numel[t0 + i];
            a.first_block[i] = blocks;
            blocks += (int)((numel[t0 + i] + ADAMW_CHUNK - 1) / ADAMW_CHUNK);
        }
        a.first_block[a.n] = blocks;
        a.slots = slots + used;
        if (blocks) hipLaunchKernelGGL(finite_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a);
        used += blocks;
    }
    hipLaunchKernelGGL(finite_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const int*)slots, used, sc, (int*)verdict_dev);
    return check_launch("finite_kernel");
}

extern "C" int msmp_adamw_guarded_f32(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                                      float* const* exp_avg_sq, const int64_t* numel, const float* lr_dev, float beta1, float beta2,
                                      float eps, float weight_decay, int64_t* step_dev, const int32_t* verdict_dev, int64_t* skipped_dev,
                                      msmp_stream_t stream) {
    MSMP_REQUIRE(lr_dev && step_dev && verdict_dev && skipped_dev, MSMP_ERR_ARG, "msmp_adamw_guarded_f32: null pointer");
    // everything adamw_launch refuses is refused here first: the counters must not move for a call that updates nothing
    MSMP_REQUIRE(n_tensors >= 0 && (n_tensors == 0 || (params && grads && exp_avg && exp_avg_sq && numel)), MSMP_ERR_ARG, "msmp_adamw_guarded_f32: null pointer");
    MSMP_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, MSMP_ERR_ARG, "msmp_adamw_guarded_f32: bad hyper-parameters");
    for (int i = 0; i < n_tensors; ++i)
        MSMP_REQUIRE(((params[i] && grads[i] && exp_avg[i] && exp_avg_sq[i]) || numel[i] == 0) && numel[i] >= 0 && numel[i] < (1L << 31),
                     MSMP_ERR_ARG,          // an empty tensor is never read or written
                     "msmp_adamw_guarded_f32: bad tensor %d (null pointer or element count)", i);
    hipLaunchKernelGGL(adamw_advance_guarded_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (long long*)step_dev, (const int*)verdict_dev,
                       (long long*)skipped_dev);
    return adamw_launch(n_tensors, params, grads, exp_avg, exp_avg_sq, numel, 0.f, beta1, beta2, eps, weight_decay, 1, step_dev, lr_dev, stream,
                        (const int*)verdict_dev);
}

extern "C" int msmp_status_poison_f32(float* scalar, msmp_stream_t stream) {
    MSMP_REQUIRE(scalar, MSMP_ERR_ARG, "msmp_status_poison_f32: null pointer");
    const int* status = status_ptr();
    if (!status) return MSMP_OK;          // no status word: nothing can have been raised
    hipLaunchKernelGGL(status_poison_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, status, scalar);
    return check_launch("status_poison_kernel");
}
