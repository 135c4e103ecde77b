// msmp_grad_weights_f32 on validated arguments (grad_weights_kernel.hip) for the two layer backwards; library-internal.
#pragma once
#include "msmp_common.h"

namespace msmp {
constexpr int GW_MAX_JOBS = 10;
int launch_grad_weights(int n_jobs, const float* const* a, const float* const* b, const int64_t* rows, const int* lda, const int* ldb,
                        const int* k2, float* const* out_w, float* const* out_b, float* workspace, int64_t workspace_floats,
                        hipStream_t stream, const float* const* b2 = nullptr, const int* ldb2 = nullptr, const int* ksplit = nullptr);
}  // namespace msmp
