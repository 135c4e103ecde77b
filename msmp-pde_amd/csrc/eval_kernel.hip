// Evaluation of one rollout step against a device-resident dataset: what the reference's test loops make of a prediction and the labels
// of its window -- criterion(pred, graph.y) with MSELoss(reduction='sum') (experiments/train_helper.py:184, 239, 261) and
// torch.square(pred - graph.y), torch.square(graph.y) of compute_L2_norms (:400-401, :430-431) -- as ONE launch that reads the labels
// straight from the store (no label tensor exists) and writes the time column create_next_graph (common/utils.py:454-469) gives the
// next window.  For graph b with s = sample_idx[b], p = steps[b], component c and time offset k < tw:
//
//   d_i = pred[b nx + i, c tw + k] - store[s, p + k, c, i]      (float32, as `pred - graph.y`)
//   err_out[b ld + c tw + k] = sum_i (double)d_i (double)d_i     nrm_out[b ld + c tw + k] = sum_i (double)y_i (double)y_i,  y_i the label
//   pos_out[2 (b nx + i)]    = t_axis[p + tw]  where p + tw <= nt - tw (else the column keeps its bytes; column 1 is never touched)
//
// One work item is a (graph, component), taken by one workgroup of 256 threads; which workgroup takes it changes nothing.  With
// KP = the power of two >= tw and NS = min(64, 256 / KP), thread (j, k) = (tid / KP, tid % KP), j < NS, k < tw, owns column k and the
// nodes i with (i mod 64) mod NS == j.  ORDER OF SUMMATION of a column, the same at every batch and grid size: thread (j, k) adds its
// nodes' terms to a float64 partial in ascending i (64-node chunk after chunk); the NS partials are then added in ascending j,
// starting from partial 0.  The work item walks the 64-node chunks in ascending order: the chunk's [tw, 64] label window goes through
// LDS as in batch_assemble_kernel (256-byte row segments, one wave per time row, odd row stride 65), `pred` is read along its rows
// (consecutive threads walk k within a node) before the barrier, so its latency overlaps the staging.
//
// The indices cannot be checked by the host.  A graph whose s is outside 0 .. n_samples - 1 or whose p is outside tw .. nt - tw reads
// nothing from `store` (nor from `pred`): its comps tw entries of both outputs are quiet NaNs, its pos_out rows, where written, come
// from the clamped p, and every other graph is what it would have been.  No allocation, no synchronisation, no atomic, no memset:
// the launch holds pointers and sizes only and can be captured.
#include "msmp_common.h"

namespace msmp {

constexpr int EW_THREADS = 256;
constexpr int EW_NODES = 64;              // nodes per chunk: one 256-byte row segment per wave load
constexpr int EW_MAX_TW = 64;
constexpr int EW_LD = EW_NODES + 1;       // odd LDS row stride
constexpr int EW_MAX_PER = EW_MAX_TW / 4; // nodes of a chunk per thread at the widest window (KP = 64, NS = 4)

struct EvalWindowArgs {
    const float* store;
    const int32_t* sample_idx;
    const int32_t* steps;
    const float* pred;
    const float* t_axis;
    double* err_out;
    double* nrm_out;
    float* pos_out;
    long n_samples;
    long n_items;        // batch * comps
    long ld;
    int nt, comps, nx, tw, kshift;       // KP = 1 << kshift
};

__global__ __launch_bounds__(EW_THREADS) void eval_window_kernel(const EvalWindowArgs a) {
    __shared__ float tile[EW_MAX_TW * EW_LD];
    __shared__ double part[2][EW_THREADS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tw = a.tw, nx = a.nx, comps = a.comps;
    const int kp = 1 << a.kshift;
    const int ns = min(EW_NODES, EW_THREADS / kp);
    const int per = EW_NODES / ns;                            // nodes of a chunk per thread: 1 .. EW_MAX_PER
    const int k = tid & (kp - 1), sub = tid >> a.kshift;
    const bool active = k < tw && sub < ns;
    const long ld_p = (long)comps * tw;
    const double qnan = __builtin_nan("");

    for (long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int c = (int)(item % comps);
        const int b = (int)(item / comps);
        const int s = a.sample_idx[b], p = a.steps[b];
        const bool valid = s >= 0 && (long)s < a.n_samples && p >= tw && p <= a.nt - tw;      // the same for every thread
        double err = 0.0, nrm = 0.0;

        if (valid) {
            const float* src0 = a.store + (((long)s * a.nt + p) * comps + c) * nx;
            const long row_stride = (long)comps * nx;
            const float* pr0 = a.pred + (long)b * nx * ld_p + c * tw + k;
            for (int i0 = 0; i0 < nx; i0 += EW_NODES) {
                const int n_here = min(EW_NODES, nx - i0);
                float pv[EW_MAX_PER];
#pragma unroll
                for (int j = 0; j < EW_MAX_PER; ++j) {
                    const int node = sub + j * ns;
                    pv[j] = (active && j < per && node < n_here) ? pr0[(long)(i0 + node) * ld_p] : 0.0f;
                }
                if (lane < n_here) {
                    const float* src = src0 + i0 + lane;
#pragma unroll 8
                    for (int r = wave; r < tw; r += EW_THREADS / 64) tile[r * EW_LD + lane] = src[r * row_stride];
                }
                __syncthreads();
#pragma unroll
                for (int j = 0; j < EW_MAX_PER; ++j) {
                    const int node = sub + j * ns;
                    if (active && j < per && node < n_here) {
                        const float y = tile[k * EW_LD + node];
                        const float d = pv[j] - y;
                        err += (double)d * (double)d;
                        nrm += (double)y * (double)y;
                    }
                }
                __syncthreads();          // the next chunk overwrites the tile
            }
        }

        part[0][tid] = err;
        part[1][tid] = nrm;
        __syncthreads();
        if (tid < tw) {
            double e = part[0][tid], n = part[1][tid];
            for (int j = 1; j < ns; ++j) {
                e += part[0][(j << a.kshift) + tid];
                n += part[1][(j << a.kshift) + tid];
            }
            const long o = (long)b * a.ld + c * tw + tid;
            a.err_out[o] = valid ? e : qnan;
            a.nrm_out[o] = valid ? n : qnan;
        }
        if (c == 0 && a.pos_out) {
            const int pn = min(max(p, tw), a.nt - tw) + tw;
            if (pn <= a.nt - tw) {
                const float t_next = a.t_axis[pn];
                float* po = a.pos_out + 2 * (long)b * nx;
                for (int i = tid; i < nx; i += EW_THREADS) po[2 * (long)i] = t_next;
            }
        }
        __syncthreads();          // the next work item overwrites the partials
    }
}

}  // namespace msmp

using namespace msmp;

extern "C" int msmp_eval_window_f32(const float* store, int64_t n_samples, int nt, int comps, int nx, const int32_t* sample_idx,
                                    const int32_t* steps, int batch, int tw, const float* pred, const float* t_axis, double* err_out,
                                    double* nrm_out, int64_t ld, float* pos_out, msmp_stream_t stream) {
    const char* who = "msmp_eval_window_f32";
    MSMP_REQUIRE(comps == 1 || comps == 2, MSMP_ERR_ARG, "%s: comps=%d is not 1 or 2", who, comps);
    MSMP_REQUIRE(batch >= 1 && nx >= 1 && nt >= 1 && n_samples >= 1 && n_samples < (1L << 31), MSMP_ERR_ARG,
                 "%s: bad sizes (batch=%d, nx=%d, nt=%d, n_samples=%lld outside 1 .. 2^31 - 1)", who, batch, nx, nt, (long long)n_samples);
    MSMP_REQUIRE((long)batch * nx < (1L << 31), MSMP_ERR_ARG, "%s: bad sizes (batch * nx = %lld nodes, 2^31 or more)", who,
                 (long long)batch * nx);
    MSMP_REQUIRE(store && sample_idx && steps && pred && err_out && nrm_out, MSMP_ERR_ARG, "%s: null pointer", who);
    MSMP_REQUIRE(t_axis || !pos_out, MSMP_ERR_ARG, "%s: null pointer (pos_out needs t_axis)", who);
    MSMP_REQUIRE(tw >= 1 && tw <= EW_MAX_TW, MSMP_ERR_UNSUPPORTED, "%s: time_window %d outside 1..%d", who, tw, EW_MAX_TW);
    MSMP_REQUIRE(nt >= 2 * tw, MSMP_ERR_UNSUPPORTED, "%s: nt=%d holds no window of 2 * time_window = %d steps", who, nt, 2 * tw);
    MSMP_REQUIRE(ld >= (int64_t)comps * tw, MSMP_ERR_ARG, "%s: ld=%lld is below comps * time_window = %d", who, (long long)ld, comps * tw);

    EvalWindowArgs a;
    a.store = store, a.sample_idx = sample_idx, a.steps = steps, a.pred = pred, a.t_axis = t_axis;
    a.err_out = err_out, a.nrm_out = nrm_out, a.pos_out = pos_out;
    a.n_samples = (long)n_samples, a.n_items = (long)batch * comps, a.ld = (long)ld;
    a.nt = nt, a.comps = comps, a.nx = nx, a.tw = tw;
    a.kshift = 0;
    while ((1 << a.kshift) < tw) ++a.kshift;
    const unsigned grid = (unsigned)(a.n_items < 65536 ? a.n_items : 65536);       // the rest by stride: an item's numbers do not depend on who takes it
    hipLaunchKernelGGL(eval_window_kernel, dim3(grid), dim3(EW_THREADS), 0, (hipStream_t)stream, a);
    return check_launch("eval_window_kernel");
}
