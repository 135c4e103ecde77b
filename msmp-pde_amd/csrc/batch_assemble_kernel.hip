// Batch assembly from a device-resident dataset: what GraphCreator.create_data + create_graph (common/utils.py:300-428) and
// create_next_graph (:431-471) make of a [B, nt, (2,) nx] block of trajectories -- the window gather, the two component-major
// flattenings of GraphCreator._flatten (:350-357), the (t, x) position rows and the repeated equation-parameter columns -- as ONE launch
// that reads the sample and step indices on the device.  For graph b with s = sample_idx[b], p = steps[b]:
//
//   x_out[b nx + i, c tw + k] = store[s, p - tw + k, c, i]         y_out[b nx + i, c tw + k] = store[s, p + k, c, i]
//   pos_out[b nx + i]         = (t_axis[p], x_grid[i])             vars_out[v B nx + b nx + i] = var_table[s, v]
//
// It is a transposition [2 tw, nx] -> [nx, tw] per (graph, component) and nothing else, so it is bound by HBM.  One work item is a
// (graph, component, 64-node chunk): its 2 tw x 64 window goes through LDS, read from `store` as 256-byte row segments (one wave per
// time row, lane = node), written out with the transposed index: consecutive threads walk k within a node and then the next node, so a
// chunk's [64, tw] block of x_out is one contiguous span with comps = 1 and 64 spans of tw floats with comps = 2.  The LDS row stride is
// 65 floats: the transposed read steps 65 words from lane to lane, one bank each.  256 threads take work items in a grid-stride loop.
// pos and vars are written by the first component's work item of a chunk.
//
// The indices cannot be checked by the host.  A graph whose s is outside 0 .. n_samples - 1 or whose p is outside tw .. nt - tw reads
// nothing from `store`: its rows of x_out / y_out are quiet NaNs (the loss of such a batch is NaN, which optim.AdamW(skip_nonfinite)
// skips), its pos / vars rows come from the clamped p and s, and the other graphs of the batch are what they would have been.
// No allocation, no synchronisation, no atomic, no memset: the launch holds pointers and sizes only and can be captured.
#include "msmp_common.h"

namespace msmp {

constexpr int BA_THREADS = 256;
constexpr int BA_NODES = 64;              // nodes per work item: one 256-byte row segment per wave load
constexpr int BA_MAX_TW = 64;
constexpr int BA_LD = BA_NODES + 1;       // odd LDS row stride

struct BatchAssembleArgs {
    const float* store;
    const int32_t* sample_idx;
    const int32_t* steps;
    const float* t_axis;
    const float* x_grid;
    const float* var_table;
    float* x_out;
    float* y_out;
    float* pos_out;
    float* vars_out;
    long n_samples;
    long n_items;        // batch * comps * chunks
    int nt, comps, nx, batch, tw, n_vars, chunks;
};

// MODE 0: create_data + create_graph.  MODE 1: create_next_graph (labels and pos[:, 0] only).
template <int MODE>
__global__ __launch_bounds__(BA_THREADS) void batch_assemble_kernel(const BatchAssembleArgs a) {
    __shared__ float tile[2 * BA_MAX_TW * BA_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tw = a.tw, nx = a.nx, comps = a.comps;
    const int rows = MODE == 0 ? 2 * tw : tw;                 // time rows staged: [p - tw, p + tw) or [p, p + tw)
    const int dn = BA_THREADS / tw, dk = BA_THREADS % tw;     // one stride of the flat output index as (nodes, steps)
    const float qnan = __builtin_nanf("");

    for (long item = blockIdx.x; item < a.n_items; item += gridDim.x) {
        const int chunk = (int)(item % a.chunks);
        const long bc = item / a.chunks;
        const int c = (int)(bc % comps);
        const int b = (int)(bc / comps);
        const int i0 = chunk * BA_NODES;
        const int n_here = min(BA_NODES, nx - i0);
        const int s = a.sample_idx[b], p = a.steps[b];
        const bool valid = s >= 0 && (long)s < a.n_samples && p >= tw && p <= a.nt - tw;

        if (valid && lane < n_here) {
            const int t0 = MODE == 0 ? p - tw : p;
            const float* src = a.store + (((long)s * a.nt + t0) * comps + c) * nx + i0 + lane;
            const long row_stride = (long)comps * nx;
            // eight row segments in flight per wave (measured no different from four: at these sizes a work item is a chain of three
            // dependent round trips -- indices, window, store -- and the launch is bound by that latency)
#pragma unroll 8
            for (int r = wave; r < rows; r += BA_THREADS / 64) tile[r * BA_LD + lane] = src[r * row_stride];
        }
        __syncthreads();

        const long node0 = (long)b * nx + i0;
        const long ld_out = (long)comps * tw;
        float* xo = MODE == 0 ? a.x_out + node0 * ld_out + c * tw : nullptr;
        float* yo = a.y_out + node0 * ld_out + c * tw;
        const int y_row0 = MODE == 0 ? tw : 0;
        int node = tid / tw, k = tid % tw;
        while (node < n_here) {
            const long o = node * ld_out + k;
            if (MODE == 0) xo[o] = valid ? tile[k * BA_LD + node] : qnan;
            yo[o] = valid ? tile[(y_row0 + k) * BA_LD + node] : qnan;
            node += dn;
            k += dk;
            if (k >= tw) {
                k -= tw;
                ++node;
            }
        }

        if (c == 0 && tid < n_here) {
            const int pc = min(max(p, tw), a.nt - tw);
            const long n = node0 + tid;
            a.pos_out[2 * n] = a.t_axis[pc];
            if (MODE == 0) {
                a.pos_out[2 * n + 1] = a.x_grid[i0 + tid];
                const long sc = min(max((long)s, 0L), a.n_samples - 1);
                const long col = (long)a.batch * nx;
                for (int v = 0; v < a.n_vars; ++v) a.vars_out[v * col + n] = a.var_table[sc * a.n_vars + v];
            }
        }
        __syncthreads();          // the next work item overwrites the tile
    }
}

}  // namespace msmp

using namespace msmp;

extern "C" int msmp_batch_assemble_f32(const float* store, int64_t n_samples, int nt, int comps, int nx, const int32_t* sample_idx,
                                       const int32_t* steps, int batch, int tw, const float* t_axis, const float* x_grid,
                                       const float* var_table, int n_vars, int mode, float* x_out, float* y_out, float* pos_out,
                                       float* vars_out, msmp_stream_t stream) {
    const char* who = "msmp_batch_assemble_f32";
    MSMP_REQUIRE(mode == 0 || mode == 1, MSMP_ERR_ARG, "%s: mode=%d is not 0 (create_graph) or 1 (create_next_graph)", who, mode);
    MSMP_REQUIRE(comps == 1 || comps == 2, MSMP_ERR_ARG, "%s: comps=%d is not 1 or 2", who, comps);
    MSMP_REQUIRE(n_vars >= 0 && n_vars <= 3, MSMP_ERR_ARG, "%s: n_vars=%d outside 0..3", who, n_vars);
    MSMP_REQUIRE(batch >= 1 && nx >= 1 && nt >= 1 && n_samples >= 1 && n_samples < (1L << 31), MSMP_ERR_ARG,
                 "%s: bad sizes (batch=%d, nx=%d, nt=%d, n_samples=%lld outside 1 .. 2^31 - 1)", who, batch, nx, nt, (long long)n_samples);
    MSMP_REQUIRE((long)batch * nx < (1L << 31), MSMP_ERR_ARG, "%s: bad sizes (batch * nx = %lld nodes, 2^31 or more)", who,
                 (long long)batch * nx);
    MSMP_REQUIRE(store && sample_idx && steps && t_axis && y_out && pos_out, MSMP_ERR_ARG, "%s: null pointer", who);
    if (mode == 0) {
        MSMP_REQUIRE(x_grid && x_out, MSMP_ERR_ARG, "%s: null pointer (mode 0 needs x_grid and x_out)", who);
        MSMP_REQUIRE(n_vars == 0 || (var_table && vars_out), MSMP_ERR_ARG, "%s: null pointer (n_vars=%d needs var_table and vars_out)", who,
                     n_vars);
    }
    MSMP_REQUIRE(tw >= 1 && tw <= BA_MAX_TW, MSMP_ERR_UNSUPPORTED, "%s: time_window %d outside 1..%d", who, tw, BA_MAX_TW);
    MSMP_REQUIRE(nt >= 2 * tw, MSMP_ERR_UNSUPPORTED, "%s: nt=%d holds no window of 2 * time_window = %d steps", who, nt, 2 * tw);

    BatchAssembleArgs a;
    a.store = store, a.sample_idx = sample_idx, a.steps = steps, a.t_axis = t_axis, a.x_grid = x_grid, a.var_table = var_table;
    a.x_out = x_out, a.y_out = y_out, a.pos_out = pos_out, a.vars_out = vars_out;
    a.n_samples = (long)n_samples;
    a.nt = nt, a.comps = comps, a.nx = nx, a.batch = batch, a.tw = tw, a.n_vars = mode == 0 ? n_vars : 0;
    a.chunks = (nx + BA_NODES - 1) / BA_NODES;
    a.n_items = (long)batch * comps * a.chunks;
    const unsigned grid = (unsigned)(a.n_items < 8192 ? a.n_items : 8192);       // 256 CUs x 4 resident tiles x 8; the rest by stride
    if (mode == 0)
        hipLaunchKernelGGL(batch_assemble_kernel<0>, dim3(grid), dim3(BA_THREADS), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(batch_assemble_kernel<1>, dim3(grid), dim3(BA_THREADS), 0, (hipStream_t)stream, a);
    return check_launch("batch_assemble_kernel");
}
