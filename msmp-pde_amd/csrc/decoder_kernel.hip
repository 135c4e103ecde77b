// Decoders of the solver classes, each fused into one pass: nothing but h (read) and out (write)
// touches memory.  1-D classes (experiments/models_gnn.py:210-224, 275-279):
//   diff = Conv1d(8 -> 1, k2)( Swish( Conv1d(1 -> 8, k1, stride s1)( h[:, None, :] ) ) )
//   out  = u[:, -1:] + cumsum(dt)[None, :] * diff
// ~7.7 kFMA per node: VALU work, ~3 GFLOP per E2-2048 batch; HBM traffic N*(512 + 4 + 100) bytes = 126 MB.  Weights are indexed
// with compile-time constants: the compiler keeps them in SGPRs (scalar loads).
// Both kernels give a node to EIGHT lanes, split by position: a lane that kept a whole row and both intermediate arrays in registers
// would need 256 VGPRs + 250 AGPRs, one wave per SIMD.
#include "decoder_geometry.h"      // DecSplit, the argument blocks (shared with decoder_bwd_kernel.hip)

namespace msmp {

// ----------------------------------------------------------------------------------------------
// Lane q (0..7) of a node computes the intermediate positions [q PP, (q + 1) PP) of all eight channels from a 26-28-value window of
// the row, the node's 8 x L1 intermediates meet in LDS (the node's [8][LP] table), and lane q then forms OPL consecutive outputs from
// a (OPL + K2 - 1)-value window per channel.  < 100 registers, three workgroups per CU.
// Summation order: every sum starts from its bias and adds its taps j = 0 .. k - 1 in ascending order with fmaf, one intermediate
// channel c = 0 .. 7 after the other into the output; cumsum(dt) is formed by repeated float32 addition like torch.cumsum on the device.
// decoder_split_node is lane q of node n (row: the node's 128 floats, of the last node for the lanes past the end, which are not
// `live` and write nothing; mrow: the node's table); of `a` it takes the weights, u, dt and out.
// ----------------------------------------------------------------------------------------------
template <int TW, int K1, int S1, int K2>
__device__ __forceinline__ void decoder_split_node(const float* row, float* mrow, int q, bool live, long n, const DecArgs& a) {
    using G = DecSplit<TW, K1, S1, K2>;
    constexpr int L1 = G::L1, PP = G::PP, XW = G::XW, OPL = G::OPL, MW4 = G::MW4, LP = G::LP;
    const int p0 = q * PP;
    float x[XW];
    {
        const int x0 = p0 * S1;
#pragma unroll
        for (int i = 0; i < XW; ++i) x[i] = row[x0 + i < H ? x0 + i : H - 1];
    }
#pragma unroll 1
    for (int c = 0; c < 8; ++c) {
        float w1c[K1];
#pragma unroll
        for (int j = 0; j < K1; ++j) w1c[j] = a.w1[c * K1 + j];
        const float bc = a.b1[c];
        float s[PP];
#pragma unroll
        for (int pp = 0; pp < PP; ++pp) s[pp] = bc;
#pragma unroll
        for (int j = 0; j < K1; ++j)
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) s[pp] = fmaf(w1c[j], x[pp * S1 + j], s[pp]);
#pragma unroll
        for (int pp = 0; pp < PP; ++pp)
            if (p0 + pp < L1) mrow[c * LP + p0 + pp] = swishf(s[pp]);
    }
    __syncthreads();        // every lane of a node's table has written before any reads
    // ---- outputs t0 .. t0 + OPL - 1 of this lane -------------------------------------------------------------------------
    const int t0 = q * OPL;
    float o[OPL];
    const float bias2 = a.b2[0];
#pragma unroll
    for (int i = 0; i < OPL; ++i) o[i] = bias2;
#pragma unroll 1
    for (int c = 0; c < 8; ++c) {
        float w2c[K2];
#pragma unroll
        for (int j = 0; j < K2; ++j) w2c[j] = a.w2[c * K2 + j];
        float m[4 * MW4];
#pragma unroll
        for (int i = 0; i < MW4; ++i) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(mrow + c * LP + t0 + 4 * i);
            m[4 * i] = v[0]; m[4 * i + 1] = v[1]; m[4 * i + 2] = v[2]; m[4 * i + 3] = v[3];
        }
#pragma unroll
        for (int j = 0; j < K2; ++j)
#pragma unroll
            for (int i = 0; i < OPL; ++i) o[i] = fmaf(w2c[j], m[i + j], o[i]);
    }
    if (!live || t0 >= TW) return;
    float* op = a.out + (size_t)n * TW;
    if (a.u == nullptr) {
#pragma unroll
        for (int i = 0; i < OPL; ++i)
            if (t0 + i < TW) op[t0 + i] = o[i];
        return;
    }
    const float ul = a.u[(size_t)n * TW + TW - 1];
    float tcum = 0.f;
    for (int t = 0; t < t0; ++t) tcum += a.dt;          // cumsum of a constant, float32 partial sums like torch.cumsum on the device
#pragma unroll
    for (int i = 0; i < OPL; ++i) {
        tcum += a.dt;
        if (t0 + i < TW) op[t0 + i] = ul + tcum * o[i];
    }
}

template <int TW, int K1, int S1, int K2>
__global__ __launch_bounds__(256) void decoder_split_kernel(DecArgs a) {
    using G = DecSplit<TW, K1, S1, K2>;
    constexpr int LP = G::LP, NODES = G::NODES;
    __shared__ __attribute__((aligned(16))) float mid[NODES * 8 * LP];
    const int q = threadIdx.x & 7, nl = threadIdx.x >> 3;
    const long n = (long)blockIdx.x * NODES + nl;
    const long nc = n < a.n_nodes ? n : a.n_nodes - 1;
    decoder_split_node<TW, K1, S1, K2>(a.h + (size_t)nc * H, mid + (size_t)nl * 8 * LP, q, n < a.n_nodes, n, a);
}

// ----------------------------------------------------------------------------------------------
// Decoder of the *2D solver classes (two solution components), experiments/models_gnn2D.py:79-88, 125-141:
//   diff = Conv1d(8 -> 2, k2)( Swish( Conv1d(2 -> 8, k1, stride s1)( hd ) ) ),   hd = double_mlp(h)  [N, 2, 128]
//   out  = unflatten(u) + cumsum(dt) * diff, flattened back to [N, 2*tw]
// Split by position like decoder_split_kernel: lane q builds the intermediate positions [q PP, (q + 1) PP) of all eight channels from
// windows of BOTH input rows, the node's 8 x L1 intermediates meet in LDS, lane q forms OPL consecutive outputs of both components.
// Summation order: an intermediate starts from its bias and adds the taps of input row 0, then of row 1, ascending; an output adds,
// per channel, its taps ascending from 0, then the eight channel sums as a tree (pairs, pairs of pairs, halves), then the bias.
// ----------------------------------------------------------------------------------------------
template <int TW, int K1, int S1, int K2>
__global__ __launch_bounds__(256) void decoder2d_split_kernel(Dec2Args a) {
    using G = DecSplit<TW, K1, S1, K2>;
    constexpr int L1 = G::L1, PP = G::PP, XW = G::XW, OPL = G::OPL, MW4 = G::MW4, LP = G::LP, NODES = G::NODES;
    __shared__ __attribute__((aligned(16))) float mid[NODES * 8 * LP];
    const int q = threadIdx.x & 7, nl = threadIdx.x >> 3;
    const long n = (long)blockIdx.x * NODES + nl;
    const long nc = n < a.n_nodes ? n : a.n_nodes - 1;
    const int p0 = q * PP;
    float x[2][XW];
#pragma unroll
    for (int ci = 0; ci < 2; ++ci) {
        const float* row = a.hd + ((size_t)nc * 2 + ci) * H;
        const int x0 = p0 * S1;
#pragma unroll
        for (int i = 0; i < XW; ++i) x[ci][i] = row[x0 + i < H ? x0 + i : H - 1];
    }
    float* mrow = mid + (size_t)nl * 8 * LP;
#pragma unroll 1
    for (int c = 0; c < 8; ++c) {
        const float bc = a.b1[c];
        float s[PP];
#pragma unroll
        for (int pp = 0; pp < PP; ++pp) s[pp] = bc;
#pragma unroll
        for (int ci = 0; ci < 2; ++ci) {
            float w[K1];
#pragma unroll
            for (int j = 0; j < K1; ++j) w[j] = a.w1[(c * 2 + ci) * K1 + j];
#pragma unroll
            for (int j = 0; j < K1; ++j)
#pragma unroll
                for (int pp = 0; pp < PP; ++pp) s[pp] = fmaf(w[j], x[ci][pp * S1 + j], s[pp]);
        }
#pragma unroll
        for (int pp = 0; pp < PP; ++pp)
            if (p0 + pp < L1) mrow[c * LP + p0 + pp] = swishf(s[pp]);
    }
    __syncthreads();
    const int t0 = q * OPL;
    float sc[2][8][OPL];          // per component and channel: the tap sums of this lane's outputs
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        float m[4 * MW4];
#pragma unroll
        for (int i = 0; i < MW4; ++i) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(mrow + c * LP + t0 + 4 * i);
            m[4 * i] = v[0]; m[4 * i + 1] = v[1]; m[4 * i + 2] = v[2]; m[4 * i + 3] = v[3];
        }
#pragma unroll
        for (int co = 0; co < 2; ++co) {
            float w[K2];
#pragma unroll
            for (int j = 0; j < K2; ++j) w[j] = a.w2[(co * 8 + c) * K2 + j];
#pragma unroll
            for (int i = 0; i < OPL; ++i) sc[co][c][i] = 0.f;
#pragma unroll
            for (int j = 0; j < K2; ++j)
#pragma unroll
                for (int i = 0; i < OPL; ++i) sc[co][c][i] = fmaf(w[j], m[i + j], sc[co][c][i]);
        }
    }
    if (n >= a.n_nodes || t0 >= TW) return;
    const float b2v[2] = {a.b2[0], a.b2[1]};
    float tcum = 0.f;
    for (int t = 0; t < t0; ++t) tcum += a.dt;
#pragma unroll
    for (int i = 0; i < OPL; ++i) {
        tcum += a.dt;
        if (t0 + i < TW) {
#pragma unroll
            for (int co = 0; co < 2; ++co) {
                // the eight channel sums as a tree: pairs, pairs of pairs, halves
                const float s01 = sc[co][0][i] + sc[co][1][i], s23 = sc[co][2][i] + sc[co][3][i];
                const float s45 = sc[co][4][i] + sc[co][5][i], s67 = sc[co][6][i] + sc[co][7][i];
                const float v = (s01 + s23) + (s45 + s67);
                const size_t o = (size_t)n * 2 * TW + co * TW + t0 + i;
                a.out[o] = a.u[o] + tcum * (v + b2v[co]);
            }
        }
    }
}

// ----------------------------------------------------------------------------------------------
// Gated CNN decoder of the GLU classes (hidden width 164): two networks of the same geometry, `gate` on the first 82 values of a row and
// `diff` on the last 82,  Conv1d(C -> 8, 6, stride 2) -> Swish -> Conv1d(8 -> C, 15)  each (L1 = 39 intermediate positions, 25 outputs):
//   1-D (C = 1, experiments/models_gnn.py:1455-1456, 1514-1521):   out = (1 - scale) u[:, -1:] + cumsum(dt) (scale diff)
//   2-D (C = 2, models_gnn2D.py:1291-1298, 1355-1366; rows of hd = double_mlp(h), component stride 164):
//                                                                  out = (1 - scale) u + (cumsum(dt) scale) diff,  every column of u
// with scale = gate(row[:82]), diff = diff(row[82:]); no sigmoid on scale, as in the reference.
// Split like decoder_split_kernel: eight lanes per node, lane q builds the intermediate positions [q PP, (q + 1) PP) of all eight channels,
// the node's 8 x L1 intermediates meet in the node's LDS table, lane q then forms OPL consecutive outputs of every component.  The two
// networks run one after the other through the SAME table (a barrier after the reads of `gate` frees it for `diff`) and the lane keeps
// the C x OPL outputs of `gate` in registers meanwhile: LDS, and with it the workgroups per CU, stay those of the one-network decoders, and
// a network's 14-value windows (28 in 2-D) are dead before the other's are loaded.  The outputs are formed two intermediate channels at a
// time: with all eight unrolled at once the compiler took 184 / 230 vector registers (1-D / 2-D), in pairs 73 / 115.
// Rows are read with a caller-given stride `ld` as single floats: the second half of a row starts 328 bytes in, 8-byte aligned only.
// Summation order (plain fp32 fmaf, no fp16 split: the range status word is not touched): an intermediate starts from its bias and adds the
// taps of input component 0, then of component 1, ascending; an output adds, per intermediate channel, its taps ascending from 0, then the
// eight channel sums as a tree (pairs, pairs of pairs, halves), then the bias; cumsum(dt) is formed by repeated float32 addition.
// ----------------------------------------------------------------------------------------------
// One network of lane q: o[co][i] = output t0 + i of component co.  row: the node's (clamped) row, already offset to the network's half;
// component ci starts ci * CS floats further.  Ends with a barrier: the table may be written again.
template <class G, int C, int CS, int R, int K1, int S1, int K2>
__device__ __forceinline__ void decoder_gated_net(const float* row, float* mrow, int q, const DecNet& w, float (&o)[C][G::OPL]) {
    constexpr int L1 = G::L1, PP = G::PP, XW = G::XW, OPL = G::OPL, MW4 = G::MW4, LP = G::LP;
    const int p0 = q * PP;
    float x[C][XW];
#pragma unroll
    for (int ci = 0; ci < C; ++ci) {
        const int x0 = p0 * S1;
#pragma unroll
        for (int i = 0; i < XW; ++i) x[ci][i] = row[ci * CS + (x0 + i < R ? x0 + i : R - 1)];
    }
#pragma unroll 1
    for (int c = 0; c < 8; ++c) {
        const float bc = w.b1[c];
        float s[PP];
#pragma unroll
        for (int pp = 0; pp < PP; ++pp) s[pp] = bc;
#pragma unroll
        for (int ci = 0; ci < C; ++ci) {
            float wt[K1];
#pragma unroll
            for (int j = 0; j < K1; ++j) wt[j] = w.w1[(c * C + ci) * K1 + j];
#pragma unroll
            for (int j = 0; j < K1; ++j)
#pragma unroll
                for (int pp = 0; pp < PP; ++pp) s[pp] = fmaf(wt[j], x[ci][pp * S1 + j], s[pp]);
        }
#pragma unroll
        for (int pp = 0; pp < PP; ++pp)
            if (p0 + pp < L1) mrow[c * LP + p0 + pp] = swishf(s[pp]);
    }
    __syncthreads();        // every lane of a node's table has written before any reads
    const int t0 = q * OPL;
    float half[C][OPL], tot[C][OPL];
#pragma unroll 1
    for (int cp = 0; cp < 4; ++cp) {          // channel pairs one after the other: two channels' windows live at a time
        float sc[C][2][OPL];                  // per component and channel of the pair: the tap sums of this lane's outputs
#pragma unroll
        for (int cc = 0; cc < 2; ++cc) {
            const int c = 2 * cp + cc;
            float m[4 * MW4];
#pragma unroll
            for (int i = 0; i < MW4; ++i) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(mrow + c * LP + t0 + 4 * i);
                m[4 * i] = v[0]; m[4 * i + 1] = v[1]; m[4 * i + 2] = v[2]; m[4 * i + 3] = v[3];
            }
#pragma unroll
            for (int co = 0; co < C; ++co) {
                float wt[K2];
#pragma unroll
                for (int j = 0; j < K2; ++j) wt[j] = w.w2[(co * 8 + c) * K2 + j];
#pragma unroll
                for (int i = 0; i < OPL; ++i) sc[co][cc][i] = 0.f;
#pragma unroll
                for (int j = 0; j < K2; ++j)
#pragma unroll
                    for (int i = 0; i < OPL; ++i) sc[co][cc][i] = fmaf(wt[j], m[i + j], sc[co][cc][i]);
            }
        }
        // the eight channel sums as a tree: pairs, pairs of pairs, halves
#pragma unroll
        for (int co = 0; co < C; ++co)
#pragma unroll
            for (int i = 0; i < OPL; ++i) {
                const float pair = sc[co][0][i] + sc[co][1][i];
                if (cp & 1) {
                    const float quad = half[co][i] + pair;
                    tot[co][i] = cp == 1 ? quad : tot[co][i] + quad;
                } else {
                    half[co][i] = pair;
                }
            }
    }
#pragma unroll
    for (int co = 0; co < C; ++co) {
        const float b2v = w.b2[co];
#pragma unroll
        for (int i = 0; i < OPL; ++i) o[co][i] = tot[co][i] + b2v;
    }
    __syncthreads();        // every lane has read the table before the next network writes it
}

// C = 1: decoder_gated_kernel (rows of h), C = 2: decoder2d_gated_kernel (rows of hd)
template <int C, int W, int TW, int K1, int S1, int K2>
__device__ __forceinline__ void decoder_gated_body(const DecGatedArgs& a, float* mid) {
    constexpr int R = W / 2;
    using G = DecSplit<TW, K1, S1, K2, R>;
    constexpr int OPL = G::OPL, LP = G::LP, NODES = G::NODES;
    const int q = threadIdx.x & 7, nl = threadIdx.x >> 3;
    const long n = (long)blockIdx.x * NODES + nl;
    const long nc = n < a.n_nodes ? n : a.n_nodes - 1;          // lanes past the end: a valid row, nothing stored
    const float* row = a.h + (size_t)nc * (size_t)a.ld;
    float* mrow = mid + (size_t)nl * 8 * LP;
    float scale[C][OPL], diff[C][OPL];
#pragma unroll 1
    for (int net = 0; net < 2; ++net) {                         // gate, then diff, through the same table
        const DecNet w{net ? a.diff.w1 : a.gate.w1, net ? a.diff.b1 : a.gate.b1, net ? a.diff.w2 : a.gate.w2, net ? a.diff.b2 : a.gate.b2};
        decoder_gated_net<G, C, W, R, K1, S1, K2>(row + net * R, mrow, q, w, diff);
        if (net == 0) {
#pragma unroll
            for (int co = 0; co < C; ++co)
#pragma unroll
                for (int i = 0; i < OPL; ++i) scale[co][i] = diff[co][i];
        }
    }
    const int t0 = q * OPL;
    if (n >= a.n_nodes || t0 >= TW) return;
    float tcum = 0.f;
    for (int t = 0; t < t0; ++t) tcum += a.dt;          // cumsum of a constant, float32 partial sums like torch.cumsum on the device
    const float* up = a.u + (size_t)n * C * TW;
    float* op = a.out + (size_t)n * C * TW;
    const float ul = C == 1 ? up[TW - 1] : 0.f;
#pragma unroll
    for (int i = 0; i < OPL; ++i) {
        tcum += a.dt;
        if (t0 + i < TW) {
            if (C == 1) {
                op[t0 + i] = (1.0f - scale[0][i]) * ul + tcum * (scale[0][i] * diff[0][i]);
            } else {
#pragma unroll
                for (int co = 0; co < C; ++co) {
                    const int k = co * TW + t0 + i;
                    op[k] = (1.0f - scale[co][i]) * up[k] + (tcum * scale[co][i]) * diff[co][i];
                }
            }
        }
    }
}

template <int W, int TW, int K1, int S1, int K2>
__global__ __launch_bounds__(256) void decoder_gated_kernel(DecGatedArgs a) {
    using G = DecSplit<TW, K1, S1, K2, W / 2>;
    __shared__ __attribute__((aligned(16))) float mid[G::NODES * 8 * G::LP];
    decoder_gated_body<1, W, TW, K1, S1, K2>(a, mid);
}

template <int W, int TW, int K1, int S1, int K2>
__global__ __launch_bounds__(256) void decoder2d_gated_kernel(DecGatedArgs a) {
    using G = DecSplit<TW, K1, S1, K2, W / 2>;
    __shared__ __attribute__((aligned(16))) float mid[G::NODES * 8 * G::LP];
    decoder_gated_body<2, W, TW, K1, S1, K2>(a, mid);
}

}  // namespace msmp

using namespace msmp;

// One launcher per kernel.  `timed`: the inference entries, inside the event bracket of the DECODER family; the forward-for-training
// entries (msmp_*_train_fwd_f32: the forward half of the decoder under autograd, whose backward is decoder_bwd_kernel.hip) launch the SAME
// kernels outside it, so the family keeps counting the launches of no-grad forwards only.
#define MSMP_DEC_SPLIT(KERNEL, TW_, K1_, S1_, K2_) do { using G_ = DecSplit<TW_, K1_, S1_, K2_>; \
        hipLaunchKernelGGL((KERNEL<TW_, K1_, S1_, K2_>), dim3((unsigned)((n_nodes + G_::NODES - 1) / G_::NODES)), dim3(G_::NODES * 8), 0, st, a); } while (0)

static int decoder2d(const char* who, bool timed, const float* hd, const float* u, int64_t n_nodes, int tw, const float* w1, const float* b1,
                     const float* w2, const float* b2, float dt, float* out, msmp_stream_t stream) {
    MSMP_REQUIRE(hd && u && w1 && b1 && w2 && b2 && out, MSMP_ERR_ARG, "%s: null pointer", who);
    MSMP_REQUIRE(n_nodes > 0 && n_nodes < (1L << 31), MSMP_ERR_ARG, "%s: bad n_nodes", who);
    Dec2Args a{hd, u, (long)n_nodes, w1, b1, w2, b2, dt, out};
    hipStream_t st = (hipStream_t)stream;
    if (timed) timing_begin(MSMP_K_DECODER, st);
    switch (tw) {   // experiments/models_gnn2D.py:79-88
        case 25: MSMP_DEC_SPLIT(decoder2d_split_kernel, 25, 16, 3, 14); break;
        case 50: MSMP_DEC_SPLIT(decoder2d_split_kernel, 50, 12, 2, 10); break;
        default:
            set_error("%s: time_window %d (the reference defines 25, 50)", who, tw);
            return MSMP_ERR_UNSUPPORTED;
    }
    if (timed) timing_end(MSMP_K_DECODER, st);
    return check_launch("decoder2d_split_kernel");
}

static int decoder1d(const char* who, bool timed, const float* h, const float* u, int64_t n_nodes, int tw, const float* w1, const float* b1,
                     const float* w2, const float* b2, float dt, float* out, msmp_stream_t stream) {
    MSMP_REQUIRE(h && w1 && b1 && w2 && b2 && out, MSMP_ERR_ARG, "%s: null pointer", who);
    MSMP_REQUIRE(n_nodes > 0 && n_nodes < (1L << 31), MSMP_ERR_ARG, "%s: bad n_nodes", who);
    DecArgs a{h, u, (long)n_nodes, w1, b1, w2, b2, dt, out};
    hipStream_t st = (hipStream_t)stream;
    if (timed) timing_begin(MSMP_K_DECODER, st);
    switch (tw) {   // experiments/models_gnn.py:210-224
        case 20: MSMP_DEC_SPLIT(decoder_split_kernel, 20, 15, 4, 10); break;
        case 25: MSMP_DEC_SPLIT(decoder_split_kernel, 25, 16, 3, 14); break;
        case 50: MSMP_DEC_SPLIT(decoder_split_kernel, 50, 12, 2, 10); break;
        default:
            set_error("%s: time_window %d (the reference defines 20, 25, 50)", who, tw);
            return MSMP_ERR_UNSUPPORTED;
    }
    if (timed) timing_end(MSMP_K_DECODER, st);
    return check_launch("decoder_split_kernel");
}
#undef MSMP_DEC_SPLIT

extern "C" int msmp_decoder2d_f32(const float* hd, const float* u, int64_t n_nodes, int tw, const float* w1, const float* b1,
                                  const float* w2, const float* b2, float dt, float* out, msmp_stream_t stream) {
    return decoder2d("msmp_decoder2d_f32", true, hd, u, n_nodes, tw, w1, b1, w2, b2, dt, out, stream);
}

extern "C" int msmp_decoder2d_train_fwd_f32(const float* hd, const float* u, int64_t n_nodes, int tw, const float* w1, const float* b1,
                                            const float* w2, const float* b2, float dt, float* out, msmp_stream_t stream) {
    return decoder2d("msmp_decoder2d_train_fwd_f32", false, hd, u, n_nodes, tw, w1, b1, w2, b2, dt, out, stream);
}

extern "C" int msmp_decoder_f32(const float* h, const float* u, int64_t n_nodes, int tw, const float* w1, const float* b1,
                                const float* w2, const float* b2, float dt, float* out, msmp_stream_t stream) {
    return decoder1d("msmp_decoder_f32", true, h, u, n_nodes, tw, w1, b1, w2, b2, dt, out, stream);
}

extern "C" int msmp_decoder_train_fwd_f32(const float* h, const float* u, int64_t n_nodes, int tw, const float* w1, const float* b1,
                                          const float* w2, const float* b2, float dt, float* out, msmp_stream_t stream) {
    return decoder1d("msmp_decoder_train_fwd_f32", false, h, u, n_nodes, tw, w1, b1, w2, b2, dt, out, stream);
}

// The gated decoders exist for the one geometry the reference defines (hidden width 164, time_window 25): anything else is refused by
// value before a launch, and the host keeps its PyTorch ops.  msmp_tune("wide_dec", ...) is read by the host only.
static int decoder_gated(const char* who, bool two_d, bool timed, const float* h, int ld, const float* u, int64_t n_nodes, int width, int tw,
                         const DecNet& gate, const DecNet& diff, float dt, float* out, msmp_stream_t stream) {
    MSMP_REQUIRE(h && u && out && gate.w1 && gate.b1 && gate.w2 && gate.b2 && diff.w1 && diff.b1 && diff.w2 && diff.b2, MSMP_ERR_ARG,
                 "%s: null pointer", who);
    MSMP_REQUIRE(n_nodes > 0 && n_nodes < (1L << 31), MSMP_ERR_ARG, "%s: bad n_nodes", who);
    MSMP_REQUIRE(width == 164 && tw == 25, MSMP_ERR_UNSUPPORTED, "%s: width %d, time_window %d (the reference defines 164, 25)", who, width, tw);
    const int comps = two_d ? 2 : 1;
    MSMP_REQUIRE(ld >= comps * width, MSMP_ERR_ARG, "%s: row stride ld = %d < %d", who, ld, comps * width);
    DecGatedArgs a{h, (long)ld, u, (long)n_nodes, gate, diff, dt, out};
    using G = DecSplit<25, 6, 2, 15, 82>;
    const dim3 grid((unsigned)((n_nodes + G::NODES - 1) / G::NODES)), block(G::NODES * 8);
    hipStream_t st = (hipStream_t)stream;
    if (timed) timing_begin(MSMP_K_DECODER, st);
    if (two_d) hipLaunchKernelGGL((decoder2d_gated_kernel<164, 25, 6, 2, 15>), grid, block, 0, st, a);      // models_gnn2D.py:1291-1298
    else hipLaunchKernelGGL((decoder_gated_kernel<164, 25, 6, 2, 15>), grid, block, 0, st, a);              // models_gnn.py:1455-1456
    if (timed) timing_end(MSMP_K_DECODER, st);
    return check_launch(two_d ? "decoder2d_gated_kernel" : "decoder_gated_kernel");
}

#define MSMP_DEC_GATED_ENTRY(NAME, TWO_D, TIMED)                                                                                              \
    extern "C" int NAME(const float* h, int ld, const float* u, int64_t n_nodes, int width, int tw, const float* gate_w1, const float* gate_b1, \
                        const float* gate_w2, const float* gate_b2, const float* diff_w1, const float* diff_b1, const float* diff_w2,           \
                        const float* diff_b2, float dt, float* out, msmp_stream_t stream) {                                                     \
        return decoder_gated(#NAME, TWO_D, TIMED, h, ld, u, n_nodes, width, tw, DecNet{gate_w1, gate_b1, gate_w2, gate_b2},                     \
                             DecNet{diff_w1, diff_b1, diff_w2, diff_b2}, dt, out, stream);                                                      \
    }
MSMP_DEC_GATED_ENTRY(msmp_decoder_gated_f32, false, true)
MSMP_DEC_GATED_ENTRY(msmp_decoder2d_gated_f32, true, true)
MSMP_DEC_GATED_ENTRY(msmp_decoder_gated_train_fwd_f32, false, false)
MSMP_DEC_GATED_ENTRY(msmp_decoder2d_gated_train_fwd_f32, true, false)
#undef MSMP_DEC_GATED_ENTRY

