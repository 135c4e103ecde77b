// Backward of the decoders of decoder_kernel.hip, each as ONE launch plus a fixed-order sum of the parameter partials: for a network
//   O = Conv1d(8 -> C, K2)( m ),  m = Swish(s),  s = Conv1d(C -> 8, K1, stride S1)( x )           (x: C rows of R values of a node)
// and dO, the gradient of its output,
//   dW2[co][c][j] = sum_n sum_t dO[n,co,t] m[n,c,t+j]        db2 = sum dO        dm[n,c,p] = sum_co sum_j w2[co][c][j] dO[n,co,p-j]
//   ds = dm Swish'(s)       dW1[c][ci][j] = sum_n sum_p ds[n,c,p] x[n,ci,p S1+j]  db1 = sum ds
//   dh[n,ci,i] = sum_c sum_{p S1+j=i} w1[c][ci][j] ds[n,c,p]
// dO from grad_out g and c_t = cumsum(dt) (repeated float32 addition, as in the forward):
//   one network:  dO = g c_t with the Euler update, dO = g without (RETURN_DIFF)
//   gated:        d scale = g (c_t diff - u*),  d diff = g c_t scale;  u* = u[:, -1] in 1-D, u[:, co tw + t] in 2-D
// Nothing is saved by the forward: the Swish pre-activations are recomputed from the row (the gated backward recomputes both networks'
// outputs first).  No gradient for u or dt.  Plain fp32 fmaf: the range status word is not touched.
//
// Shape: the forward's.  A workgroup takes DEC_BWD_NODES = 16 nodes, eight lanes each, split by position (lane q: the intermediate
// positions [q PP, (q + 1) PP) of all eight channels), the node's 8 x LP table in LDS.  Phases of a network through that table:
//   A  m into the table (the rows and dO are staged in LDS beside it)
//   B  dW2 / db2: a thread owns parameter entries e = tid, tid + 128, .. and sums over the workgroup's nodes and positions
//   C  the lanes recompute s channel by channel, form dm from their dO window and overwrite the table with ds
//   D  dW1 / db1 like B;  dh: lane q the row positions q, q + 8, ..
// A thread keeps at most three entries per phase in registers over the grid-stride loop and writes them once, to the workgroup's own
// row of the workspace: no atomics, no memset.  decoder_bwd_sum_kernel then adds the (at most DEC_BWD_GRID_CAP) rows, a wave per
// entry: lane l rows l, l + 64, .. ascending, then a butterfly.  Same bits on every call; dh of a node depends on that node's row,
// its g row and the weights only (fixed summation order: channels ascending, taps ascending).
// LDS: 16 x (table 8 LP + 4 | row | dO) floats: 32 KB (1-D, tw 20 / 25) .. 67 KB (2-D, tw 50), two to five workgroups per CU.
#include "decoder_geometry.h"

namespace msmp {

constexpr int DBT = DEC_BWD_NODES * 8;          // threads per workgroup

// C components, NETS networks side by side in a component's CS = NETS R values; MODE 0: dO = g, 1: Euler, 2: gated (NETS == 2)
template <int C_, int R_, int NETS_, int TW_, int K1_, int S1_, int K2_, int MODE_>
struct DecBwd {
    static constexpr int C = C_, R = R_, NETS = NETS_, TW = TW_, K1 = K1_, S1 = S1_, K2 = K2_, MODE = MODE_;
    using G = DecSplit<TW, K1, S1, K2, R>;
    static constexpr int L1 = G::L1, PP = G::PP, XW = G::XW, OPL = G::OPL, LP = G::LP;
    static constexpr int CS = NETS * R;                 // component stride of a row
    static constexpr int RW = C * CS;                   // row floats (also the compact dh row)
    static constexpr int NS = 8 * LP + 4;               // table stride of a node: + 4 floats, so that the eight nodes of a wave start in different banks
    static constexpr int PADF = K2 - 1;                 // zeros in front of a staged dO row: dm's taps need no bounds
    static constexpr int DOL = PADF + 8 * PP;           // staged dO row
    static constexpr int DW = PP + K2 - 1;              // dO window of a lane
    static constexpr int NW1 = 8 * C * K1, E6 = NW1 + 8;        // phase D entries: dW1 | db1
    static constexpr int NW2 = C * 8 * K2, E4 = NW2 + C;        // phase B entries: dW2 | db2
    static constexpr int NET_E = E6 + E4;               // a network's part of a partial row: [dW1 | db1 | dW2 | db2]
    static constexpr int ROW = NETS * NET_E;
    static constexpr int EPT4 = (E4 + DBT - 1) / DBT, EPT6 = (E6 + DBT - 1) / DBT;
    static constexpr int NJ = (K1 + S1 - 1) / S1;       // taps that can reach one row position
    static constexpr int LDS_FLOATS = DEC_BWD_NODES * (NS + RW + C * DOL) + NETS * NW1;
    static_assert(NET_E == dec_bwd_net_entries(C, K1, K2), "partial row");
    static_assert(MODE != 2 || NETS == 2, "gated: two networks");
};

template <class T>
__device__ __forceinline__ void dec_bwd_load_x(const float* row, int q, float (&x)[T::C][T::XW]) {
    const int x0 = q * T::PP * T::S1;
#pragma unroll
    for (int ci = 0; ci < T::C; ++ci)
#pragma unroll
        for (int i = 0; i < T::XW; ++i) x[ci][i] = row[ci * T::CS + (x0 + i < T::R ? x0 + i : T::R - 1)];
}

// pre-activations of channel c at this lane's positions: bias, then the taps of component 0, then of component 1, ascending (the forward's order)
template <class T>
__device__ __forceinline__ void dec_bwd_conv1(const float (&x)[T::C][T::XW], const DecNet& w, int c, float (&s)[T::PP]) {
    const float bc = w.b1[c];
#pragma unroll
    for (int pp = 0; pp < T::PP; ++pp) s[pp] = bc;
#pragma unroll
    for (int ci = 0; ci < T::C; ++ci) {
        float wt[T::K1];
#pragma unroll
        for (int j = 0; j < T::K1; ++j) wt[j] = w.w1[(c * T::C + ci) * T::K1 + j];
#pragma unroll
        for (int j = 0; j < T::K1; ++j)
#pragma unroll
            for (int pp = 0; pp < T::PP; ++pp) s[pp] = fmaf(wt[j], x[ci][pp * T::S1 + j], s[pp]);
    }
}

// phase A: m = Swish(s) of this lane's positions into the node's table
template <class T>
__device__ __forceinline__ void dec_bwd_phase_a(const float (&x)[T::C][T::XW], const DecNet& w, float* mrow, int q) {
    const int p0 = q * T::PP;
#pragma unroll 1
    for (int c = 0; c < 8; ++c) {
        float s[T::PP];
        dec_bwd_conv1<T>(x, w, c, s);
#pragma unroll
        for (int pp = 0; pp < T::PP; ++pp)
            if (p0 + pp < T::L1) mrow[c * T::LP + p0 + pp] = swishf(s[pp]);
    }
}

// outputs t0 .. t0 + OPL - 1 of every component from the node's table (gated: the networks' outputs enter each other's gradient)
template <class T>
__device__ __forceinline__ void dec_bwd_outputs(const float* mrow, const DecNet& w, int q, float (&o)[T::C][T::OPL]) {
    const int t0 = q * T::OPL;
#pragma unroll
    for (int co = 0; co < T::C; ++co) {
        const float b = w.b2[co];
#pragma unroll
        for (int i = 0; i < T::OPL; ++i) o[co][i] = b;
    }
#pragma unroll 1
    for (int c = 0; c < 8; ++c) {
        float m[T::OPL + T::K2 - 1];
#pragma unroll
        for (int i = 0; i < T::OPL + T::K2 - 1; ++i) m[i] = mrow[c * T::LP + t0 + i];
#pragma unroll
        for (int co = 0; co < T::C; ++co)
#pragma unroll
            for (int j = 0; j < T::K2; ++j) {
                const float wv = w.w2[(co * 8 + c) * T::K2 + j];
#pragma unroll
                for (int i = 0; i < T::OPL; ++i) o[co][i] = fmaf(wv, m[i + j], o[co][i]);
            }
    }
}

// phases B, C, D of one network.  In: the table holds m, dos the staged dO, rows the staged rows, x this lane's windows of the network's
// rows.  acc4 / acc6: this thread's parameter entries.  Ends with a barrier: the table and dos may be written again.
template <class T>
__device__ __forceinline__ void dec_bwd_net(int net, const float (&x)[T::C][T::XW], const DecNet& w, float* tab, const float* rows, const float* dos,
                                            const float* w1s, int nvalid, bool live, long n, float* dh, float (&acc4)[T::EPT4], float (&acc6)[T::EPT6]) {
    constexpr int C = T::C, K1 = T::K1, S1 = T::S1, K2 = T::K2, L1 = T::L1, PP = T::PP, LP = T::LP, NS = T::NS, TW = T::TW;
    const int tid = threadIdx.x, q = tid & 7, nl = tid >> 3;
    // ---- B: dW2[co][c][j] and db2[co] ---------------------------------------------------------------------------------
#pragma unroll
    for (int k = 0; k < T::EPT4; ++k) {
        const int e = tid + k * DBT;
        float s = 0.f;
        if (e < T::NW2) {
            const int co = e / (8 * K2), c = (e / K2) % 8, j = e % K2;
            for (int nn = 0; nn < nvalid; ++nn) {
                const float* d = dos + (nn * C + co) * T::DOL + T::PADF;
                const float* m = tab + nn * NS + c * LP + j;
#pragma unroll 5
                for (int t = 0; t < TW; ++t) s = fmaf(d[t], m[t], s);
            }
        } else if (e < T::E4) {
            const int co = e - T::NW2;
            for (int nn = 0; nn < nvalid; ++nn) {
                const float* d = dos + (nn * C + co) * T::DOL + T::PADF;
#pragma unroll 5
                for (int t = 0; t < TW; ++t) s += d[t];
            }
        }
        acc4[k] += s;
    }
    // this lane's dO windows: dwin[co][i] = dO[co][q PP - (K2 - 1) + i], zero outside 0 .. TW - 1
    float dwin[C][T::DW];
#pragma unroll
    for (int co = 0; co < C; ++co)
#pragma unroll
        for (int i = 0; i < T::DW; ++i) dwin[co][i] = dos[(nl * C + co) * T::DOL + q * PP + i];
    __syncthreads();        // every thread has read m: the table takes ds
    // ---- C: ds = dm Swish'(s) -------------------------------------------------------------------------------------------
    {
        float* mrow = tab + nl * NS;
        const int p0 = q * PP;
#pragma unroll 1
        for (int c = 0; c < 8; ++c) {
            float s[PP], dm[PP];
            dec_bwd_conv1<T>(x, w, c, s);
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) dm[pp] = 0.f;
#pragma unroll
            for (int co = 0; co < C; ++co)
#pragma unroll
                for (int j = 0; j < K2; ++j) {
                    const float wv = w.w2[(co * 8 + c) * K2 + j];
#pragma unroll
                    for (int pp = 0; pp < PP; ++pp) dm[pp] = fmaf(wv, dwin[co][pp + (K2 - 1) - j], dm[pp]);
                }
#pragma unroll
            for (int pp = 0; pp < PP; ++pp) {
                const float sg = sigmoidf_(s[pp]);
                const float dsw = sg * fmaf(s[pp], 1.0f - sg, 1.0f);        // Swish'(s) = sigma (1 + s (1 - sigma))
                if (p0 + pp < L1) mrow[c * LP + p0 + pp] = dm[pp] * dsw;
            }
        }
    }
    __syncthreads();        // ds complete
    // ---- D: dW1[c][ci][j] and db1[c] ------------------------------------------------------------------------------------
#pragma unroll
    for (int k = 0; k < T::EPT6; ++k) {
        const int e = tid + k * DBT;
        float s = 0.f;
        if (e < T::NW1) {
            const int c = e / (C * K1), ci = (e / K1) % C, j = e % K1;
            for (int nn = 0; nn < nvalid; ++nn) {
                const float* d = tab + nn * NS + c * LP;
                const float* xr = rows + nn * T::RW + ci * T::CS + net * T::R + j;
#pragma unroll 3
                for (int p = 0; p < L1; ++p) s = fmaf(d[p], xr[p * S1], s);
            }
        } else if (e < T::E6) {
            const int c = e - T::NW1;
            for (int nn = 0; nn < nvalid; ++nn) {
                const float* d = tab + nn * NS + c * LP;
#pragma unroll 3
                for (int p = 0; p < L1; ++p) s += d[p];
            }
        }
        acc6[k] += s;
    }
    // ---- D: dh, lane q the row positions q, q + 8, .. -------------------------------------------------------------------
    if (live) {
        const float* drow = tab + nl * NS;
        const float* wn = w1s + net * T::NW1;
#pragma unroll
        for (int ci = 0; ci < C; ++ci) {
            float* out = dh + (size_t)n * T::RW + ci * T::CS + net * T::R;
#pragma unroll 1
            for (int i = q; i < T::R; i += 8) {
                const int r = i % S1, pb = i / S1;
                float v = 0.f;
#pragma unroll
                for (int c = 0; c < 8; ++c)
#pragma unroll
                    for (int jj = 0; jj < T::NJ; ++jj) {
                        const int j = r + jj * S1, p = pb - jj;
                        const bool ok = j < K1 && p >= 0 && p < L1;
                        const float wv = wn[(c * C + ci) * K1 + (ok ? j : 0)];
                        const float dv = drow[c * LP + (ok ? p : 0)];
                        v = ok ? fmaf(wv, dv, v) : v;
                    }
                out[i] = v;
            }
        }
    }
    __syncthreads();        // every thread has read ds and dos
}

template <class T>
__global__ __launch_bounds__(DBT) void decoder_bwd_kernel(DecBwdArgs a) {
    constexpr int C = T::C, TW = T::TW, OPL = T::OPL, NS = T::NS;
    __shared__ __attribute__((aligned(16))) float lds[T::LDS_FLOATS];
    float* tab = lds;                                   // [16][NS]
    float* rows = tab + DEC_BWD_NODES * NS;             // [16][RW]
    float* dos = rows + DEC_BWD_NODES * T::RW;          // [16][C][DOL]
    float* w1s = dos + DEC_BWD_NODES * C * T::DOL;      // [NETS][NW1]
    const int tid = threadIdx.x, q = tid & 7, nl = tid >> 3, t0 = q * OPL;
    for (int i = tid; i < DEC_BWD_NODES * C * T::DOL; i += DBT) dos[i] = 0.f;       // the pads stay zero: only t < TW is written below
    for (int i = tid; i < T::NETS * T::NW1; i += DBT) w1s[i] = a.net[i / T::NW1].w1[i % T::NW1];
    float acc4[T::NETS][T::EPT4], acc6[T::NETS][T::EPT6];
#pragma unroll
    for (int ne = 0; ne < T::NETS; ++ne) {
#pragma unroll
        for (int k = 0; k < T::EPT4; ++k) acc4[ne][k] = 0.f;
#pragma unroll
        for (int k = 0; k < T::EPT6; ++k) acc6[ne][k] = 0.f;
    }
    const long nblk = (a.n_nodes + DEC_BWD_NODES - 1) / DEC_BWD_NODES;
    __syncthreads();
#pragma unroll 1
    for (long blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
        const long n0 = blk * DEC_BWD_NODES;
        const int nvalid = a.n_nodes - n0 < DEC_BWD_NODES ? (int)(a.n_nodes - n0) : DEC_BWD_NODES;
        const long n = n0 + nl;
        const bool live = nl < nvalid;
        const long nc = live ? n : a.n_nodes - 1;       // lanes past the end: a valid row, dO = 0, nothing stored
        const float* row = a.h + (size_t)nc * (size_t)a.ld;
        for (int i = tid; i < nvalid * T::RW; i += DBT) rows[i] = a.h[(size_t)(n0 + i / T::RW) * (size_t)a.ld + i % T::RW];
        // grad_out and cumsum(dt) of this lane's outputs
        float g[C][OPL], tc[OPL];
        {
            float tcum = 0.f;
            for (int t = 0; t < t0; ++t) tcum += a.dt;          // float32 partial sums, like the forward
#pragma unroll
            for (int i = 0; i < OPL; ++i) {
                tcum += a.dt;
                tc[i] = tcum;
#pragma unroll
                for (int co = 0; co < C; ++co) g[co][i] = live && t0 + i < TW ? a.g[(size_t)n * C * TW + co * TW + t0 + i] : 0.f;
            }
        }
        float* mrow = tab + nl * NS;
        float* drow = dos + nl * C * T::DOL + T::PADF;
        float x[C][T::XW];
        if constexpr (T::MODE != 2) {
#pragma unroll
            for (int co = 0; co < C; ++co)
#pragma unroll
                for (int i = 0; i < OPL; ++i)
                    if (t0 + i < TW) drow[co * T::DOL + t0 + i] = T::MODE == 1 ? g[co][i] * tc[i] : g[co][i];
            dec_bwd_load_x<T>(row, q, x);
            dec_bwd_phase_a<T>(x, a.net[0], mrow, q);
            __syncthreads();
            dec_bwd_net<T>(0, x, a.net[0], tab, rows, dos, w1s, nvalid, live, n, a.dh, acc4[0], acc6[0]);
        } else {
            float scale[C][OPL], diff[C][OPL];
            dec_bwd_load_x<T>(row, q, x);                       // gate: the first R values of a component
            dec_bwd_phase_a<T>(x, a.net[0], mrow, q);
            __syncthreads();
            dec_bwd_outputs<T>(mrow, a.net[0], q, scale);
            __syncthreads();                                    // the table takes diff's m
            dec_bwd_load_x<T>(row + T::R, q, x);
            dec_bwd_phase_a<T>(x, a.net[1], mrow, q);
            __syncthreads();
            dec_bwd_outputs<T>(mrow, a.net[1], q, diff);
            float dgate[C][OPL];
            const float* up = a.u + (size_t)nc * C * TW;
#pragma unroll
            for (int co = 0; co < C; ++co)
#pragma unroll
                for (int i = 0; i < OPL; ++i) {
                    const bool in = t0 + i < TW;
                    const float us = C == 1 ? up[TW - 1] : up[co * TW + (in ? t0 + i : 0)];
                    dgate[co][i] = g[co][i] * (tc[i] * diff[co][i] - us);
                    if (in) drow[co * T::DOL + t0 + i] = (g[co][i] * tc[i]) * scale[co][i];
                }
            __syncthreads();                                    // dO of diff staged
            dec_bwd_net<T>(1, x, a.net[1], tab, rows, dos, w1s, nvalid, live, n, a.dh, acc4[1], acc6[1]);
            dec_bwd_load_x<T>(row, q, x);
            dec_bwd_phase_a<T>(x, a.net[0], mrow, q);
#pragma unroll
            for (int co = 0; co < C; ++co)
#pragma unroll
                for (int i = 0; i < OPL; ++i)
                    if (t0 + i < TW) drow[co * T::DOL + t0 + i] = dgate[co][i];
            __syncthreads();
            dec_bwd_net<T>(0, x, a.net[0], tab, rows, dos, w1s, nvalid, live, n, a.dh, acc4[0], acc6[0]);
        }
    }
    // this workgroup's row of the partials: every entry written once
    float* prow = a.partial + (size_t)blockIdx.x * T::ROW;
#pragma unroll
    for (int ne = 0; ne < T::NETS; ++ne) {
#pragma unroll
        for (int k = 0; k < T::EPT6; ++k)
            if (tid + k * DBT < T::E6) prow[ne * T::NET_E + tid + k * DBT] = acc6[ne][k];
#pragma unroll
        for (int k = 0; k < T::EPT4; ++k)
            if (tid + k * DBT < T::E4) prow[ne * T::NET_E + T::E6 + tid + k * DBT] = acc4[ne][k];
    }
}

// Second stage: entry e of the gradients = the sum of column e of the partial rows in a fixed order (a wave per entry: lane l the rows
// l, l + 64, .. ascending, then a butterfly over the lanes).  seg: where the entries of a partial row go, start[k] .. start[k + 1] - 1 to dst[k].
struct DecBwdSum {
    const float* partial;
    int rows, row_floats, n_seg;
    int start[9];
    float* dst[8];
};

__global__ __launch_bounds__(256) void decoder_bwd_sum_kernel(DecBwdSum s) {
    const int e = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (e >= s.row_floats) return;          // a whole wave
    float v = 0.f;
    for (int r = lane; r < s.rows; r += 64) v += s.partial[(size_t)r * s.row_floats + e];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    if (lane == 0) {
        int k = 0;
        while (k + 1 < s.n_seg && e >= s.start[k + 1]) ++k;
        s.dst[k][e - s.start[k]] = v;
    }
}

}  // namespace msmp

using namespace msmp;

// 1-D / 2-D decoders of the 128-wide classes (geometries of msmp_decoder_f32 / msmp_decoder2d_f32), gated decoders of the GLU classes
template <int C, int MODE> using Bwd20 = DecBwd<C, H, 1, 20, 15, 4, 10, MODE>;
template <int C, int MODE> using Bwd25 = DecBwd<C, H, 1, 25, 16, 3, 14, MODE>;
template <int C, int MODE> using Bwd50 = DecBwd<C, H, 1, 50, 12, 2, 10, MODE>;
template <int C> using BwdGated = DecBwd<C, 82, 2, 25, 6, 2, 15, 2>;

// floats of a partial row, 0: no such decoder
static int dec_bwd_row_floats(int comps, int gated, int width, int tw) {
    if (comps != 1 && comps != 2) return 0;
    if (gated) return width == 164 && tw == 25 ? 2 * dec_bwd_net_entries(comps, 6, 15) : 0;
    if (width != H) return 0;
    switch (tw) {
        case 20: return comps == 1 ? dec_bwd_net_entries(1, 15, 10) : 0;
        case 25: return dec_bwd_net_entries(comps, 16, 14);
        case 50: return dec_bwd_net_entries(comps, 12, 10);
    }
    return 0;
}

extern "C" size_t msmp_decoder_bwd_workspace_bytes(int comps, int gated, int width, int tw) {
    return (size_t)DEC_BWD_GRID_CAP * (size_t)dec_bwd_row_floats(comps, gated, width, tw) * sizeof(float);
}

template <class T>
static int dec_bwd_launch(const char* who, DecBwdArgs a, const DecNetGrad* grads, hipStream_t st) {
    const long nblk = (a.n_nodes + DEC_BWD_NODES - 1) / DEC_BWD_NODES;
    const int grid = nblk < DEC_BWD_GRID_CAP ? (int)nblk : DEC_BWD_GRID_CAP;
    hipLaunchKernelGGL((decoder_bwd_kernel<T>), dim3(grid), dim3(DBT), 0, st, a);
    DecBwdSum s{};
    s.partial = a.partial;
    s.rows = grid;
    s.row_floats = T::ROW;
    s.n_seg = 4 * T::NETS;
    for (int ne = 0; ne < T::NETS; ++ne) {
        const int k = 4 * ne, o = ne * T::NET_E;
        s.start[k] = o;                     s.dst[k] = grads[ne].w1;
        s.start[k + 1] = o + T::NW1;        s.dst[k + 1] = grads[ne].b1;
        s.start[k + 2] = o + T::E6;         s.dst[k + 2] = grads[ne].w2;
        s.start[k + 3] = o + T::E6 + T::NW2; s.dst[k + 3] = grads[ne].b2;
    }
    s.start[s.n_seg] = T::ROW;
    hipLaunchKernelGGL(decoder_bwd_sum_kernel, dim3((T::ROW + 3) / 4), dim3(256), 0, st, s);
    return check_launch(who);
}

static bool all_set(const DecNet& w, const DecNetGrad& g) { return w.w1 && w.b1 && w.w2 && w.b2 && g.w1 && g.b1 && g.w2 && g.b2; }

static int decoder_bwd(const char* who, int comps, const float* g, const float* h, int64_t n_nodes, int tw, bool euler, const DecNet& w, float dt,
                       float* dh, const DecNetGrad& grad, void* workspace, size_t workspace_bytes, msmp_stream_t stream) {
    MSMP_REQUIRE(g && h && dh && workspace && all_set(w, grad), MSMP_ERR_ARG, "%s: null pointer", who);
    MSMP_REQUIRE(n_nodes > 0 && n_nodes < (1L << 31), MSMP_ERR_ARG, "%s: bad n_nodes", who);
    const size_t need = msmp_decoder_bwd_workspace_bytes(comps, 0, H, tw);
    MSMP_REQUIRE(need != 0, MSMP_ERR_UNSUPPORTED, "%s: time_window %d (the reference defines %s25, 50)", who, tw, comps == 1 ? "20, " : "");
    MSMP_REQUIRE(workspace_bytes >= need, MSMP_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    DecBwdArgs a{h, (long)(comps * H), nullptr, g, (long)n_nodes, {w, DecNet{}}, dt, dh, (float*)workspace};
    hipStream_t st = (hipStream_t)stream;
    if (comps == 2) {
        if (tw == 25) return dec_bwd_launch<Bwd25<2, 1>>(who, a, &grad, st);
        return dec_bwd_launch<Bwd50<2, 1>>(who, a, &grad, st);
    }
    if (euler) {
        if (tw == 20) return dec_bwd_launch<Bwd20<1, 1>>(who, a, &grad, st);
        if (tw == 25) return dec_bwd_launch<Bwd25<1, 1>>(who, a, &grad, st);
        return dec_bwd_launch<Bwd50<1, 1>>(who, a, &grad, st);
    }
    if (tw == 20) return dec_bwd_launch<Bwd20<1, 0>>(who, a, &grad, st);
    if (tw == 25) return dec_bwd_launch<Bwd25<1, 0>>(who, a, &grad, st);
    return dec_bwd_launch<Bwd50<1, 0>>(who, a, &grad, st);
}

extern "C" int msmp_decoder_bwd_f32(const float* grad_out, const float* h, int64_t n_nodes, int tw, int euler, const float* w1, const float* b1,
                                    const float* w2, const float* b2, float dt, float* dh, float* dw1, float* db1, float* dw2, float* db2,
                                    void* workspace, size_t workspace_bytes, msmp_stream_t stream) {
    return decoder_bwd("msmp_decoder_bwd_f32", 1, grad_out, h, n_nodes, tw, euler != 0, DecNet{w1, b1, w2, b2}, dt, dh, DecNetGrad{dw1, db1, dw2, db2},
                       workspace, workspace_bytes, stream);
}

extern "C" int msmp_decoder2d_bwd_f32(const float* grad_out, const float* hd, int64_t n_nodes, int tw, const float* w1, const float* b1,
                                      const float* w2, const float* b2, float dt, float* dh, float* dw1, float* db1, float* dw2, float* db2,
                                      void* workspace, size_t workspace_bytes, msmp_stream_t stream) {
    return decoder_bwd("msmp_decoder2d_bwd_f32", 2, grad_out, hd, n_nodes, tw, true, DecNet{w1, b1, w2, b2}, dt, dh, DecNetGrad{dw1, db1, dw2, db2},
                       workspace, workspace_bytes, stream);
}

static int decoder_gated_bwd(const char* who, int comps, const float* g, const float* h, int ld, const float* u, int64_t n_nodes, int width, int tw,
                             const DecNet& gate, const DecNet& diff, float dt, float* dh, const DecNetGrad& dgate, const DecNetGrad& ddiff,
                             void* workspace, size_t workspace_bytes, msmp_stream_t stream) {
    MSMP_REQUIRE(g && h && u && dh && workspace && all_set(gate, dgate) && all_set(diff, ddiff), MSMP_ERR_ARG, "%s: null pointer", who);
    MSMP_REQUIRE(n_nodes > 0 && n_nodes < (1L << 31), MSMP_ERR_ARG, "%s: bad n_nodes", who);
    const size_t need = msmp_decoder_bwd_workspace_bytes(comps, 1, width, tw);
    MSMP_REQUIRE(need != 0, MSMP_ERR_UNSUPPORTED, "%s: width %d, time_window %d (the reference defines 164, 25)", who, width, tw);
    MSMP_REQUIRE(ld >= comps * width, MSMP_ERR_ARG, "%s: row stride ld = %d < %d", who, ld, comps * width);
    MSMP_REQUIRE(workspace_bytes >= need, MSMP_ERR_WORKSPACE, "%s: workspace of %zu bytes, %zu needed", who, workspace_bytes, need);
    DecBwdArgs a{h, (long)ld, u, g, (long)n_nodes, {gate, diff}, dt, dh, (float*)workspace};
    const DecNetGrad grads[2] = {dgate, ddiff};
    hipStream_t st = (hipStream_t)stream;
    if (comps == 2) return dec_bwd_launch<BwdGated<2>>(who, a, grads, st);
    return dec_bwd_launch<BwdGated<1>>(who, a, grads, st);
}

#define MSMP_DEC_GATED_BWD_ENTRY(NAME, COMPS)                                                                                                    \
    extern "C" int NAME(const float* grad_out, const float* h, int ld, const float* u, int64_t n_nodes, int width, int tw, const float* gate_w1,   \
                        const float* gate_b1, const float* gate_w2, const float* gate_b2, const float* diff_w1, const float* diff_b1,              \
                        const float* diff_w2, const float* diff_b2, float dt, float* dh, float* dgate_w1, float* dgate_b1, float* dgate_w2,        \
                        float* dgate_b2, float* ddiff_w1, float* ddiff_b1, float* ddiff_w2, float* ddiff_b2, void* workspace,                      \
                        size_t workspace_bytes, msmp_stream_t stream) {                                                                            \
        return decoder_gated_bwd(#NAME, COMPS, grad_out, h, ld, u, n_nodes, width, tw, DecNet{gate_w1, gate_b1, gate_w2, gate_b2},                 \
                                 DecNet{diff_w1, diff_b1, diff_w2, diff_b2}, dt, dh, DecNetGrad{dgate_w1, dgate_b1, dgate_w2, dgate_b2},           \
                                 DecNetGrad{ddiff_w1, ddiff_b1, ddiff_w2, ddiff_b2}, workspace, workspace_bytes, stream);                          \
    }
MSMP_DEC_GATED_BWD_ENTRY(msmp_decoder_gated_bwd_f32, 1)
MSMP_DEC_GATED_BWD_ENTRY(msmp_decoder2d_gated_bwd_f32, 2)
#undef MSMP_DEC_GATED_BWD_ENTRY
