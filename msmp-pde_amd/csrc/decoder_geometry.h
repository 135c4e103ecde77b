// Geometry and argument blocks of the decoder kernels, shared by the forward (decoder_kernel.hip) and the backward
// (decoder_bwd_kernel.hip): a network is Conv1d(C -> 8, K1, stride S1) -> Swish -> Conv1d(8 -> C, K2) on a row of R values.
#pragma once
#include "msmp_common.h"

namespace msmp {

template <int TW, int K1, int S1, int K2, int R = H>                // R: length of the row a network reads (the gated decoders: half a 164-wide row)
struct DecSplit {
    static constexpr int L1 = (R - K1) / S1 + 1;
    static constexpr int PP = (L1 + 7) / 8;                          // intermediate positions per lane
    static constexpr int XW = (PP - 1) * S1 + K1;                    // row values a lane needs
    static constexpr int OPL = TW > 32 ? 8 : 4;                      // consecutive outputs per lane (multiple of 4: aligned 16-byte LDS reads)
    static constexpr int MW = OPL + K2 - 1;                          // intermediate values per channel a lane needs for them
    static constexpr int MW4 = (MW + 3) / 4;
    static constexpr int LP = ((7 * OPL + 4 * MW4 > L1 ? 7 * OPL + 4 * MW4 : L1) + 3) / 4 * 4 + 4;      // padded row of the LDS table
    static constexpr int NODES = 8 * LP * 4 * 32 <= 49152 ? 32 : 16;  // nodes per workgroup (LDS <= 48 KB)
    static_assert(L1 - K2 + 1 == TW && 8 * OPL >= TW, "decoder geometry");
};

struct DecArgs {
    const float* h;      // [N,128]
    const float* u;      // [N,tw] (nullptr: the decoder output alone, what MSSMP_PDE_Solver_sub returns, models_gnn.py:1679-1682)
    long n_nodes;
    const float* w1;     // [8][k1]
    const float* b1;     // [8]
    const float* w2;     // [8][k2]
    const float* b2;     // [1]
    float dt;
    float* out;          // [N,tw]
};

struct Dec2Args {
    const float* hd;     // [N, 2, 128]
    const float* u;      // [N, 2*tw]
    long n_nodes;
    const float* w1;     // [8][2][k1]
    const float* b1;     // [8]
    const float* w2;     // [2][8][k2]
    const float* b2;     // [2]
    float dt;
    float* out;          // [N, 2*tw]
};

struct DecNet {
    const float* w1;     // [8][C][k1]
    const float* b1;     // [8]
    const float* w2;     // [C][8][k2]
    const float* b2;     // [C]
};

struct DecGatedArgs {
    const float* h;      // 1-D: [N, ld] rows of 164;  2-D: [N, ld] rows of 2 x 164 (hd)
    long ld;             // row stride in floats
    const float* u;      // [N, C tw]
    long n_nodes;
    DecNet gate, diff;
    float dt;
    float* out;          // [N, C tw]
};

// ---- backward (decoder_bwd_kernel.hip) ---------------------------------------------------------------------------------
// Gradients of one network, in the layouts of its parameters.
struct DecNetGrad {
    float* w1;           // [8][C][k1]
    float* b1;           // [8]
    float* w2;           // [C][8][k2]
    float* b2;           // [C]
};

// Partial sums of the parameter gradients: every workgroup writes ONE row of the workspace, a second launch adds the rows in a fixed
// order.  The grid is capped (grid-stride loop over blocks of DEC_BWD_NODES nodes), so the workspace does not grow with N.
constexpr int DEC_BWD_NODES = 16;           // nodes per workgroup pass (eight lanes each: 128 threads)
constexpr int DEC_BWD_GRID_CAP = 512;       // workgroups, and with it partial rows, at most

// Entries of a network's partial row: [dW1 | db1 | dW2 | db2]
__host__ __device__ constexpr int dec_bwd_net_entries(int comps, int k1, int k2) { return 8 * comps * k1 + 8 + comps * 8 * k2 + comps; }

struct DecBwdArgs {
    const float* h;      // rows of `nets` x (C components of R values); component stride and network offset are template constants
    long ld;             // row stride in floats
    const float* u;      // gated only: [N, C tw]
    const float* g;      // grad_out [N, C tw]
    long n_nodes;
    DecNet net[2];       // one-network decoders: net[0]; gated: gate, diff
    float dt;
    float* dh;           // compact rows: [N, C W]
    float* partial;      // [gridDim.x][row_floats]
};

}  // namespace msmp
