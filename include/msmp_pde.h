/*
 * msmp_pde.h -- C-ABI of libmsmp_pde.so: the MI355X (gfx950) message-passing rollout path of MSMP-PDE.
 *
 * This is the drop-in boundary.  The reference (Leqr/MSMP-PDE, 100 % Python)
 * reaches native code for this path only through third-party Python extensions (torch_geometric,
 * torch_scatter, torch_cluster, lem_cuda); each entry point below names the reference call site it
 * replaces (paths relative to the reference root).  Conventions:
 *
 *   - plain C: raw DEVICE pointers + sizes, no torch / C++ types;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); every call is stream-ordered,
 *     never synchronises the device and never allocates: scratch comes from `workspace`;
 *   - all matrices row-major; float tensors are fp32 unless the name says f64; indices are int32 on
 *     the compute path (int64 only where the reference's `edge_index` is produced / consumed);
 *   - returns MSMP_OK (0) or a negative MSMP_ERR_*; msmp_last_error() gives the text; never throws;
 *   - hidden width is fixed at MSMP_HIDDEN = 128 (hidden_features, experiments/models_gnn.py:158).
 *
 * Layer weights are passed as a "packed layer" blob made by msmp_pack_layer_f32 from the reference's
 * eight nn.Linear tensors ([out,in] layout); see DESIGN.md section 3 for the blob layout.
 */
#ifndef MSMP_PDE_H
#define MSMP_PDE_H

#include <stddef.h>
#include <stdint.h>

/* The library is built with hidden visibility and -Bsymbolic: only the msmp_* entry points are exported, and its
 * internal (rocPRIM, C++ runtime template) symbols can neither be interposed by nor leak into the host process
 * (PyTorch ships its own rocPRIM build). */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define MSMP_HIDDEN 128
#define MSMP_MAX_VARS 8          /* len(eq_variables) + 1 <= 8 */

#define MSMP_OK               0
#define MSMP_ERR_ARG         -1  /* null pointer / bad size */
#define MSMP_ERR_UNSUPPORTED -2  /* shape outside what the kernels are built for */
#define MSMP_ERR_WORKSPACE   -3  /* workspace too small */
#define MSMP_ERR_HIP         -4  /* HIP runtime error (text in msmp_last_error) */

/* flags for msmp_node_update_f32 / msmp_mp_layer_f32 */
#define MSMP_LAYER_RESIDUAL_SWISH 0  /* GNN_Layer.update    experiments/models_gnn.py:77-86  : x + Swish(W4 . + b4) */
#define MSMP_LAYER_LIN            1  /* GNN_LayerLin.update experiments/models_gnn.py:140-149: W4 . + b4           */
/* OR-ed into `mode` of msmp_mp_layer_f32: evaluate message_net_1 on the materialised per-edge
 * concatenation (the reference's literal order of operations) instead of the per-node factorisation. */
#define MSMP_LAYER_DENSE_MESSAGE  16

typedef void* msmp_stream_t;

/* ABI version: 470 = msmp_batch_assemble_f32 added; 460 = msmp_grads_finite_workspace_bytes, msmp_grads_finite_f32, msmp_adamw_guarded_f32 and msmp_status_poison_f32 added; 450 = msmp_g2_gate_blend_f32, msmp_g2_gate_blend_bwd_workspace_bytes, msmp_g2_gate_blend_bwd_f32 and the switch "g2_gate" added; 440 = the eight msmp_*lstm* entries and the switch "lstm_train" added; 430 = the six msmp_*mlp_train* entries and the switch "mlp_train" added; 420 = the five entries of the 128-wide LEM training pair removed (msmp_lem_train_fwd_wide_f32 / _bwd_wide_f32 serve every
 * width) and the blob of msmp_pack_lem_f32 without its last section, which only that pair read; 410 = msmp_mp_layer_decode_f32 and msmp_decoder_t removed;
 * 400 = round 4 (msmp_tiles_t: listed, period_tiles, period_nodes; msmp_build_tiles writes 3 statistics);
 * 300 = round 3 (msmp_last_status, msmp_tiles_t checked on every entry point that takes one).  Bumped whenever a
 * prototype or a blob layout changes; the ctypes host refuses a library whose version is not the one it was written for. */
#define MSMP_ABI_VERSION 470
int msmp_version(void);
const char* msmp_last_error(void);

/* Sticky range status of the fp16-split matrix path ("Range").  The default kernels carry node rows scaled
 * by 2^8 (saturating at +-65504, i.e. |x| <= 255) and hidden activations scaled by 2^6 (|x| < 1023, beyond that fp16 inf); the
 * reference has no such limit.  Kernels OR a bit into a host-visible word when a value leaves that range, so wrong-but-finite or
 * NaN output never goes unnoticed:
 *   MSMP_STATUS_INPUT_RANGE     an input feature (u, pos / L, a variables column) had |x| > 255 or was not finite
 *                               (msmp_prepare_nodes, msmp_pack_node_features_f32);
 *   MSMP_STATUS_NODE_SATURATED  a hidden-state row staged by the tile kernel, a row of the blend, or an aggregate written by a
 *                               message kernel had |x| > 255 (or was NaN: an activation above 1023 overflowed upstream);
 *   MSMP_STATUS_NONFINITE       the InstanceNorm statistics of a graph were not finite (node tail).
 * msmp_last_status reads the word WITHOUT synchronising (it lives in host-mapped memory the kernels update with system-scope
 * atomics: what it returns covers all work that has completed; after a stream synchronise, all work issued).  reset != 0 clears
 * it.  Remedy: rescale the data, or run the exact-fp32 kernels (msmp_tune("split", 0): no range limit). */
#define MSMP_STATUS_INPUT_RANGE    1
#define MSMP_STATUS_NODE_SATURATED 2
#define MSMP_STATUS_NONFINITE      4
int msmp_last_status(int* flags_out, int reset);
/* Knobs for A/B measurements and validation (not part of the data contract).  Every key below can be set and queried; each entry
 * names its default.  msmp_tune returns MSMP_ERR_ARG for NULL, for a key that is not listed ("unknown key") and for a value outside
 * a key's stated range (the value stays as it was); msmp_tune_query returns 0 for NULL and for a key that is not listed.
 *   "split"   1 (default): the GEMMs of the node / edge / LEM kernels run on the fp16 matrix pipe with a 2-way
 *             fp16 split of both operands (fp32-class accuracy); 0: the fp32-MFMA kernels.  It also selects
 *             the LEM kernel: 1 the weight-stationary lem_encoder_ws3_kernel, 0 the fp32 lem_encoder_kernel.
 *   "edge_nb" 0 (default) auto, 1 / 2 force the 128- / 256-edge tile of the factorised message kernel.
 *   "tile"    2 (default): with node tiles that are at least 60 % full (>= 76 edges per tile on average), project P / Q inside the message
 *             kernel, else the gather kernels; 3: the same regardless of the fill; 1: msmp_node_project_f32 + tile kernel on the
 *             staged P / Q rows; 0: ignore the tiles (gather kernels).
 *   "bwd_gemm" 1 (default) / 2: msmp_mp_layer_bwd_f32 runs its row GEMMs on its own bf16x3 MFMA kernels (fused bias / Swish / dSwish epilogues;
 *             128-row workgroups from 32 768 rows on, 32-row workgroups whose waves split the output channels below);
 *             0: rocblas_sgemm + separate epilogue passes (A/B runs only: librocblas is loaded on first use).
 *   "lem_share" k (default 1; accepted: 1 to 16): k LEM launches share the GPU (sub-batches on k streams): each plans its rounds for CUs / k.
 *   "lem_tail" 1 (default): the LEM launch ends with a round of one-tile workgroups where that saves >= 0.3 of a round; 0: three-tile
 *             workgroups only (same bits either way).
 *   "lem_wide" 1 (default): the host's no-grad LEM at widths other than 128 is one msmp_lem_encoder_wide_f32 launch; 0: the loop of two
 *             library GEMMs + msmp_wide_lem_z_f32 / _y_f32 per time step (the entry itself does not read the key).
 *   "lem_wide_train" 1 (default): under autograd the host's LEM at every width is msmp_lem_train_fwd_wide_f32 + msmp_lem_train_bwd_wide_f32 +
 *             one msmp_grad_weights_cat_f32; 0: the PyTorch ops of the restated cell, differentiated by autograd (the entries themselves do
 *             not read the key; any value other than 0 selects the kernels).
 *   "wide_msg" 1 (default): the host's no-grad layer at widths other than 128 evaluates the message half of a head as one
 *             msmp_wide_message_f32 launch; 0: msmp_wide_gather_swish_f32 + msmp_linear_f32 + msmp_wide_scatter_mean_f32 around two
 *             [E, ld] tensors (the entry itself does not read the key).  The host takes the fused launch only while "split" and
 *             "lem_wide" are 1 as well: "lem_wide" 0 selects the unfused width-generic path as a whole, bitwise the exact-fp32 evaluation.
 *   "wide_tail" 1: the host's no-grad layer at widths other than 128 evaluates the node half of a layer (both heads of a gated
 *             pair) as one msmp_wide_node_tail_f32 launch on graphs of up to 128 nodes; 0 (default): per head a concatenation and two
 *             msmp_linear_f32, then msmp_wide_norm_blend_f32 (the entry itself does not read the key).  The host takes the fused launch only while "wide_msg",
 *             "split" and "lem_wide" are 1 as well, so each of those keeps selecting the path it selected before this kernel.  The
 *             fused launch runs update_net_2 CENTRED per graph (on Swish(z_n) - Swish(z of the graph's first node), without its bias b4:
 *             InstanceNorm removes the constant), so b4 does not enter its result.
 *   "wide_proj" 1: the host's no-grad layer at widths other than 128 evaluates the P / Q projections of message_net_1 (both heads of
 *             a gated pair) as one msmp_wide_node_proj_f32 launch; 0 (default): a concatenation [h | u | pos | vars] and two msmp_linear_f32 per head
 *             (the entry itself does not read the key).  The host takes the fused launch only while "wide_msg", "split" and "lem_wide" are 1
 *             as well, so each of those keeps selecting the path it selected before this kernel.
 *   "wide_bwd" 1 (default): under autograd the host's layer at widths other than 128 runs the width-generic HIP forward (saving only the
 *             layer inputs) and one msmp_wide_layer_bwd_f32 call per layer / gated pair as its backward; 0: PyTorch ops differentiated by
 *             torch.autograd (the entry itself does not read the key; any value other than 0 selects the kernels).  float64 inputs and sizes the
 *             entry refuses by value keep the PyTorch ops.  Measured: DESIGN.md section 4.23.
 *   "wide_dec" 1 (default): the host's no-grad forward of the GLU classes ends in one msmp_decoder_gated_f32 / msmp_decoder2d_gated_f32
 *             launch (2-D: after double_mlp as one msmp_linear_f32); 0: the decoder's PyTorch ops (the entries themselves do not read the
 *             key; any value other than 0 selects the launch).  The host takes the launch only while "wide_msg", "split" and "lem_wide"
 *             are 1 as well, so each of those keeps selecting the path it selected before these kernels.
 *   "dec_bwd" 1 (default): under autograd the host's CNN decoder of every solver class is msmp_decoder*_train_fwd_f32 forward and one
 *             msmp_decoder*_bwd_f32 call backward; 0: PyTorch-ROCm ops (Toeplitz GEMMs) differentiated by torch.autograd (the entries
 *             themselves do not read the key; any value other than 0 selects the kernels).  The GLU classes take them only while "wide_msg",
 *             "split" and "lem_wide" are 1 as well.  CPU tensors, float64, a `u` that requires grad and sizes the entries refuse by value
 *             keep the PyTorch ops.  Measured: DESIGN.md section 4.24.
 *   "mlp_train" 1 (default): under autograd the host's Swish MLPs around the encoder and decoder (embedding_mlp, lemoutput_mlp,
 *             lstmoutput_mlp, double_mlp) are one msmp_mlp_train_fwd_f32 launch forward and one msmp_mlp_train_bwd_f32 call backward;
 *             0: the PyTorch module (library GEMMs and elementwise kernels) differentiated by torch.autograd (the entries themselves
 *             do not read the key; any value other than 0 selects the kernels).  CPU tensors, float64, a call in which nothing requires
 *             grad and sizes the entries refuse by value keep the PyTorch ops.  Measured: DESIGN.md section 4.25.
 *   "lstm_train" 1: the host's LSTM encoder (the LSTM ablation classes) is ONE msmp_lstm_train_fwd_f32 launch, with `saved` and followed by
 *             msmp_lstm_train_bwd_f32 + one msmp_grad_weights_cat_f32 under autograd, with saved = NULL without; 0 (default): torch.nn.LSTM
 *             (MIOpen) with and without grad (the entries themselves do not read the key; any value other than 0 selects the kernels).  CPU
 *             tensors, float64, step inputs that require grad and sizes the entries refuse by value keep torch.nn.LSTM.  Measured, and why it
 *             ships at 0 although every measured configuration is faster at 1: DESIGN.md section 4.26.
 *   switch "g2_gate" 1 (default): the host's gradient-gated pair (MP_PDE_Solver2DLEMLinG2) evaluates the gate statistic, tanh and blend
 *             between its two layer calls as ONE msmp_g2_gate_blend_f32 launch, under autograd with tau saved and msmp_g2_gate_blend_bwd_f32 as
 *             its backward; 0: PyTorch-ROCm ops around msmp_scatter_mean_f32 (about 14 launches and five [E, width] tensors per pair),
 *             differentiated by torch.autograd (the entries themselves do not read the key; any value other than 0 selects the kernels).  CPU
 *             tensors, float64 and widths the entries refuse by value keep the PyTorch ops.  Measured: DESIGN.md section 4.27.
 *   "tile_arith" 1 (default): ranged tiles take their node rows by arithmetic on tile_halo; 0: always through the node list.
 *   "tile_align" 0 (default): the host cuts the node tiles of a batch of identical graphs at graph boundaries only where tile_nodes divides
 *             the graph size; 1: also where it does not (bitwise graph-order / sharding equivariance on knn graphs, 11-20 % more tiles
 *             there).  No entry point reads the key.
 *   "tail"    1 (default): msmp_mp_layer_f32 uses msmp_node_tail_f32 for graphs of up to 128 nodes; 0: the piecewise kernels.
 *   "pair"    gated pair: both heads' projection / message kernels in one launch each (bit-identical results): 0 never,
 *             1 (default) for batches of up to 65 536 nodes, where a step is bound by the latency of its ~60 dependent launches, 2 always. */
int msmp_tune(const char* key, int value);
int msmp_tune_query(const char* key);

/* ---------------------------------------------------------------------------------------------
 * Weights
 * ------------------------------------------------------------------------------------------- */
/* Number of floats of one packed layer for a given u-feature width `tw` (25; 50 for *2D) and
 * variable count `nv` = len(eq_variables)+1. */
int64_t msmp_packed_layer_floats(int tw, int nv);

/* Pack message_net_1/2 and update_net_1/2 of one GNN_Layer / GNN_LayerLin
 * (experiments/models_gnn.py:47-58, 112-121) into the kernel layout.  w1 [128, 256+tw+1+nv],
 * w2 [128,128], w3 [128, 256+nv], w4 [128,128], b* [128]; all device pointers, reference layout. */
int msmp_pack_layer_f32(const float* w1, const float* b1, const float* w2, const float* b2,
                        const float* w3, const float* b3, const float* w4, const float* b4,
                        int tw, int nv, float* packed_out, msmp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Graph structure (rows G1 of SURVEY section 8a)
 * ------------------------------------------------------------------------------------------- */
/* CSR-by-target from the reference's edge_index [2,E] int64 (row 0 source j, row 1 target i;
 * torch_geometric MessagePassing flow='source_to_target', experiments/models_gnn.py:65,128).
 * Writes rowptr [N+1], col [E] (source of each edge, grouped by ascending target, original relative
 * order kept inside a target) and tgt [E] (target of each CSR slot).  If the input is already grouped
 * by ascending target (what the graph builders emit) no sort is needed; otherwise a stable device
 * sort runs in `workspace` (size from msmp_build_csr_workspace_bytes). */
size_t msmp_build_csr_workspace_bytes(int64_t n_edges, int64_t n_nodes);
int msmp_build_csr(const int64_t* edge_index, int64_t n_edges, int64_t n_nodes,
                   int32_t* rowptr_out, int32_t* col_out, int32_t* tgt_out,
                   void* workspace, size_t workspace_bytes, msmp_stream_t stream);

/* torch_cluster.radius_graph(x, r, batch, loop=False, max_num_neighbors) as called at
 * common/utils.py:368, on `dim`-column float64 coordinates x [N,dim]; graph g owns nodes
 * graph_ptr[g]..graph_ptr[g+1]-1.  Pair (j -> i) kept iff same graph, i != j and squared distance
 * < r*r (float64, strict); at most max_neighbors sources per target, lowest index first.
 * Two calls: _count writes rowptr [N+1] (in-degree prefix sums; E = rowptr[N]); _fill writes
 * edge_index [2,E] int64 in canonical order (ascending target, then ascending source). */
int msmp_radius_graph_count_f64(const double* x, int dim, const int32_t* graph_ptr, int64_t n_graphs,
                                int64_t n_nodes, double r, int max_neighbors,
                                int32_t* rowptr_out, msmp_stream_t stream);
int msmp_radius_graph_fill_f64(const double* x, int dim, const int32_t* graph_ptr, int64_t n_graphs,
                               int64_t n_nodes, double r, int max_neighbors, const int32_t* rowptr,
                               int64_t n_edges, int64_t* edge_index_out, msmp_stream_t stream);

/* torch_cluster.knn_graph(x, k, batch, loop=False) as called at common/utils.py:377,380: per target
 * its min(k, n_g-1) nearest same-graph nodes, ascending float64 squared distance, ties -> lower
 * index.  rowptr [N+1] and edge_index [2,E] are both written; E = sum_g n_g*min(k, n_g-1) is known
 * to the caller from graph sizes and passed as n_edges (writes past it are suppressed). */
int msmp_knn_graph_f64(const double* x, int dim, const int32_t* graph_ptr, int64_t n_graphs,
                       int64_t n_nodes, int k, int64_t n_edges, int32_t* rowptr_out,
                       int64_t* edge_index_out, msmp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Message-passing layer pieces (rows L1-L5)
 * ------------------------------------------------------------------------------------------- */
/* L1  GNN_Layer.message / GNN_LayerLin.message, experiments/models_gnn.py:69-75 / 132-138, with the
 * PyG gathers of propagate (:65,128) fused in:
 *   msg[e] = Swish(W2 Swish(W1 [h_i, h_j, u_i-u_j, pos_i-pos_j, vars_i] + b1) + b2),
 * i = tgt[e], j = col[e].  h [N,128], u [N,tw], pos [N] (= pos_x), vars [N,nv], msg_out [E,128]. */
int msmp_edge_mlp_f32(const float* h, const float* u, const float* pos, const float* vars,
                      const int32_t* tgt, const int32_t* col, int64_t n_nodes, int64_t n_edges,
                      int tw, int nv, const float* packed, float* msg_out, msmp_stream_t stream);

/* L1 + L2 fused: agg[i] = mean over the in-edges of i of the message above, without materialising the
 * [E,128] message tensor (messages are reduced per target inside the workgroup, in CSR order).  Needs
 * every target's in-edges to fit one workgroup tile: max_in_degree <= 256, else MSMP_ERR_UNSUPPORTED
 * (then use msmp_edge_mlp_f32 + msmp_scatter_mean_f32). */
int msmp_edge_aggregate_f32(const float* h, const float* u, const float* pos, const float* vars,
                            const int32_t* rowptr, const int32_t* col, const int32_t* tgt,
                            int64_t n_nodes, int64_t n_edges, int max_in_degree, int tw, int nv,
                            const float* packed, float* agg_out, msmp_stream_t stream);

/* Per-node factorisation of message_net_1 (linear in its concatenated input):
 *   W1 [h_i, h_j, u_i-u_j, p_i-p_j, v_i] + b1 = P[i] + Q[j],
 *   P[n] = W1[:, 0:128] h_n + W1[:, 256:] [u_n, p_n, v_n] + b1,   Q[n] = W1[:, 128:256] h_n - W1[:, 256:] [u_n, p_n, 0].
 * msmp_node_project_f32 writes P and Q [N,128]; msmp_edge_aggregate_projected_f32 then computes the same
 * agg as msmp_edge_aggregate_f32 from them (5.3x fewer FLOPs in message_net_1; only the place where partial
 * sums are rounded differs).  This is the default inside msmp_mp_layer_f32. */
int msmp_node_project_f32(const float* h, const float* u, const float* pos, const float* vars,
                          int64_t n_nodes, int tw, int nv, const float* packed, float* p_out,
                          float* q_out, msmp_stream_t stream);
int msmp_edge_aggregate_projected_f32(const float* p, const float* q, const int32_t* rowptr,
                                      const int32_t* col, const int32_t* tgt, int64_t n_nodes,
                                      int64_t n_edges, int max_in_degree, int tw, int nv,
                                      const float* packed, float* agg_out, msmp_stream_t stream);

/* Node tiles for the LDS-staged message kernel (north_star: "LDS staging of node tiles for edge gather"; the gathers it
 * replaces are PyG propagate's x_i = x[edge_index[1]], x_j = x[edge_index[0]], experiments/models_gnn.py:65,128).
 * A tile = four WAVE GROUPS of `group_nodes` consecutive TARGET nodes each (tile_nodes = 4 group_nodes) with all their in-edges
 * (at most 32 per group: one lane per edge, a target's edges never straddle two waves, so the per-target mean is one more MFMA
 * on the wave's message tile) plus every node those edges read as a source: at most MSMP_TILE_NCAP distinct nodes, listed per
 * tile with the targets first (slot k < tile size is node tile * tile_nodes + k), so the kernel loads each node row of a tile
 * ONCE (coalesced, 512-byte rows) into LDS and every edge reads its two operands from there through the per-edge slot pair.
 * Works for any graph whose tiles fit (banded 1-D radius / knn graphs, periodic wrap-around included: the list is by node id, not
 * by window); msmp_build_tiles reports the largest list / group edge count it met so the caller can pick a smaller group_nodes
 * or fall back to the gather kernels (always for in-degrees above 32). */
#define MSMP_TILE_NCAP  32       /* distinct nodes of a tile: one 32-row MFMA block */
#define MSMP_TILE_EDGES 128      /* edge lanes of a tile: one 32-lane group per wave */
typedef struct {
    int32_t tile_nodes;          /* target nodes per tile = 4 * group_nodes */
    int32_t group_nodes;         /* target nodes per wave group */
    int32_t n_tiles;             /* ceil(n_nodes / tile_nodes) */
    const int32_t* tile_node;    /* [n_tiles][MSMP_TILE_NCAP] node ids (unused slots repeat the tile's first node) */
    const int32_t* tile_count;   /* [n_tiles] number of valid slots */
    const int32_t* tile_halo;    /* [n_tiles][4]: (lo start, lo count, hi start, hi count) when the tile's sources outside it are one
                                  * run of consecutive nodes below and one above (slots then follow node order and the kernel needs
                                  * no list lookup); lo count = -1 otherwise */
    const int32_t* edge_slot;    /* [n_tiles][MSMP_TILE_EDGES]: lane 32 g + k = k-th in-edge (CSR order) of wave group g: target slot | source slot << 8;
                                  * 0 at lanes without an edge */
    int32_t listed;              /* != 0: some tile is not "ranged" (msmp_build_tiles' stats[2] > 0): the kernels read every slot's node
                                  * from tile_node; 0: they compute it from tile_halo and never touch the list */
    int32_t period_tiles;        /* 0: the arrays above describe all n_tiles tiles of the batch.  > 0 (ABI 400): the batch is
                                  * n_nodes / period_nodes copies of ONE pattern (the reference's batches: the same grid for every
                                  * sample, common/utils.py:364-380), the arrays hold the period_tiles tiles of one copy (built from
                                  * its CSR, node ids 0 .. period_nodes - 1; tile_nodes need not divide period_nodes: the last tile of
                                  * a copy is short, so no tile straddles two graphs) and tile t of the launch uses entry
                                  * t mod period_tiles with node ids shifted by (t div period_tiles) * period_nodes.  n_tiles is still the
                                  * launch's tile count.  rowptr passed beside such a descriptor is the whole batch's. */
    int32_t period_nodes;
} msmp_tiles_t;
/* stats_out (device, 3 x int32): largest node list, largest edge count of a wave group over the tiles (lists longer than
 * MSMP_TILE_NCAP are truncated in the output, groups of more than 32 edges cut: the structure is then not usable with this
 * group_nodes), number of tiles that are not ranged (-> msmp_tiles_t.listed). */
int msmp_build_tiles(const int32_t* rowptr, const int32_t* col, int64_t n_nodes, int64_t n_edges, int group_nodes,
                     int32_t* tile_node_out, int32_t* tile_count_out, int32_t* tile_halo_out, int32_t* edge_slot_out,
                     int32_t* stats_out, msmp_stream_t stream);
/* L1 + L2 on node tiles: same result as msmp_edge_aggregate_projected_f32 (p, q given: the tile's P / Q rows are staged in
 * LDS) or, with p == q == NULL, as msmp_node_project_f32 + msmp_edge_aggregate_projected_f32 in ONE launch: the tile's h / u /
 * pos / vars rows are staged in LDS, P and Q of the tile's nodes are computed there (halo nodes recomputed per tile) and never
 * touch HBM.  feat (may be NULL): the packed [u | pos | vars] rows of msmp_pack_node_features_f32; they are the same for every
 * layer of a forward, so packing them once saves each layer's tile staging the scalar loads of those columns.
 * Folded form (p == q == NULL): tw + 1 + nv <= 128 (up to four 32-column tail chunks); the staged form takes any width.
 * msmp_node_feature_stride: 32 x the tail chunks (-1 for invalid sizes); msmp_prepare_nodes accepts strides up to 128. */
int msmp_node_feature_stride(int tw, int nv);
/* Feature preparation of Solver.forward (experiments/models_gnn.py:1325-1352; models_gnn2D.py:104-116) in one launch: x [N,tw] and
 * pos [N,2] = (t, x) in float32 or float64 (*_f64 flags), n_cols per-node parameter columns [N] (`cols`, `col_f64`, host arrays)
 * each divided by col_div (1 for the boundary-condition flags) ->  u = float(x), pos_x = float(pos[:,1] / L),
 * pos_t = float(pos[:,0] / tmax), vars [N, 1 + n_cols] = [pos_t | cols / div], and, if feat_out != NULL, the packed rows of
 * msmp_pack_node_features_f32.  Divisions are evaluated in the input's dtype, like the tensor expressions they replace. */
int msmp_prepare_nodes(const void* x, int x_f64, const void* pos, int pos_f64, int64_t n_nodes, int tw, double L, double tmax,
                       int n_cols, const void* const* cols, const int* col_f64, const double* col_div, float* u_out,
                       float* pos_x_out, float* pos_t_out, float* vars_out, float* feat_out, msmp_stream_t stream);
int msmp_pack_node_features_f32(const float* u, const float* pos, const float* vars, int64_t n_nodes, int tw, int nv,
                                float* feat_out, msmp_stream_t stream);
int msmp_edge_aggregate_tiled_f32(const float* h, const float* u, const float* pos, const float* vars, const float* feat,
                                  const float* p, const float* q, const int32_t* rowptr, const msmp_tiles_t* tiles, int64_t n_nodes,
                                  int64_t n_edges, int tw, int nv, const float* packed, float* agg_out, msmp_stream_t stream);

/* L2  PyG aggr='mean' (torch_scatter scatter-mean; experiments/models_gnn.py:42,107):
 *   agg[i] = sum_{e in CSR row i} msg[e] / max(deg_i, 1), fixed summation order (CSR order). */
int msmp_scatter_mean_f32(const float* msg, const int32_t* rowptr, int64_t n_nodes,
                          float* agg_out, msmp_stream_t stream);

/* L3  update(): experiments/models_gnn.py:77-86 (MSMP_LAYER_RESIDUAL_SWISH) / 140-149 (MSMP_LAYER_LIN)
 * on [h, agg, vars]. */
int msmp_node_update_f32(const float* h, const float* agg, const float* vars, int64_t n_nodes, int nv,
                         const float* packed, int mode, float* out, msmp_stream_t stream);

/* L4  torch_geometric.nn.InstanceNorm(128) (affine=False, no running stats), experiments/models_gnn.py:
 * 59,66,122,129: per graph g and channel (x-mean)/sqrt(biased var + eps). */
/* Node tail of one layer in one launch: update head(s) + InstanceNorm (+ gated blend), for batches whose graphs have at
 * most 128 nodes (MSMP_ERR_UNSUPPORTED otherwise, and on the fp32-MFMA path: chain the piecewise entry points there).
 *   packed_gate == NULL: out = InstanceNorm(update(h, agg_main))                 GNN_Layer / GNN_LayerLin.forward tail,
 *                                                                                experiments/models_gnn.py:61-67,80-86 / 124-130,143-149
 *   packed_gate != NULL: out = (1 - tau) h + tau Swish(IN(update_main)),  tau = sigmoid(IN(update_gate))       :1366-1368
 * agg_* [N,128] are the mean-aggregated messages of the respective head (msmp_edge_aggregate*_f32); graph_ptr
 * [n_graphs+1]; mode as in msmp_node_update_f32.  The pre-norm tensors stay in registers. */
int msmp_node_tail_f32(const float* h, const float* agg_main, const float* agg_gate, const float* vars,
                       const int32_t* graph_ptr, int64_t n_nodes, int64_t n_graphs, int max_graph_nodes, int nv,
                       const float* packed_main, const float* packed_gate, int mode, float eps, float* out,
                       msmp_stream_t stream);

/* max_graph_nodes = size of the largest graph (0 if unknown): up to 128 nodes the rows of a graph are read once
 * and kept in registers across the three passes; larger graphs use the generic kernels (same results). */
int msmp_instance_norm_f32(const float* x, const int32_t* graph_ptr, int64_t n_graphs,
                           int max_graph_nodes, float eps, float* out, msmp_stream_t stream);

/* L4+L5  gate blend, experiments/models_gnn.py:1204-1207 / 1365-1368 (models_gnn2D.py:267-269, 438-441):
 *   tau = sigmoid(InstanceNorm(gate_pre));  out = (1-tau)*h + tau*Swish(InstanceNorm(main_pre)). */
int msmp_gate_blend_f32(const float* h, const float* gate_pre, const float* main_pre,
                        const int32_t* graph_ptr, int64_t n_graphs, int max_graph_nodes, float eps,
                        float* out, msmp_stream_t stream);

/* One whole message-passing layer: GNN_Layer.forward / GNN_LayerLin.forward
 * (experiments/models_gnn.py:61-67 / 124-130) = L1 -> L2 -> L3 -> L4; when packed_gate != NULL the
 * gated pair of one iteration of the solver loop (L5) is evaluated and blended.  h_out may not alias h.
 * max_in_degree = largest CSR row length (pass -1 if unknown): when <= 256 the fused L1+L2 kernel is
 * used, otherwise the message tensor goes through the workspace; max_graph_nodes as in
 * msmp_instance_norm_f32.  Workspace size from msmp_mp_layer_workspace_bytes (same max_in_degree).
 * tiles (may be NULL): node tiles of the structure (msmp_build_tiles); with them rows L1 + L2 run on the LDS-staged tile
 * kernel (msmp_edge_aggregate_tiled_f32, per-node projections folded in), without them on the gather kernels; feat (may be
 * NULL) as in msmp_edge_aggregate_tiled_f32. */
size_t msmp_mp_layer_workspace_bytes(int64_t n_nodes, int64_t n_edges, int gated, int max_in_degree);
int msmp_mp_layer_f32(const float* h, const float* u, const float* pos, const float* vars,
                      const float* feat, const int32_t* rowptr, const int32_t* col, const int32_t* tgt,
                      const msmp_tiles_t* tiles, const int32_t* graph_ptr, int64_t n_nodes, int64_t n_edges, int64_t n_graphs,
                      int max_in_degree, int max_graph_nodes, int tw, int nv, const float* packed_main,
                      const float* packed_gate, int mode,
                      float eps, float* h_out, void* workspace, size_t workspace_bytes,
                      msmp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * LEM node encoder (replaces the absent `lem_cuda` extension)
 * ------------------------------------------------------------------------------------------- */
/* Pack LEMcuda's parameters (experiments/models_gnn.py:305-330: weights [3*128, 128+ninp], weights_lin_z
 * [128, 128+ninp], bias [3*128], bias_lin_z [128]; column block 0..127 multiplies the state, the rest
 * the step input) and optionally lemoutput_mlp.{0,2} (:1287-1291; all four NULL to skip) for
 * msmp_lem_encoder_f32.  ninp <= 8. */
int64_t msmp_packed_lem_floats(void);
int msmp_pack_lem_f32(const float* weights, const float* weights_lin_z, const float* bias,
                      const float* bias_lin_z, const float* mlp_w0, const float* mlp_b0,
                      const float* mlp_w1, const float* mlp_b1, int ninp, float* packed_out,
                      msmp_stream_t stream);

/* Row stride (floats) of the step-input tensor for a given ninp: ninp rounded up to even. */
int msmp_lem_input_stride(int ninp);

/* LEM.forward (experiments/models_gnn.py:340-342 -> lem_cuda.forward :290) on xin [N, T, stride]
 * (node-major; row t = the step input torch.cat((pos_x, u_t, variables)) of :1360, zero padded from ninp
 * to stride = msmp_lem_input_stride(ninp)), zero initial states,
 * followed when with_mlp != 0 by lemoutput_mlp (:1363).  h_out [N,128] = all_y[-1] (or the MLP of it).
 * PARITY UNPINNED against lem_cuda (source absent); follows the published LEM cell. */
int msmp_lem_encoder_f32(const float* xin, int64_t n_nodes, int t_len, int ninp, float dt,
                         const float* packed, int with_mlp, float* h_out, msmp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Decoder
 * ------------------------------------------------------------------------------------------- */
/* 1-D solver decoder, experiments/models_gnn.py:210-224 (output_mlp for time_window 20 / 25 / 50) and
 * :275-279:  out = u[:, -1:] + cumsum(dt) * Conv1d(8,1,k2)(Swish(Conv1d(1,8,k1,stride)(h[:, None, :]))).
 * w1 [8,1,k1], b1 [8], w2 [1,8,k2], b2 [1] in the reference's Conv1d layouts; h [N,128]; u, out [N,tw].
 * u == NULL: out = the decoder output alone (no Euler update), what MSSMP_PDE_Solver_sub returns (:1679-1682). */
int msmp_decoder_f32(const float* h, const float* u, int64_t n_nodes, int tw, const float* w1,
                     const float* b1, const float* w2, const float* b2, float dt, float* out,
                     msmp_stream_t stream);

/* *2D solver decoder, experiments/models_gnn2D.py:79-88 (output_mlp for time_window 25 / 50) and :125-141 after
 * double_mlp:  out = u + cumsum(dt) * Conv1d(8,2,k2)(Swish(Conv1d(2,8,k1,stride)(hd))), hd [N,2,128] = double_mlp(h);
 * w1 [8,2,k1], b1 [8], w2 [2,8,k2], b2 [2]; u, out [N, 2*tw] (component-major). */
int msmp_decoder2d_f32(const float* hd, const float* u, int64_t n_nodes, int tw, const float* w1,
                       const float* b1, const float* w2, const float* b2, float dt, float* out,
                       msmp_stream_t stream);

/* Gated CNN decoder of the GLU classes (hidden width 164, time_window 25), the two networks and the gated Euler update in one launch.
 * 1-D, experiments/models_gnn.py:1455-1456 (output_mlp_gate / output_mlp_diff) and :1514-1521:
 *   scale = Conv1d(8,1,15)(Swish(Conv1d(1,8,6,stride 2)(h[:, None, :82]))),  diff = the same of output_mlp_diff on h[:, None, 82:],
 *   out = (1 - scale) * u[:, -1:] + cumsum(dt) * (scale * diff)              (no sigmoid on scale, as in the reference).
 * h: rows of `width` floats at a row stride of ld floats (ld >= width; no alignment beyond that of a float); u, out [N, tw].
 * gate_* / diff_*: w1 [8,1,6], b1 [8], w2 [1,8,15], b2 [1] of the two networks in the reference's Conv1d layouts.
 * Any (width, tw) other than (164, 25) returns MSMP_ERR_UNSUPPORTED before anything is launched (the reference defines no other);
 * null pointers, n_nodes outside 1 .. 2^31 - 1 and ld < width return MSMP_ERR_ARG.  Plain fp32 arithmetic: no range status. */
int msmp_decoder_gated_f32(const float* h, int ld, const float* u, int64_t n_nodes, int width, int tw, const float* gate_w1,
                           const float* gate_b1, const float* gate_w2, const float* gate_b2, const float* diff_w1, const float* diff_b1,
                           const float* diff_w2, const float* diff_b2, float dt, float* out, msmp_stream_t stream);

/* The same for the 2-D GLU class, experiments/models_gnn2D.py:1291-1298 and :1355-1366, after double_mlp:
 *   scale = Conv1d(8,2,15)(Swish(Conv1d(2,8,6,stride 2)(hd[:, :, :82]))),  diff = the same of output_mlp_diff on hd[:, :, 82:],
 *   out = (1 - scale) * unflatten(u) + cumsum(dt) * scale * diff, flattened back to [N, 2*tw]   (every column of u).
 * hd: per node two component rows of `width` floats, component 1 `width` floats after component 0, nodes ld floats apart
 * (ld >= 2 * width: msmp_linear_f32 writes double_mlp at ld = 384 and the decoder reads it in place); u, out [N, 2*tw] (component-major).
 * gate_* / diff_*: w1 [8,2,6], b1 [8], w2 [2,8,15], b2 [2].  Refusals as above, with ld < 2 * width. */
int msmp_decoder2d_gated_f32(const float* hd, int ld, const float* u, int64_t n_nodes, int width, int tw, const float* gate_w1,
                             const float* gate_b1, const float* gate_w2, const float* gate_b2, const float* diff_w1, const float* diff_b1,
                             const float* diff_w2, const float* diff_b2, float dt, float* out, msmp_stream_t stream);

/* The decoders under autograd: forward-for-training entries and one backward call each.
 * msmp_decoder*_train_fwd_f32 have the prototypes, the kernels and the bits of their inference twins above; they only stay outside the
 * event bracket of the DECODER family (msmp_timing_*), which keeps counting no-grad forwards alone. */
int msmp_decoder_train_fwd_f32(const float* h, const float* u, int64_t n_nodes, int tw, const float* w1,
                               const float* b1, const float* w2, const float* b2, float dt, float* out, msmp_stream_t stream);
int msmp_decoder2d_train_fwd_f32(const float* hd, const float* u, int64_t n_nodes, int tw, const float* w1,
                                 const float* b1, const float* w2, const float* b2, float dt, float* out, msmp_stream_t stream);
int msmp_decoder_gated_train_fwd_f32(const float* h, int ld, const float* u, int64_t n_nodes, int width, int tw, const float* gate_w1,
                                     const float* gate_b1, const float* gate_w2, const float* gate_b2, const float* diff_w1, const float* diff_b1,
                                     const float* diff_w2, const float* diff_b2, float dt, float* out, msmp_stream_t stream);
int msmp_decoder2d_gated_train_fwd_f32(const float* hd, int ld, const float* u, int64_t n_nodes, int width, int tw, const float* gate_w1,
                                       const float* gate_b1, const float* gate_w2, const float* gate_b2, const float* diff_w1, const float* diff_b1,
                                       const float* diff_w2, const float* diff_b2, float dt, float* out, msmp_stream_t stream);

/* Backward of the decoders: from grad_out (the gradient of `out`, same shape), the forward's inputs and weights to dh (the gradient of the
 * rows, COMPACT whatever the forward's row stride: [N,128], [N,2,128], [N,164], [N,2,164]) and the gradients of the weights in the layouts of
 * the weights.  Every element of every output is written, nothing is accumulated; no gradient for u or dt.  Nothing the forward computed is
 * needed: the Swish pre-activations (gated: both networks' outputs too) are recomputed from the rows.  Plain fp32 fmaf: no range status.
 * One launch of at most 512 workgroups (16 nodes per pass, grid-stride beyond 8 192 nodes), each writing its sums of the weight gradients to
 * its own row of `workspace`, then a second small launch that adds the rows in a fixed order: no atomics, no memset, no synchronisation,
 * capturable, the same bits on every call; a node's dh row depends on that node's row, its grad_out row and the weights only.
 * workspace: msmp_decoder_bwd_workspace_bytes(comps (1 | 2), gated (0 | 1), width, tw) bytes, independent of n_nodes (512 partial rows);
 * 0 for a decoder that does not exist.  MSMP_ERR_WORKSPACE if workspace_bytes is below it.
 * Refusals as the forward entries': null pointers (workspace included) and n_nodes outside 1 .. 2^31 - 1 MSMP_ERR_ARG, any other time
 * window / width MSMP_ERR_UNSUPPORTED before anything is launched, gated: ld < comps * width MSMP_ERR_ARG.
 *   msmp_decoder_bwd_f32:  euler != 0: the forward had a u (out = u[:, -1:] + cumsum(dt) diff: d diff = grad_out cumsum(dt));
 *                          euler == 0: u == NULL there (d diff = grad_out).  tw 20 / 25 / 50.
 *   msmp_decoder2d_bwd_f32: hd [N,2,128], tw 25 / 50.
 *   gated (width 164, tw 25): d scale = grad_out (cumsum(dt) diff - u*), d diff = grad_out cumsum(dt) scale, u* = u[:, -1] in 1-D and
 *                          u[:, co tw + t] in 2-D; dgate_* / ddiff_*: the gradients of the two networks. */
size_t msmp_decoder_bwd_workspace_bytes(int comps, int gated, int width, int tw);
int msmp_decoder_bwd_f32(const float* grad_out, const float* h, int64_t n_nodes, int tw, int euler, const float* w1, const float* b1,
                         const float* w2, const float* b2, float dt, float* dh, float* dw1, float* db1, float* dw2, float* db2,
                         void* workspace, size_t workspace_bytes, msmp_stream_t stream);
int msmp_decoder2d_bwd_f32(const float* grad_out, const float* hd, int64_t n_nodes, int tw, const float* w1, const float* b1,
                           const float* w2, const float* b2, float dt, float* dh, float* dw1, float* db1, float* dw2, float* db2,
                           void* workspace, size_t workspace_bytes, msmp_stream_t stream);
int msmp_decoder_gated_bwd_f32(const float* grad_out, const float* h, int ld, const float* u, int64_t n_nodes, int width, int tw,
                               const float* gate_w1, const float* gate_b1, const float* gate_w2, const float* gate_b2, const float* diff_w1,
                               const float* diff_b1, const float* diff_w2, const float* diff_b2, float dt, float* dh, float* dgate_w1,
                               float* dgate_b1, float* dgate_w2, float* dgate_b2, float* ddiff_w1, float* ddiff_b1, float* ddiff_w2,
                               float* ddiff_b2, void* workspace, size_t workspace_bytes, msmp_stream_t stream);
int msmp_decoder2d_gated_bwd_f32(const float* grad_out, const float* hd, int ld, const float* u, int64_t n_nodes, int width, int tw,
                                 const float* gate_w1, const float* gate_b1, const float* gate_w2, const float* gate_b2, const float* diff_w1,
                                 const float* diff_b1, const float* diff_w2, const float* diff_b2, float dt, float* dh, float* dgate_w1,
                                 float* dgate_b1, float* dgate_w2, float* dgate_b2, float* ddiff_w1, float* ddiff_b1, float* ddiff_w2,
                                 float* ddiff_b2, void* workspace, size_t workspace_bytes, msmp_stream_t stream);

/* `double_mlp` of the *2D solver classes, experiments/models_gnn2D.py:66-70 (nn.Linear(128, 256) + Swish; the Unflatten is a view):
 * out [rows, n_out] = Swish(x [rows, k] w^T + bias), w [n_out, k] in nn.Linear's layout; n_out a multiple of 128, k a multiple of 4 up to 288.
 * fp32-exact products on the bf16 matrix pipe.  workspace: msmp_linear_swish_workspace_bytes(k, n_out) bytes (0 = unsupported sizes). */
size_t msmp_linear_swish_workspace_bytes(int k, int n_out);
int msmp_linear_swish_f32(const float* x, int64_t rows, int k, const float* w, const float* bias, int n_out, float* out,
                          void* workspace, size_t workspace_bytes, msmp_stream_t stream);

/* msmp_lem_encoder_f32 with the step inputs assembled in the kernel from the node arrays (no [N, T, ninp] tensor in HBM):
 *   two_d = 0: x_t = [pos_x, u_t, variables]                                experiments/models_gnn.py:1357-1360, ninp = 2 + nv
 *   two_d = 1: x_t = [pos_x, u_t, u_{tw+t}, dt_cum_t + pos_t, variables[1:]]  experiments/models_gnn2D.py:429-433, ninp = 3 + nv
 * u [N, tw] ([N, 2 tw] for two_d), pos_x / pos_t [N], vars [N, nv] (column 0 = pos_t), dt_cum [tw] = cumsum(pde.dt);
 * `packed` from msmp_pack_lem_f32 with that ninp.  MSMP_ERR_UNSUPPORTED on the exact-fp32 path (msmp_tune("split", 0)). */
int msmp_lem_encoder_nodes_f32(const float* u, const float* pos_x, const float* pos_t, const float* vars, const float* dt_cum,
                               int64_t n_nodes, int tw, int nv, int two_d, float dt, const float* packed, int with_mlp,
                               float* h_out, msmp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Training backward of a message-passing layer: the non-GEMM pieces.  The host layer
 * re-evaluates the layer in materialised form with library GEMMs (the reference does the same through autograd over
 * experiments/models_gnn.py:61-149) and calls these between them.
 * ------------------------------------------------------------------------------------------- */
/* The backward of msmp_mp_layer_f32 in one call: given grad_out = dL/d h_out it recomputes the layer (or the gated pair)
 * from its inputs in materialised form and returns dh_out = dL/dh [N,128] and the gradients of the eight parameters of each
 * layer (what torch.autograd produces over experiments/models_gnn.py:61-149 and the blend :1204-1207).  params_* / grads_*:
 * arrays of 8 device pointers in the order message_net_1.0.weight, .bias, message_net_2.0.weight, .bias, update_net_1.0.weight,
 * .bias, update_net_2.0.weight, .bias, in the reference's [out, in] layouts (NOT the packed blobs); gate arrays NULL for a
 * single layer.  u, pos, vars carry no gradient.  GEMMs with edge- / node-sized outputs run on the library's own bf16x3 row-GEMM
 * kernels at every size; only with msmp_tune("bwd_gemm", 0) do they go to rocblas_sgemm, which is then looked up in the process
 * at run time (MSMP_ERR_UNSUPPORTED if librocblas cannot be loaded; never loaded otherwise).  src_rowptr [N+1] / src_perm [E] (both or
 * neither): the CSR edge ids regrouped by SOURCE node, ascending inside a source; with them dh's source-side scatter runs in
 * that fixed order (bitwise reproducible gradients), without them it uses float atomics.  tw + 1 + nv <= 128; above 64 (2-D windows
 * of 50) only with src_rowptr / src_perm and the own GEMMs (tune "bwd_gemm" != 0), else MSMP_ERR_UNSUPPORTED.
 * Workspace: msmp_mp_layer_bwd_workspace_bytes (0 for invalid sizes). */
size_t msmp_mp_layer_bwd_workspace_bytes(int64_t n_nodes, int64_t n_edges, int tw, int nv, int gated);
int msmp_mp_layer_bwd_f32(const float* grad_out, const float* h, const float* u, const float* pos, const float* vars,
                          const int32_t* rowptr, const int32_t* col, const int32_t* tgt, const int32_t* src_rowptr,
                          const int32_t* src_perm, const int32_t* graph_ptr,
                          int64_t n_nodes, int64_t n_edges, int64_t n_graphs, int tw, int nv,
                          const float* const* params_main, const float* const* params_gate, int mode, float eps,
                          float* dh_out, float* const* grads_main, float* const* grads_gate, void* workspace,
                          size_t workspace_bytes, msmp_stream_t stream);

/* Fused AdamW step over all parameter tensors (experiments/train.py:410: optim.AdamW(model.parameters(), lr=args.lr); PyTorch
 * defaults betas (0.9, 0.999), eps 1e-8, weight_decay 1e-2): arrays of n_tensors device pointers (parameter, gradient, first and
 * second moment: fp32, contiguous) and element counts (host array); `step` = 1, 2, ... (bias correction).  One launch per 48
 * tensors.  Same update rule and order of operations as torch.optim.AdamW.  A tensor of 0 elements is legal, as it is for
 * torch.optim.AdamW: its four pointers are not read and may be NULL.  A NULL pointer of any other tensor is MSMP_ERR_ARG. */
int msmp_adamw_f32(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                   float* const* exp_avg_sq, const int64_t* numel, float lr, float beta1, float beta2, float eps,
                   float weight_decay, int64_t step, msmp_stream_t stream);
/* The same step for a captured training iteration (a hipGraph replays fixed kernel arguments): the step count lives in device
 * memory (step_dev[0], int64, advanced by this call) and so does the learning rate (lr_dev[0]; a scheduler's new value is a
 * host-to-device copy between replays).  Bias corrections are computed on the device from step_dev.  Tensors of 0 elements as in
 * msmp_adamw_f32 (pointers may be NULL); step_dev advances once per call whatever the tensors hold. */
int msmp_adamw_capturable_f32(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                              float* const* exp_avg_sq, const int64_t* numel, const float* lr_dev, float beta1, float beta2,
                              float eps, float weight_decay, int64_t* step_dev, msmp_stream_t stream);

/* verdict bits of msmp_grads_finite_f32 */
#define MSMP_NONFINITE_GRAD   1   /* a gradient element is NaN or +-Inf */
#define MSMP_NONFINITE_SCALAR 2   /* a watched scalar is NaN or +-Inf */
/* The guard of a training step.  The reference's loop (experiments/train_helper.py:125-141, optimizer of experiments/train.py:410) has none
 * and needs none: its model has no input range.  Here a forward that leaves the range of the fp16-split path, or a NaN in a label, gives
 * a non-finite loss, and AdamW would write the non-finite gradients into every weight and both moments.  The three entries below
 * refuse such an update on the device: no atomics, no memset, no host read-back, so a captured (hipGraph) step stays a graph.
 * All three return MSMP_ERR_ARG for a null pointer or a bad count before anything is launched.
 *
 * msmp_grads_finite_f32: verdict_dev[0] (int32, overwritten by every call) = 0 if every element of the n_tensors gradient tensors
 * (device pointers and host element counts as msmp_adamw_f32; 48 descriptors per launch, 4096 elements per block) and every one of the
 * n_scalars (0 .. 4) single-float device scalars (the loss) is finite, else MSMP_NONFINITE_GRAD | MSMP_NONFINITE_SCALAR as they apply.
 * NaN and +-Inf are not finite; FLT_MAX, denormals and zeros are.  The pointer of a tensor
 * of 0 elements is not read and may be NULL.  Two launches per call (one more per further 48 tensors): every block
 * overwrites its own word of workspace (>= msmp_grads_finite_workspace_bytes(n_tensors, numel) bytes, else MSMP_ERR_WORKSPACE; the query
 * returns 0 for arguments the entry refuses), the final block overwrites the verdict. */
size_t msmp_grads_finite_workspace_bytes(int n_tensors, const int64_t* numel);
int msmp_grads_finite_f32(int n_tensors, const float* const* grads, const int64_t* numel, int n_scalars, const float* const* scalars,
                          int32_t* verdict_dev, void* workspace, size_t workspace_bytes, msmp_stream_t stream);
/* msmp_adamw_capturable_f32 (experiments/train.py:410) behind that verdict: with verdict_dev[0] == 0 the same launches on the same
 * arithmetic (bit for bit, step_dev advanced by one); with any other value no parameter, moment or step_dev byte changes and
 * skipped_dev[0] (int64) advances by one.  Tensors of 0 elements as in msmp_adamw_f32: their pointers may be NULL. */
int msmp_adamw_guarded_f32(int n_tensors, float* const* params, const float* const* grads, float* const* exp_avg,
                           float* const* exp_avg_sq, const int64_t* numel, const float* lr_dev, float beta1, float beta2,
                           float eps, float weight_decay, int64_t* step_dev, const int32_t* verdict_dev, int64_t* skipped_dev,
                           msmp_stream_t stream);
/* The sticky range status (msmp_last_status) as a value in the stream: if the word is not 0 when this one-wave kernel runs, scalar[0]
 * becomes a quiet NaN (the loss sum of experiments/train_helper.py:125-141, before the data-parallel all-reduce: every rank then takes the
 * same decision).  The word is read with a system-scope atomic load; the kernels that raise it do so with system-scope atomic ORs, so
 * stream order is enough.  Without a status word (its allocation failed) nothing is launched. */
int msmp_status_poison_f32(float* scalar, msmp_stream_t stream);

/* A training batch from a device-resident dataset in ONE launch: GraphCreator.create_data + create_graph (common/utils.py:300-428;
 * mode 0) or the label / time half of create_next_graph (common/utils.py:431-471, 454-469; mode 1), with the sample and step indices
 * read on the device (experiments/train_helper.py:94-112 draws them per iteration).
 *   store      [n_samples, nt, comps, nx] fp32: the downprojected split in the per-sample layout of HDF5Dataset.__getitem__
 *              (common/utils.py:156-264); comps = 2 for the AD / *2D experiments, else 1;
 *   sample_idx, steps   [batch] int32 DEVICE arrays;   t_axis [nt], x_grid [nx];   var_table [n_samples, n_vars] (NULL at n_vars = 0).
 * For graph b with s = sample_idx[b], p = steps[b], node i < nx, component c < comps, k < tw:
 *   x_out[b nx + i, c tw + k] = store[s, p - tw + k, c, i]      ([batch nx, comps tw], component-major as GraphCreator._flatten, :350-357)
 *   y_out[b nx + i, c tw + k] = store[s, p + k, c, i]
 *   pos_out[b nx + i]         = (t_axis[p], x_grid[i])          ([batch nx, 2])
 *   vars_out[v batch nx + b nx + i] = var_table[s, v]           (n_vars contiguous columns of batch nx floats)
 * mode 1 writes y_out and column 0 of pos_out only (column 1 keeps its bytes); x_out, x_grid, var_table and vars_out may be NULL.
 * The indices live on the device, so the entry cannot refuse a bad one; the kernel never reads outside `store`: a graph whose s is
 * outside 0 .. n_samples - 1 or whose p is outside tw .. nt - tw gets quiet-NaN rows in x_out and y_out (a NaN loss, which
 * msmp_adamw_guarded_f32 skips), pos / vars rows from t_axis[clamp(p, tw, nt - tw)] and row clamp(s, 0, n_samples - 1), and every
 * other graph of the batch is unaffected.  Refused by value before anything is launched -- MSMP_ERR_ARG: a null pointer; batch, nx,
 * nt or n_samples outside 1 .. 2^31 - 1; batch nx >= 2^31; comps not 1 or 2; n_vars outside 0..3; mode not 0 or 1.
 * MSMP_ERR_UNSUPPORTED: tw outside 1..64, or nt < 2 tw.  No allocation, no synchronisation, no atomics, no memset: only pointers and
 * sizes are baked into the launch, so a captured one replayed after sample_idx / steps were overwritten assembles the new batch. */
int msmp_batch_assemble_f32(const float* store, int64_t n_samples, int nt, int comps, int nx, const int32_t* sample_idx,
                            const int32_t* steps, int batch, int tw, const float* t_axis, const float* x_grid, const float* var_table,
                            int n_vars, int mode, float* x_out, float* y_out, float* pos_out, float* vars_out, msmp_stream_t stream);

/* One rollout step of the reference's evaluation loops (experiments/train_helper.py:150-296 test_timestep_losses / test_unrolled_losses,
 * :362-471 compute_L2_norms) in ONE launch: the squared error of a prediction against the labels of its window, read straight from
 * the store of msmp_batch_assemble_f32 (no label tensor is made), the squared norm of those labels, and the time column
 * create_next_graph (common/utils.py:454-469) writes for the next window.
 *   store, sample_idx, steps, t_axis   as in msmp_batch_assemble_f32 (t_axis may be NULL when pos_out is NULL);
 *   pred       [batch nx, comps tw] fp32: the model's output for the windows starting at steps[b];
 *   err_out, nrm_out   float64, row b at + b ld (ld >= comps tw; the padding keeps its bytes);   pos_out [batch nx, 2] fp32 or NULL.
 * For graph b with s = sample_idx[b], p = steps[b], component c < comps, k < tw, and y_i = store[s, p + k, c, i]:
 *   d_i = pred[b nx + i, c tw + k] - y_i                         (formed in fp32, as the reference's `pred - graph.y`)
 *   err_out[b ld + c tw + k] = sum_i (double)d_i (double)d_i
 *   nrm_out[b ld + c tw + k] = sum_i (double)y_i (double)y_i      (the reference squares the label, train_helper.py:401)
 *   pos_out[2 (b nx + i)]    = t_axis[p + tw]   if p + tw <= nt - tw; otherwise column 0 keeps its bytes.  Column 1 is never touched.
 * Accumulation is float64 in a fixed order that depends on neither the grid nor `batch` (graph b's numbers are the same bits in any
 * batch): with KP the power of two >= tw and NS = min(64, 256 / KP), a column is NS partial sums -- partial j takes the nodes i with
 * (i mod 64) mod NS == j in ascending i -- added in ascending j.
 * The indices live on the device, so the entry cannot refuse a bad one; the kernel never reads outside `store`: a graph whose s is
 * outside 0 .. n_samples - 1 or whose p is outside tw .. nt - tw gets quiet NaNs in its comps tw entries of err_out and nrm_out, its
 * pos_out rows (where written) come from clamp(p, tw, nt - tw), and every other graph is unaffected.  Refused by value before
 * anything is launched -- MSMP_ERR_ARG: a null store, sample_idx, steps, pred, err_out or nrm_out; a null t_axis with a pos_out;
 * batch, nx, nt or n_samples outside 1 .. 2^31 - 1; batch nx >= 2^31; comps not 1 or 2; ld < comps tw.  MSMP_ERR_UNSUPPORTED: tw
 * outside 1..64, or nt < 2 tw.  No allocation, no synchronisation, no atomics, no memset: only pointers and sizes are baked into the
 * launch, so a captured one replayed after steps, sample_idx or pred were overwritten evaluates the new window. */
int msmp_eval_window_f32(const float* store, int64_t n_samples, int nt, int comps, int nx, const int32_t* sample_idx,
                         const int32_t* steps, int batch, int tw, const float* pred, const float* t_axis, double* err_out,
                         double* nrm_out, int64_t ld, float* pos_out, msmp_stream_t stream);

/* Deterministic reductions for the PyTorch-side pieces of a training iteration (bias gradients of the encoder / decoder, the
 * loss of experiments/train_helper.py:125-141): fixed summation order, two kernel launches, no atomics, no memset -- safe inside a
 * captured (hipGraph) training step.  workspace >= msmp_reduce_workspace_bytes(cols) (cols = 1 for the scalar sum).
 *   msmp_colsum_f32:    out[j] = sum over rows r and columns c in [j group, (j + 1) group) of x[r][c]   (x [rows, cols] row-major)
 *   msmp_sqerr_sum_f32: out[0] = sum_i (a[i] - b[i])^2 */
size_t msmp_reduce_workspace_bytes(int cols);
int msmp_colsum_f32(const float* x, int64_t rows, int cols, int group, float* out, void* workspace, size_t workspace_bytes,
                    msmp_stream_t stream);
int msmp_sqerr_sum_f32(const float* a, const float* b, int64_t n, float* out, void* workspace, size_t workspace_bytes,
                       msmp_stream_t stream);

/* The per-edge input of message_net_1 (models_gnn.py:69-75): out[e] = cat(h[i], h[j], u[i]-u[j], pos[i]-pos[j], vars[i]),
 * i = tgt[e], j = col[e]; out [E, ld] with ld >= 256 + tw + 1 + nv a multiple of 4 (columns past the concat are not written);
 * tw + 1 + nv <= 128. */
int msmp_edge_concat_f32(const float* h, const float* u, const float* pos, const float* vars, const int32_t* tgt,
                         const int32_t* col, int64_t n_edges, int tw, int nv, int ld, float* out, msmp_stream_t stream);
/* Backward of aggr='mean' (:42,107) fused with the derivative of message_net_2's Swish:
 *   out[e] = dagg[tgt[e]] / max(deg(tgt[e]), 1) * Swish'(a2[e]),  a2 [E,128] the pre-activation of message_net_2. */
int msmp_mean_bwd_dswish_f32(const float* dagg, const int32_t* rowptr, const int32_t* tgt, const float* a2, int64_t n_edges,
                             float* out, msmp_stream_t stream);
/* Backward of msmp_instance_norm_f32 (PyG InstanceNorm, :59,66): x the normalised tensor's input, grad_y = dL/dy. */
int msmp_instance_norm_bwd_f32(const float* x, const float* grad_y, const int32_t* graph_ptr, int64_t n_graphs, float eps,
                               float* dx_out, msmp_stream_t stream);
/* Backward of msmp_gate_blend_f32 (:1204-1207) through both InstanceNorms: grad_out = dL/d out ->
 * d_gate_pre, d_main_pre (gradients of the two pre-norm tensors) and dh_out = the direct (1 - tau) path to h. */
int msmp_gate_blend_bwd_f32(const float* grad_out, const float* h, const float* gate_pre, const float* main_pre,
                            const int32_t* graph_ptr, int64_t n_graphs, float eps, float* d_gate_pre, float* d_main_pre,
                            float* dh_out, msmp_stream_t stream);

/* Weight and bias gradients of up to 8 linear layers in one call (two launches):
 *   out_w[i] [128, k2] = a[i]^T b[i][:, :k2],  out_b[i] [128] = column sums of a[i];  a[i] [rows, 128] (row stride lda >= 128) =
 *   dL/d(pre-activation), b[i] [rows, k2] (row stride ldb >= k2, k2 <= 319) = that layer's input.  Exact-fp32 MFMA partial
 *   products over row splits, summed in a fixed order (deterministic).  workspace: msmp_grad_weights_workspace_floats floats. */
int64_t msmp_grad_weights_workspace_floats(int n_jobs, const int64_t* rows, const int* k2);
int msmp_grad_weights_f32(int n_jobs, const float* const* a, const float* const* b, const int64_t* rows, const int* lda,
                          const int* ldb, const int* k2, float* const* out_w, float* const* out_b, float* workspace,
                          int64_t workspace_floats, msmp_stream_t stream);
/* The same with B given as the virtual column concatenation [b | b2] (columns >= ksplit[i] of job i come from b2[i], row stride ldb2[i]):
 * the LEM weight gradients multiply d gates with [y_{t-1} ; x_t] and [z_t ; x_t], which live in two tensors (lem_cuda.backward,
 * experiments/models_gnn.py:296-302); b2[i] == NULL: the job is as in msmp_grad_weights_f32. */
int msmp_grad_weights_cat_f32(int n_jobs, const float* const* a, const float* const* b, const float* const* b2, const int64_t* rows,
                              const int* lda, const int* ldb, const int* ldb2, const int* ksplit, const int* k2, float* const* out_w,
                              float* const* out_b, float* workspace, int64_t workspace_floats, msmp_stream_t stream);

/* Two-layer node MLP  out = Swish(W2 Swish(W1 x + b1) + b2)  in one launch: the `embedding_mlp` encoder of the LEM-free
 * solver classes (experiments/models_gnn.py:196-201 called at :269-270; models_gnn2D.py:66-71 called at :119-120).
 * w1 [128, k_in] (k_in = in_features of the first Linear <= 128), w2 [128,128], b* [128], reference layout.
 * x: [N, msmp_mlp2_input_stride(k_in)] float32, the concatenated node input [u | pos_x | variables] with rows zero-padded
 * to that stride (a multiple of 32 floats); out [N,128]. */
int64_t msmp_packed_mlp2_floats(int k_in);
int msmp_mlp2_input_stride(int k_in);
int msmp_pack_mlp2_f32(const float* w1, const float* b1, const float* w2, const float* b2, int k_in, float* packed_out,
                       msmp_stream_t stream);
int msmp_mlp2_swish_f32(const float* x, int64_t n_nodes, int k_in, const float* packed, float* out, msmp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Width-generic layer pieces: the GLU classes (hidden width 164; experiments/models_gnn.py:1379-1523 MP_PDE_SolverLEMLinGatedGLU,
 * models_gnn2D.py:1198-1366 MP_PDE_Solver2DLEMLinGatedGLU; train.py names 'MSGMP-PDE', 'MSGMP-PDE2D').  The same GNN_LayerLin
 * (message :132-138, mean :107, update :140-149, InstanceNorm :129, gated blend :1486-1489) evaluated from HBM-bound kernels around
 * a general fp32-exact row GEMM; tensors are row-major with row stride ld (a multiple of 4, >= width; padding columns stay 0).
 * ------------------------------------------------------------------------------------------- */
/* out[rows, 0 : 128 ceil(n_out / 128)] = f(x[rows, 0:k] w[n_out, k]^T + bias): mode 0 identity, 1 Swish, 2 out += x w^T (no bias). */
size_t msmp_linear_workspace_bytes(int k, int n_out);
int msmp_linear_f32(const float* x, int ldx, int64_t rows, int k, const float* w, int ldw, const float* bias, int n_out, int mode,
                    float* out, int ld_out, void* workspace, size_t workspace_bytes, msmp_stream_t stream);
/* out[e] = Swish(p[tgt[e]] + q[col[e]])  (message_net_1 factorised per node, then its Swish) */
int msmp_wide_gather_swish_f32(const float* p, const float* q, const int32_t* tgt, const int32_t* col, int64_t n_edges, int width, int ld,
                               float* out, msmp_stream_t stream);
/* PyG aggr='mean' over CSR rows, any width */
int msmp_wide_scatter_mean_f32(const float* msg, const int32_t* rowptr, int64_t n_nodes, int width, int ld, float* agg_out, msmp_stream_t stream);
int msmp_wide_swish_f32(const float* x, int64_t n_floats, float* out, msmp_stream_t stream);
/* The pointwise halves of one LEM time step at any hidden width (the GLU classes' encoder; the cell of experiments/models_gnn.py:285-342,
 * SURVEY 8c), around the two recurrent GEMMs:  g [N, 3 width] = [y, x_t] W^T + b  ->  dtbar_out = dt sigmoid(g1),
 * z <- (1 - dt sigmoid(g2)) z + dt sigmoid(g2) tanh(g3);  then with lin [N, width] = [z, x_t] Wz^T + bz:  y <- (1 - dtbar) y + dtbar tanh(lin). */
int msmp_wide_lem_z_f32(const float* g, int64_t n_nodes, int width, float dt, float* z, float* dtbar_out, msmp_stream_t stream);
int msmp_wide_lem_y_f32(const float* lin, const float* dtbar, int64_t n_floats, float* y, msmp_stream_t stream);
/* The whole T-step recurrence of that cell at any hidden width 1 <= width <= 256 in ONE launch (LEMcuda.forward / LEMFunction.forward,
 * experiments/models_gnn.py:285-342): fp16-split MFMA arithmetic of the default path, weights streamed from L2, states in registers and LDS.
 * Blob size / pack: weights [3 width, width + ninp], weights_lin_z [width, width + ninp], bias [3 width], bias_lin_z [width]; ninp 1..8. */
int64_t msmp_packed_lem_wide_floats(int ninp, int width);      /* 0 (and msmp_last_error) for a width or ninp outside the range */
int msmp_pack_lem_wide_f32(const float* weights, const float* weights_lin_z, const float* bias, const float* bias_lin_z, int ninp, int width,
                           float* packed_out, msmp_stream_t stream);
/* experiments/models_gnn.py:285-342: xin [n_nodes, t_len, msmp_lem_input_stride(ninp)] (node-major step inputs, as msmp_lem_encoder_f32),
 * y0 / z0 [n_nodes, width] the initial states (`states`, :325-332; both NULL = zeros) -> y_out = all_y[-1], z_out = all_z[-1] (or NULL),
 * dense [n_nodes, width].  MSMP_ERR_UNSUPPORTED for width outside 1..256 or ninp outside 1..8, MSMP_ERR_ARG for t_len < 1 or a null
 * required pointer; n_nodes = 0 is a no-op.  A step input with |x| > 255 or not finite raises MSMP_STATUS_INPUT_RANGE. */
int msmp_lem_encoder_wide_f32(const float* xin, int64_t n_nodes, int t_len, int ninp, int width, float dt, const float* packed,
                              const float* y0, const float* z0, float* y_out, float* z_out, msmp_stream_t stream);
/* The TRAINING pair of that cell at any hidden width 1 <= width <= 256, 128 included (lem_wide_train_kernel.hip): it
 * replaces lem_cuda.forward / lem_cuda.backward as LEMFunction uses them (experiments/models_gnn.py:285-302).  The forward is the recurrence
 * (no lemoutput_mlp) that also saves what the backward needs, as the reference saves all_X / all_X2 / all_multi_scales /
 * all_lin_new_z_state; the backward is the back-propagation through time down to dL/d(pre-activations), of which the parameter gradients
 * are GEMMs over the N*T rows:  d weights = dg[g1 | g2 | g3]^T [y_{t-1} | x_t],  d weights_lin_z = dg[lin]^T [z_t | x_t],  d bias* = column
 * sums.  Wp = 32 ceil(width / 32), ldg = 128 ceil(width / 128).  Three-way bf16 split products (fp32-exact): no input range, the range
 * status is neither read nor raised.  Blobs: weights [3 width, width + ninp], weights_lin_z
 * [width, width + ninp], bias [3 width], bias_lin_z [width], ninp 1..8;
 *   msmp_packed_lem_wide_train_floats = 6144 kt^2 + 1152 kt, msmp_packed_lem_wide_bwd_floats = 6144 kt^2 floats (kt = ceil(width / 32)),
 * 0 (and msmp_last_error) for a width or ninp outside the range.  All blobs, `saved` and `dg_out` are 16-byte aligned. */
int64_t msmp_packed_lem_wide_train_floats(int ninp, int width);
int msmp_pack_lem_wide_train_f32(const float* weights, const float* weights_lin_z, const float* bias, const float* bias_lin_z, int ninp,
                                 int width, float* packed_out, msmp_stream_t stream);
int64_t msmp_packed_lem_wide_bwd_floats(int ninp, int width);
int msmp_pack_lem_wide_bwd_f32(const float* weights, const float* weights_lin_z, int ninp, int width, float* packed_out, msmp_stream_t stream);
/* saved [6][n_nodes][t_len][Wp] floats: dt*sigmoid(g2), tanh(g3), dt*sigmoid(g1), tanh(lin), y_{t-1}, z_t (every element is written);
 * dg [n_nodes][t_len][4][ldg] floats.  0 (and msmp_last_error) for a width outside 1..256, n_nodes < 0 or t_len < 1. */
int64_t msmp_lem_wide_saved_floats(int64_t n_nodes, int t_len, int width);
int64_t msmp_lem_wide_dg_floats(int64_t n_nodes, int t_len, int width);
/* xin [n_nodes, t_len, msmp_lem_input_stride(ninp)]; y0 / z0 [n_nodes, width] (both NULL = zeros) -> y_out, z_out (or NULL) dense
 * [n_nodes, width]; saved may be NULL when no backward follows (the state-carrying LEMS under no_grad).  MSMP_ERR_UNSUPPORTED for width
 * outside 1..256 or ninp outside 1..8; MSMP_ERR_ARG for t_len < 1, a null required pointer, one initial state without the other or a
 * misaligned blob / saved; n_nodes = 0 is a no-op. */
int msmp_lem_train_fwd_wide_f32(const float* xin, int64_t n_nodes, int t_len, int ninp, int width, float dt, const float* packed,
                                const float* y0, const float* z0, float* saved, float* y_out, float* z_out, msmp_stream_t stream);
/* grad_y [n_nodes, width] = dL/dy_T -> dg_out: per node and step the gates (g1 | g2 | g3 | lin), ldg columns each, columns width .. ldg - 1
 * written as 0, so every gate is one or two 128-column A operands (row stride 4 ldg) of msmp_grad_weights_cat_f32 with B = [plane 4 (lin:
 * plane 5) of saved, row stride Wp | x_t].  y0 / z0: the forward's initial states (both or none).  Also MSMP_ERR_ARG for dt = 0.  Like the
 * reference's use of it, no gradient of the step inputs is produced (:300-302), nor of the initial states (carried constants, :350-353). */
int msmp_lem_train_bwd_wide_f32(const float* grad_y, const float* saved, const float* y0, const float* z0, int64_t n_nodes, int t_len,
                                int width, float dt, const float* packed_bwd, float* dg_out, msmp_stream_t stream);
/* The LSTM encoder of the LSTM ablation classes (lstm_train_kernel.hip): torch.nn.LSTM(ninp, width) -- one layer, unidirectional, no
 * projection, gate order i, f, g, o (experiments/models_gnn.py:758-767) -- at any hidden width 1 <= width <= 256, for training and
 * inference, in the fp32-exact three-way bf16 split of the LEM pair above (no input range; the range status is neither read nor raised):
 *     G = w_hh h + w_ih x_t + (b_ih + b_hh);  i = s(G_i), f = s(G_f), g = tanh(G_g), o = s(G_o);  c' = f c + i g;  h' = o tanh(c')
 * The forward is the T-step recurrence, saving what the backward needs; the backward is the back-propagation through time down to
 * dL/dG, of which the parameter gradients are GEMMs over the N*T rows:  d w_hh = dg^T h_{t-1},  d w_ih = dg^T x_t,  d b_ih = d b_hh =
 * column sums of dg.  Wp = 32 ceil(width / 32), ldg = 128 ceil(width / 128), kt = ceil(width / 32).  Parameters as torch holds them:
 * w_ih [4 width, ninp], w_hh [4 width, width], b_ih, b_hh [4 width], ninp 1..8;
 *   msmp_packed_lstm_train_floats = 6144 kt^2 + 1152 kt, msmp_packed_lstm_bwd_floats = 6144 kt^2 floats,
 * 0 (and msmp_last_error) for a width or ninp outside the range.  All blobs, `saved` and `dg_out` are 16-byte aligned. */
int64_t msmp_packed_lstm_train_floats(int ninp, int width);
int msmp_pack_lstm_train_f32(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int ninp, int width, float* packed_out,
                             msmp_stream_t stream);
int64_t msmp_packed_lstm_bwd_floats(int ninp, int width);
int msmp_pack_lstm_bwd_f32(const float* w_hh, int ninp, int width, float* packed_out, msmp_stream_t stream);
/* saved [6][n_nodes][t_len][Wp] floats: i, f, g, o, c_t, h_{t-1} (every element is written; channels width .. Wp - 1 of c and h are zeros);
 * dg [n_nodes][t_len][4][ldg] floats.  0 (and msmp_last_error) for a width outside 1..256, n_nodes < 0 or t_len < 1. */
int64_t msmp_lstm_saved_floats(int64_t n_nodes, int t_len, int width);
int64_t msmp_lstm_dg_floats(int64_t n_nodes, int t_len, int width);
/* xin [n_nodes, t_len, msmp_lem_input_stride(ninp)]; h0 / c0 [n_nodes, width] (both NULL = zeros) -> h_out = output[-1], c_out (or NULL)
 * dense [n_nodes, width]; saved NULL: no backward follows (inference: the same bits in h_out / c_out).  MSMP_ERR_UNSUPPORTED for width
 * outside 1..256 or ninp outside 1..8; MSMP_ERR_ARG for t_len < 1, a null required pointer, one initial state without the other or a
 * misaligned blob / saved; n_nodes = 0 is a no-op. */
int msmp_lstm_train_fwd_f32(const float* xin, int64_t n_nodes, int t_len, int ninp, int width, const float* packed, const float* h0,
                            const float* c0, float* saved, float* h_out, float* c_out, msmp_stream_t stream);
/* grad_h [n_nodes, width] = dL/dh_T -> dg_out: per node and step the gates (i | f | g | o), ldg columns each, columns width .. ldg - 1
 * written as 0, so every gate is one or two 128-column A operands (row stride 4 ldg) of msmp_grad_weights_cat_f32 with B = [plane 5 of
 * saved, row stride Wp | x_t].  c0: the forward's initial cell state (NULL = zeros; h0 is in the saved plane).  No gradient of the step
 * inputs is produced, nor of the initial states. */
int msmp_lstm_train_bwd_f32(const float* grad_h, const float* saved, const float* c0, int64_t n_nodes, int t_len, int width,
                            const float* packed_bwd, float* dg_out, msmp_stream_t stream);
/* The gradient gate (G2) of MP_PDE_Solver2DLEMLinG2 between the two layer calls of a pair (g2_gate_kernel.hip; experiments/models_gnn2D.py:598-611).
 * h, gate (the gate layer's output after its InstanceNorm), main (the main layer's output), out, tau_out and every row tensor of the
 * backward are [n_nodes, ld] fp32, 16-byte aligned, ONE row stride ld for all of them; columns width .. ld - 1 are neither read nor written.
 * out_rowptr [n_nodes + 1] / out_nbr [n_edges]: node i's out-edges as the TARGETS of the edges regrouped by source (GraphStructure.by_source():
 * ascending CSR edge id inside a source); in_rowptr / in_col: the CSR by target of msmp_build_csr (rowptr, col).  With t = Swish(gate) and
 * D_i = max(|out(i)|, 1):
 *     m_i = (1 / D_i) sum_{j in out(i)} (t_i - t_j)^2,   tau_i = tanh(m_i),   out_i = (1 - tau_i) h_i + tau_i Swish(main_i)
 * summed edge by edge in list order (square and add rounded separately), then times 1 / D_i: multi-edges count with their multiplicity, a
 * self-loop contributes an exact 0, a node without out-edges gets tau = 0 and out = h exactly; n_edges = 0 is valid (the list pointers must
 * still be non-null).  One launch; Swish(gate_j) is recomputed per edge, nothing edge-sized but the int32 list is read or written.  tau_out
 * NULL: tau is not saved (no backward follows; the same bits in out).  Plain fp32: no input range, the range status is neither read nor
 * raised.  Timed under MSMP_K_NORM.  Accepted: width a multiple of 4 in 4 .. 256 (anything else MSMP_ERR_UNSUPPORTED before any launch); a
 * null or misaligned pointer, ld < width or not a multiple of 4, n_nodes outside 1 .. 2^31 - 1 or n_edges outside 0 .. 2^31 - 1: MSMP_ERR_ARG
 * with msmp_last_error naming the entry and the argument. */
int msmp_g2_gate_blend_f32(const float* h, const float* gate, const float* main, int ld, const int32_t* out_rowptr, const int32_t* out_nbr,
                           int64_t n_nodes, int64_t n_edges, int width, float* out, float* tau_out, msmp_stream_t stream);
/* Its backward from grad_out = dL/dout and the forward's inputs and tau_out:
 *     dh_i = (1 - tau_i) g_i,   db_i = tau_i g_i Swish'(main_i),   q_i = g_i (Swish(main_i) - h_i) (1 - tau_i^2) / D_i,
 *     da_i = Swish'(gate_i) (2 q_i sum_{j in out(i)} (t_i - t_j) - 2 sum_{s in in(i)} q_s (t_s - t_i))
 * as two launches inside the call: a node pass (dh, db, and q into the workspace: n_nodes * width floats) and a gather pass over both
 * lists in list order (da).  No atomics, no memset, no host read-back, fixed summation order: capturable, and two calls give the same bits.
 * Every element of columns 0 .. width - 1 of dh, da, db is written.  msmp_g2_gate_blend_bwd_workspace_bytes returns 0 (and
 * msmp_last_error) for a width or n_nodes outside the range; MSMP_ERR_WORKSPACE if workspace_bytes is below it; other refusals as the forward's. */
size_t msmp_g2_gate_blend_bwd_workspace_bytes(int64_t n_nodes, int width);
int msmp_g2_gate_blend_bwd_f32(const float* grad_out, const float* h, const float* gate, const float* main, const float* tau, int ld,
                               const int32_t* out_rowptr, const int32_t* out_nbr, const int32_t* in_rowptr, const int32_t* in_col,
                               int64_t n_nodes, int64_t n_edges, int width, float* dh, float* da, float* db, void* workspace,
                               size_t workspace_bytes, msmp_stream_t stream);
/* The Swish MLPs around the encoder and decoder for TRAINING (mlp_train_kernel.hip): forward with the pre-activations saved and the whole
 * backward, one kernel launch each, in the fp32-exact three-way bf16 split of the pair above (no input range; the range status is neither
 * read nor raised).  Parameters in nn.Linear's layout (experiments/models_gnn.py: embedding_mlp, lemoutput_mlp, double_mlp):
 *   layers 2, heads 1:       out = Swish(w2 Swish(w1 x + b1) + b2)      w1 [width, k_in], b1 [width], w2 [width, width], b2 [width]
 *   layers 1, heads 1 | 2:   out = Swish(w1 x + b1)                     w1 [heads width, k_in], b1 [heads width]; w2, b2 unused (NULL)
 * with 1 <= k_in <= 256 and 1 <= width <= 256: head h is columns h width .. of out, with its own width rows of w1 (double_mlp's
 * Unflatten(1, (2, width))).  Rows are row-major fp32 with explicit row strides; only the first k_in (heads width) floats of a row are
 * read or written.  kt = ceil(width / 32), kk = ceil(k_in / 32), Wp = 32 kt.
 *   msmp_packed_mlp_train_floats = 1536 (2 heads kt kk + (layers == 2 ? 2 kt^2 : 0)) + layers heads Wp: the forward fragments of w1 (, w2),
 *   the transposed fragments for the data gradients, and the biases, written by ONE msmp_pack_mlp_train_f32 launch;
 *   msmp_mlp_train_saved_floats = layers heads n_rows Wp: the pre-activations z1 (, z2; one layer: z of each head), every element written.
 * The size entries return 0 (and msmp_last_error) for a shape outside the range or n_rows outside 1 .. 2^31 - 1.  The launch entries
 * return MSMP_ERR_UNSUPPORTED for width or k_in outside 1..256, layers outside 1..2, heads outside 1..2 or two heads of two layers;
 * MSMP_ERR_ARG for a null required pointer, n_rows outside 1 .. 2^31 - 1, a row stride shorter than its row or a blob / saved that is
 * not 16-byte aligned.  A row's results depend on nothing but that row; two calls give the same bits. */
int64_t msmp_packed_mlp_train_floats(int layers, int heads, int k_in, int width);
int msmp_pack_mlp_train_f32(const float* w1, const float* b1, const float* w2, const float* b2, int layers, int heads, int k_in, int width,
                            float* packed_out, msmp_stream_t stream);
int64_t msmp_mlp_train_saved_floats(int64_t n_rows, int layers, int heads, int width);
/* x [n_rows, ldx] -> out [n_rows, ld_out] and saved. */
int msmp_mlp_train_fwd_f32(const float* x, int ldx, int64_t n_rows, int layers, int heads, int k_in, int width, const float* packed,
                           float* saved, float* out, int ld_out, msmp_stream_t stream);
/* grad_out [n_rows, ld_grad] (the gradient of out), the forward's x and saved -> dw1, db1 (, dw2, db2) in the layouts of the parameters,
 * every element written, and, where dx is not NULL, dx [n_rows, ld_dx] = the gradient of x (two heads: the sum over the heads, accumulated
 * in head order).  One kernel launch computes dz2 = grad_out dswish(z2), da1 = w2^T dz2, dz1 = da1 dswish(z1) and dx = w1^T dz1 and leaves
 * dz2, dz1 and a1 = Swish(z1) in the workspace as row matrices of row stride 128 ceil(width / 128) (dz1 of two heads: 128 ceil(2 width /
 * 128)) with zeros in the padding columns; the weight gradients are then msmp_grad_weights_f32 jobs of 128 columns of dz each, issued
 * inside this call (fixed summation order), and one small copy for a part-filled last 128-row group.  No atomics, no memset, no
 * synchronisation, capturable.  workspace: msmp_mlp_train_bwd_workspace_bytes bytes (0 for a shape outside the range); MSMP_ERR_WORKSPACE
 * if workspace_bytes is below it. */
size_t msmp_mlp_train_bwd_workspace_bytes(int64_t n_rows, int layers, int heads, int k_in, int width);
int msmp_mlp_train_bwd_f32(const float* grad_out, int ld_grad, const float* x, int ldx, const float* saved, int64_t n_rows, int layers,
                           int heads, int k_in, int width, const float* packed, float* dx, int ld_dx, float* dw1, float* db1, float* dw2,
                           float* db2, void* workspace, size_t workspace_bytes, msmp_stream_t stream);
/* The message half of one head at any hidden width 1 <= width <= 256 in ONE launch, nothing edge-sized in memory
 * (experiments/models_gnn.py:132-138 message with message_net_1 factorised per node into p / q, :107 aggr = 'mean'):
 *   agg_out[n][c] = (1 / max(deg n, 1)) sum_{r in CSR row n} Swish(b2[c] + sum_k w2[c][k] Swish(p[n][k] + q[col[r]][k])),   c < width,
 * summed in CSR order in fp32 (the result does not depend on the batch around a node); zero in-degree gives an exact 0; columns
 * width .. ld - 1 of agg_out are written as 0 (as msmp_wide_scatter_mean_f32 writes them); p, q, agg_out [n_nodes, ld] with ld a
 * multiple of 4 in width .. 4096, 16-byte aligned; columns width .. ld - 1 of p and q are not used.  fp16-split MFMA arithmetic of the
 * default path with W2 in registers; an activation Swish(p + q) with |x| > 255 or not finite raises MSMP_STATUS_NODE_SATURATED.
 * Blob size / pack (experiments/models_gnn.py:132-138: message_net_2[0].weight [width, width] and .bias; :107): 0 and msmp_last_error
 * for a width outside 1..256. */
int64_t msmp_packed_wide_msg_floats(int width);
int msmp_pack_wide_msg_f32(const float* w2, const float* b2, int width, float* packed_out, msmp_stream_t stream);
/* experiments/models_gnn.py:132-138, :107: the largest in-degree msmp_wide_message_f32 takes at this width (at least 32, the neighbour
 * cap of the reference's radius graphs); 0 and msmp_last_error for a width outside 1..256. */
int msmp_wide_message_max_in_degree(int width);
/* experiments/models_gnn.py:132-138, :107.  max_in_degree: an upper bound of the in-degrees of rowptr (GraphStructure.max_in_degree);
 * above msmp_wide_message_max_in_degree(width): MSMP_ERR_UNSUPPORTED (the caller takes the three launches above).  MSMP_ERR_ARG for a
 * width outside 1..256, a bad ld, a null or misaligned pointer; n_nodes == 0 is a no-op, n_edges == 0 writes zeros. */
int msmp_wide_message_f32(const float* p, const float* q, const int32_t* rowptr, const int32_t* col, int64_t n_nodes, int64_t n_edges,
                          int max_in_degree, int width, int ld, const float* packed, float* agg_out, msmp_stream_t stream);
/* The node half of one layer at any hidden width 1 <= width <= 256 in ONE launch, both heads of a gated pair, on graphs of up to 128 nodes;
 * neither the concatenated update input nor z nor y goes to memory:
 *   z_k = Swish(w3_k [h | agg_k | vars] + b3_k)       update_net_1 (experiments/models_gnn.py:140-149)
 *   y_k = w4_k z_k + b4_k                             update_net_2 (GNN_LayerLin: no activation, no residual)
 *   n_k = InstanceNorm of y_k per graph and channel, biased variance, eps (:129)
 *   out = n_main   without a gate head;   out = (1 - tau) h + tau Swish(n_main),  tau = sigmoid(n_gate)   with one (:1486-1489).
 * update_net_2 is evaluated CENTRED: n_k does not change when a per-graph, per-channel constant is taken from y_k, so the kernel forms
 * w4_k 2^6 (z_n - z_ref), z_ref the row of the graph's first node, from zero accumulators.  The fp32 accumulator then rounds relative to the
 * variation of y over the graph, which the norm divides by, not to |y|, and the lo half of the operand's fp16 split stays out of the
 * fp16 denormals (|z_n - z_ref| must stay below 1024; beyond that the statistics are not finite and raise MSMP_STATUS_NONFINITE).  b4 keeps its place in the blob and is NOT read: the result does
 * not depend on it (bitwise, as long as it does not move the power of two chosen for (w4, b4)).
 * One workgroup per graph and fixed-order sums: a graph's rows do not depend on the batch around it or on its position, and two runs
 * give the same bits.  fp16-split MFMA arithmetic of the default path with node rows scaled by 2^8: an h or agg element with |x| > 255
 * or not finite raises MSMP_STATUS_NODE_SATURATED, statistics that are not finite raise MSMP_STATUS_NONFINITE.
 * Blob size / pack (experiments/models_gnn.py:140-149: update_net_1[0].weight [width, 2 width + nv] and .bias, update_net_2[0].weight
 * [width, width] and .bias, as in the state_dict): scales [8] | b3 [Wp] | b4 [Wp] | the fp16 hi / lo fragments of w3 2^s3 and w4 2^s4,
 * zero-filled up to Wp = 32 KT, KT = ceil(width / 32): 8 + 576 KT + 3072 KT^2 floats whatever nv is (the variables take one K = 16 step);
 * the powers of two are chosen on the device.  0 and msmp_last_error for a width outside 1..256 or nv outside 0..8. */
int64_t msmp_packed_wide_tail_floats(int width, int nv);
int msmp_pack_wide_tail_f32(const float* w3, const float* b3, const float* w4, const float* b4, int width, int nv, float* packed_out,
                            msmp_stream_t stream);
/* experiments/models_gnn.py:129: the largest graph (nodes) msmp_wide_node_tail_f32 takes at this width: 128, the InstanceNorm statistics
 * of a graph stay in one workgroup's registers; 0 and msmp_last_error for a width outside 1..256. */
int msmp_wide_node_tail_max_graph_nodes(int width);
/* experiments/models_gnn.py:140-149, :129, :1486-1489.  h, agg_main, agg_gate, out [n_nodes, ld] with ld a multiple of 4 in width .. 4096,
 * 16-byte aligned (columns width .. ld - 1 of the inputs are not used, of out they are written as 0; nothing outside out is written);
 * vars [n_nodes, nv], nv 0..8; graph_ptr [n_graphs + 1] node offsets; max_graph_nodes: an upper bound of the graph sizes
 * (GraphStructure.max_graph_nodes).  agg_gate == packed_gate == NULL selects the form without a gate head; one without the other is
 * MSMP_ERR_ARG.  MSMP_ERR_UNSUPPORTED for max_graph_nodes above msmp_wide_node_tail_max_graph_nodes(width) or a width outside 1..256 (the
 * caller keeps the row GEMMs and msmp_wide_norm_blend_f32, as with msmp_node_tail_f32 above 128 nodes); MSMP_ERR_ARG for a null or
 * misaligned pointer, a bad ld, nv outside 0..8 or negative sizes; n_nodes == 0 is a no-op.  Allocates nothing and never synchronises. */
int msmp_wide_node_tail_f32(const float* h, const float* agg_main, const float* agg_gate, const float* vars, const int32_t* graph_ptr,
                            int64_t n_nodes, int64_t n_graphs, int max_graph_nodes, int nv, int width, int ld, const float* packed_main,
                            const float* packed_gate, float eps, float* out, msmp_stream_t stream);
/* The per-node projections of the factorised message_net_1 at any hidden width 1 <= width <= 256 in ONE launch, both heads of a gated pair;
 * the concatenated rows [h | u | pos | vars] do not go to memory (experiments/models_gnn.py:132-138):
 *   P[n] = w1[:, 0:W] h_n + w1[:, 2W:] [u_n | pos_n | vars_n] + b1          Q[n] = w1[:, W:2W] h_n - w1[:, 2W:2W+tw+1] [u_n | pos_n]
 * so that message_net_1 of the edge j -> i is Swish(P[i] + Q[j]) (msmp_wide_message_f32 takes P and Q).  A node's rows depend on nothing
 * but that node's inputs and the weights: not on the nodes around it, on n_nodes, or on the run (bitwise).  fp16-split MFMA arithmetic of
 * the default path with node rows scaled by 2^8: an h or feature element with |x| > 255 or not finite raises MSMP_STATUS_NODE_SATURATED.
 * Blob size / pack (experiments/models_gnn.py:132-138: message_net_1[0].weight [width, 2 width + tw + 1 + nv] and .bias, as in the
 * state_dict): scales [8] | b1 [Wp] | the fp16 hi / lo fragments of the P and Q matrices times 2^s (Q's tail: the negated u | pos columns,
 * zeros for the variables), zero-filled up to Wp = 32 KT, KT = ceil(width / 32), and up to TS = ceil((tw + 1 + nv) / 16) K = 16 steps of
 * the tail: 8 + 32 KT + 1024 KT (2 KT + TS) floats; the power of two is chosen on the device.  0 and msmp_last_error for a width outside
 * 1..256, tw < 1, nv outside 1..8 or tw + 1 + nv > 128. */
int64_t msmp_packed_wide_proj_floats(int width, int tw, int nv);
/* experiments/models_gnn.py:132-138 (message_net_1[0] of GNN_LayerLin).  MSMP_ERR_ARG outside the ranges above or for a null pointer. */
int msmp_pack_wide_proj_f32(const float* w1, const float* b1, int width, int tw, int nv, float* packed_out, msmp_stream_t stream);
/* experiments/models_gnn.py:132-138.  h, p_*, q_* [n_nodes, ld] with ld a multiple of 4 in width .. 4096, 16-byte aligned (columns
 * width .. ld - 1 of h are not used, of the outputs they are written as 0; nothing outside the outputs is written); feat: the rows of
 * msmp_pack_node_features_f32 at stride msmp_node_feature_stride(tw, nv), 16-byte aligned.  packed_gate == p_gate == q_gate == NULL selects
 * the form with one head; a partial set of the three is MSMP_ERR_ARG.  MSMP_ERR_UNSUPPORTED for a width outside 1..256 or
 * tw + 1 + nv > 128 (the caller keeps the row GEMMs); MSMP_ERR_ARG for a null or misaligned pointer, a bad ld, tw < 1, nv outside 1..8 or
 * negative sizes; n_nodes == 0 is a no-op.  Allocates nothing and never synchronises. */
int msmp_wide_node_proj_f32(const float* h, const float* feat, int64_t n_nodes, int tw, int nv, int width, int ld, const float* packed_main,
                            const float* packed_gate, float* p_main, float* q_main, float* p_gate, float* q_gate, msmp_stream_t stream);
/* The backward of one GNN_LayerLin, or of a gated pair of them, at any hidden width 1..256 in one call: the width-generic counterpart of
 * msmp_mp_layer_bwd_f32, same meaning (experiments/models_gnn.py:88-149, 1486-1489; params_gate == grads_gate == NULL: a single layer).
 * grad_out, h, dh_out [N, ld] with ld = 128 ceil(width / 128), 16-byte aligned; the padding columns width .. ld - 1 are zero on input and
 * written as zero.  params_* / grads_*: arrays of 8 device pointers in the reference's [out, in] layouts with out = width (message_net_1.0.weight
 * [width, 2 width + tw + 1 + nv], ..., update_net_2.0.bias [width]); u, pos, vars carry no gradient.  ONE algorithm: message_net_1 factorised
 * through per-node projections (nothing edge-sized of width 2 width + tw + 1 + nv), fp32-exact bf16x3 row GEMMs, sums in fixed orders, batched
 * fp32-exact weight gradients; no atomics, no memset, no library GEMM: two calls on the same inputs give the same bits.  src_rowptr [N+1] /
 * src_perm [E] (the CSR edge ids regrouped by source, ascending inside a source) are REQUIRED when n_edges > 0 (MSMP_ERR_ARG without).
 * MSMP_ERR_UNSUPPORTED (nothing launched; the workspace query returns 0) for a width outside 1..256, tw + 1 + nv > 128 or nv > MSMP_MAX_VARS;
 * MSMP_ERR_ARG for a null or misaligned pointer, ld other than 128 ceil(width / 128) or bad sizes.  Allocates nothing, never synchronises. */
size_t msmp_wide_layer_bwd_workspace_bytes(int64_t n_nodes, int64_t n_edges, int tw, int nv, int width, int gated);
int msmp_wide_layer_bwd_f32(const float* grad_out, const float* h, const float* u, const float* pos, const float* vars,
                            const int32_t* rowptr, const int32_t* col, const int32_t* tgt, const int32_t* src_rowptr,
                            const int32_t* src_perm, const int32_t* graph_ptr, int64_t n_nodes, int64_t n_edges, int64_t n_graphs,
                            int tw, int nv, int width, int ld, const float* const* params_main, const float* const* params_gate,
                            float eps, float* dh_out, float* const* grads_main, float* const* grads_gate, void* workspace,
                            size_t workspace_bytes, msmp_stream_t stream);
/* gate_pre == NULL: out = InstanceNorm(main_pre); else out = (1 - tau) h + tau Swish(IN(main_pre)), tau = sigmoid(IN(gate_pre)) */
int msmp_wide_norm_blend_f32(const float* h, const float* gate_pre, const float* main_pre, const int32_t* graph_ptr, int64_t n_graphs,
                             int width, int ld, float eps, float* out, msmp_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * In-library kernel timing (measurement aid for bench.py; off by default, not part of the data path)
 * When enabled, every launch of the named kernel family is bracketed by hipEvents recorded on the
 * launch stream.  msmp_timing_read synchronises on the recorded events and returns the number of
 * launches and their summed device time since the last reset.
 * ------------------------------------------------------------------------------------------- */
#define MSMP_K_EDGE_MLP     0
#define MSMP_K_SCATTER_MEAN 1
#define MSMP_K_NODE_UPDATE  2
#define MSMP_K_NORM         3   /* instance_norm and gate_blend */
#define MSMP_K_LEM          4
#define MSMP_K_NODE_PROJ    5
#define MSMP_K_DECODER      6
#define MSMP_K_COUNT        7
int msmp_timing_enable(int kernel_mask);   /* bit k enables family k; 0 disables all */
int msmp_timing_reset(void);
int msmp_timing_read(int kernel, int64_t* launches_out, double* total_ms_out);

#ifdef __cplusplus
}
#endif
#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#endif /* MSMP_PDE_H */
