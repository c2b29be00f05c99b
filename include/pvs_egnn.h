/*
 * pvs_egnn.h - C ABI of libpvs_egnn.so: the MI355X (gfx950) implementation of the PointVS EGNN
 * message-passing hot path (forward and backward).
 *
 * The reference has no native code at all: the boundary it offers for this path is
 * the Python nn.Module surface.  Each entry point below therefore names the reference Python
 * function whose body it replaces.  The host side that keeps the reference's class surface
 * (`pointvs_amd/egnn_satorras.py` etc.) binds these with ctypes; see INTEGRATION.md for the stub a
 * reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to caller-owned memory (torch allocations); the library
 *     never allocates, frees or synchronises; all work is enqueued on `stream` (hipGraph-capturable)
 *   - floating point is fp32, except the *_f64 entries (the reference's --double: fp64 throughout, same
 *     layouts); indices int32 inside the library (the int64 COO / int64 one-hot the
 *     reference hands over is converted once per batch by pvs_graph_prepare)
 *   - row-major, dense; "[E,H] sorted" means edge rows in the CSR order produced by
 *     pvs_graph_prepare (use pvs_rows_to_input_order to get the reference's input edge order)
 *   - return value: 0 = ok, <0 = error; pvs_last_error() gives the message (thread-local)
 *   - stateless and re-entrant
 */
#ifndef PVS_EGNN_H
#define PVS_EGNN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* pvs_stream_t; /* hipStream_t */

/* ---- layer flags: one bit per EGNNLayer.__init__ switch (egnn_satorras.py:26-46) ---- */
enum {
    PVS_RESIDUAL        = 1u << 0,
    PVS_EDGE_RESIDUAL   = 1u << 1,  /* applied only when m_prev != NULL (egnn_satorras.py:194) */
    PVS_EDGE_ATTENTION  = 1u << 2,
    PVS_NORMALIZE       = 1u << 3,
    PVS_TANH            = 1u << 4,
    PVS_GRAPHNORM       = 1u << 5,
    PVS_UPDATE_COORDS   = 1u << 6,
    PVS_PERM_INVARIANT  = 1u << 7,
    PVS_NODE_ATTENTION  = 1u << 8,
    PVS_GATED_RESIDUAL  = 1u << 9,
    PVS_REZERO          = 1u << 10,
    PVS_SOFTMAX_ATT     = 1u << 11,
    /* GraphNorm per node segment, forward only, fp32: valid only together with PVS_GRAPHNORM. The graph's
     * n_norm_rows_dev then points at a DEVICE int32 table [n_graphs + 1] (the first row of every segment, as the batch
     * builders leave node_ptr / graph_ptr; n_graphs >= 1, <= n_nodes; graph_eptr may stay NULL) instead of a single
     * count. Every entry is clamped to [0, n_nodes]; segment s = rows [table[s], table[s + 1]), length
     * max(0, table[s + 1] - table[s]); the table is expected non-decreasing and is read when the kernels run (a captured
     * forward follows what is written into it). Each segment's mean and variance are bit for bit those of a call on its
     * rows alone (pvs_graphnorm_stats_segments below), each row is normalised with its own segment's pair, and rows in
     * front of table[0] or at / behind table[n_graphs] (padding) with mean = var = 0 - finite whenever the input is. A
     * segment of length 0 has mean = var = 0; nothing is divided by 0. No atomics: the same bits every call.
     * Honoured by pvs_egnn_layer_fwd, pvs_egnn_stack_fwd and pvs_egnn_layer_fwd_partial / _fwd_partial_att /
     * _fwd_partial_softmax; pvs_egnn_layer_workspace_bytes grows under it (statistics and slabs for up to n_nodes
     * segments) and the [2H] statistics slot of `saved` is unspecified. Refused, by name, by pvs_egnn_layer_bwd,
     * pvs_egnn_stack_bwd and every *_f64 entry, without PVS_GRAPHNORM, with a NULL table and with n_graphs < 1. Without
     * the flag nothing changes. */
    PVS_GRAPHNORM_SEGMENTS = 1u << 12
};

/* attention_activation_fn (egnn_satorras.py:66-71); IDENTITY is what softmax_attention selects */
enum { PVS_ACT_SIGMOID = 0, PVS_ACT_TANH = 1, PVS_ACT_RELU = 2, PVS_ACT_SILU = 3, PVS_ACT_IDENTITY = 4 };

typedef struct PvsLayerDesc {
    int32_t  hidden;       /* H = input_nf = hidden_nf = output_nf (always k,k,k in build_net). Built widths: 16, 32, 64
                            * (every kernel family) and 128 (MFMA kernels, <= 3 edge classes: the reference's --channels
                            * 65..128, parse_args.py:56, zero-padded by the caller); other sizes are padded up by the caller */
    int32_t  n_edge_attr;  /* A = edges_in_d: number of one-hot edge classes (0 = no edge_attr) */
    uint32_t flags;        /* PVS_* bits */
    int32_t  att_act;      /* PVS_ACT_* */
} PvsLayerDesc;

/* Graph in the library's layout, filled by pvs_graph_prepare. Rows = edge_index[0] (aggregation
 * target, egnn_satorras.py:135,171), cols = edge_index[1]. */
typedef struct PvsGraph {
    int32_t n_nodes;
    int32_t n_edges;
    const int32_t* rowptr;   /* [N+1] CSR offsets by row                                        */
    const int32_t* row;      /* [E]   row of each sorted edge                                   */
    const int32_t* col;      /* [E]   col of each sorted edge (stable order within a row)       */
    const uint8_t* etype;    /* [E]   one-hot class of each sorted edge (NULL when A == 0)      */
    const int32_t* perm;     /* [E]   sorted position -> input edge id                          */
    const int32_t* colptr;   /* [N+1] CSC offsets by col                                        */
    const int32_t* cedge;    /* [E]   sorted positions of the edges grouped by col (stable)     */
    const float*   inv_deg;  /* [N]   1 / max(deg_row, 1)  (unsorted_segment_mean's clamp)      */
    /* Optional DEVICE int32: the true edge count when it is only known on the device (a graph made
     * by pvs_graph_filter_ligand_edges); n_edges is then the capacity of the edge arrays. Forward only:
     * pvs_egnn_layer_fwd (and pvs_egnn_stack_fwd through it) on the MFMA edge kernel with m_out == NULL, and
     * pvs_egnn_layer_edge_sums / _edge_stats_softmax / _fwd_partial / _fwd_partial_att / _fwd_partial_softmax
     * accept such a graph. */
    const int32_t* n_edges_dev;
    /* Optional DEVICE int32 [n_graphs + 1]: first sorted edge of every graph of the batch (graphs are
     * contiguous node ranges, so contiguous edge ranges of the CSR), last entry = E; NULL / 0 when unknown.
     * Speed and values of the reference are unaffected by it; the fp16-split edge backward uses it to end its
     * 32-edge tiles at graph boundaries, because one tile shares one power-of-two scale and two graphs'
     * gradients can differ by many orders of magnitude ("f16x2").
     * ACCURACY CONTRACT for callers that leave it NULL: a tile of the H = 32 backward may then span two graphs, and the
     * smaller graph's per-edge gradients in that tile keep 22 - max(0, k - 14) bits when they are 2^-k below the
     * larger graph's (absolute error 2^-36 of the tile's largest value). pointvs_amd fills it wherever it knows the
     * batch's graphs: model forward, get_embeddings (from the batch vector), every graph prepared by
     * pvs_graph_prepare_runs (edge_ptr IS this table). */
    const int32_t* graph_eptr;
    int32_t n_graphs;
    /* Optional DEVICE int32: the number of LEADING rows that enter GraphNorm's statistics when it is only known on the
     * device (a padded, captured step: the real nodes in front, padding rows behind them). NULL: n_nodes. Read by the
     * fp32 layer entry points under PVS_GRAPHNORM (pvs_egnn_layer_fwd / _fwd_partial / _fwd_partial_att /
     * _fwd_partial_softmax / _bwd and pvs_egnn_stack_fwd / _bwd), ignored without that flag, refused by the *_f64 entry points. With n = the value
     * clamped to [0, n_nodes]: mean and variance are those of rows [0, n) - bit for bit the statistics of a call on
     * those n rows alone -, rows >= n are never read for them, ALL n_nodes rows are normalised with them, and the
     * backward is the exact gradient of that (with zero upstream gradient on the rows >= n: the gradient of the n-row
     * problem). n = 0: mean = var = 0, rstd = 1 / sqrt(eps); nothing is divided by n.
     * Under the layer flag PVS_GRAPHNORM_SEGMENTS (forward only) this member is instead a DEVICE int32 table
     * [n_graphs + 1] of segment starts and every segment of rows is normalised by its own statistics: see the flag.
     * ABI (pvs_version() >= 112): sizeof(PvsGraph) = 104, offsetof(PvsGraph, n_norm_rows_dev) = 96. */
    const int32_t* n_norm_rows_dev;
} PvsGraph;
#if defined(__cplusplus)
static_assert(sizeof(PvsGraph) == 104 && offsetof(PvsGraph, n_norm_rows_dev) == 96, "PvsGraph layout (pointvs_amd/_lib.py)");
#endif

/* Parameters of one EGNNLayer, torch nn.Linear layout W[out][in] (state_dict keys in comments). */
typedef struct PvsLayerParams {
    const float* edge_w1;   /* edge_mlp.0.weight  [H, (perm_inv?H:2H)+1+A] */
    const float* edge_b1;   /* edge_mlp.0.bias    [H]      */
    const float* edge_w2;   /* edge_mlp.2.weight  [H,H]    */
    const float* edge_b2;   /* edge_mlp.2.bias    [H]      */
    const float* coord_w1;  /* coord_mlp.0.weight [H,H]    */
    const float* coord_b1;  /* coord_mlp.0.bias   [H]      */
    const float* coord_w2;  /* coord_mlp.2.weight [1,H]    */
    const float* att_w;     /* att_mlp.0.weight   [1,H]    (edge attention) */
    const float* att_b;     /* att_mlp.0.bias     [1]      */
    const float* node_w1;   /* node_mlp.0.weight  [H,2H]   */
    const float* node_b1;   /* node_mlp.0.bias    [H]      */
    const float* node_w2;   /* node_mlp.3.weight  [H,H]    */
    const float* node_b2;   /* node_mlp.3.bias    [H]      */
    const float* gn_weight; /* node_mlp.1.weight  [H]      (graphnorm) */
    const float* gn_bias;   /* node_mlp.1.bias    [H]      */
    const float* gn_mean_scale; /* node_mlp.1.mean_scale [H] */
    const float* node_att_w;    /* node_att_mlp.0.weight [1,H] */
    const float* node_att_b;    /* node_att_mlp.0.bias   [1]   */
    const float* edge_gate;     /* edge_gate_parameter [1] */
    const float* node_gate;     /* node_gate_parameter [1] */
} PvsLayerParams;

/* Gradients, same shapes; every non-NULL member is OVERWRITTEN with this call's gradient. */
typedef struct PvsLayerGrads {
    float *edge_w1, *edge_b1, *edge_w2, *edge_b2;
    float *coord_w1, *coord_b1, *coord_w2;
    float *att_w, *att_b;
    float *node_w1, *node_b1, *node_w2, *node_b2;
    float *gn_weight, *gn_bias, *gn_mean_scale;
    float *node_att_w, *node_att_b;
    float *edge_gate, *node_gate;
} PvsLayerGrads;

const char* pvs_last_error(void);
int pvs_version(void);

/* ---------------------------------------------------------------------------------------------
 * Graph preparation: int64 COO (arbitrary order, duplicates allowed - SURVEY Q6) + int64 one-hot
 * edge_attr, as PygPointCloudDataset emits them (data_loaders.py:359-370), to CSR/CSC.
 * Replaces nothing in the reference (torch indexes the COO directly, egnn_satorras.py:190-193);
 * it is the once-per-batch price of atomics-free, deterministic segment reductions.
 *   edge_index [2,E] int64, edge_attr [E,A] int64 one-hot or NULL.
 *   status: device int32[1], 0 on success, bit0 = index out of range, bit1 = edge_attr row not
 *   one-hot; checked by the caller whenever it next synchronises.
 * Output arrays are the members of PvsGraph (caller-allocated with the sizes given there).
 * colptr / cedge may both be NULL for forward-only use (skips the second sort).
 */
size_t pvs_graph_prepare_workspace_bytes(int32_t n_nodes, int32_t n_edges);
int pvs_graph_prepare(const int64_t* edge_index, const int64_t* edge_attr, int32_t n_edge_attr,
                      int32_t n_nodes, int32_t n_edges,
                      int32_t* rowptr, int32_t* row, int32_t* col, uint8_t* etype, int32_t* perm,
                      int32_t* colptr, int32_t* cedge, float* inv_deg, int32_t* status,
                      void* workspace, size_t workspace_bytes, pvs_stream_t stream);

/* The same result as pvs_graph_prepare for an edge list with the layout of the reference's data loader,
 * without the by-row radix sort: per graph, generate_edges (preprocessing.py:108-142) emits the
 * inter-molecular block and then the intra-molecular block, each in row-major (np.where) order = two
 * row-sorted runs, and PyG collation (data_loaders.py:517-520) concatenates the graphs. node_ptr / edge_ptr
 * [n_graphs + 1] (DEVICE int32) give each graph's node and edge ranges. The layout is the caller's
 * contract; it is verified on the device and a violation sets bit 4 of *status (bits 1, 2 as in
 * pvs_graph_prepare). Outputs are array-for-array those of pvs_graph_prepare.
 * max_graph_nodes: an upper bound on the nodes of one graph, known to the caller (0 = unknown). With a bound of
 * at most 4096 the by-column lists are built by a counting transpose per graph (LDS tables over the graph's own
 * columns) instead of a radix sort of all edges by column; same arrays. A graph larger than the bound sets bit 4. */
size_t pvs_graph_prepare_runs_workspace_bytes(int32_t n_nodes, int32_t n_edges, int32_t n_graphs,
                                              int32_t max_graph_nodes);
int pvs_graph_prepare_runs(const int64_t* edge_index, const int64_t* edge_attr, int32_t n_edge_attr,
                           int32_t n_nodes, int32_t n_edges, int32_t n_graphs, const int32_t* node_ptr,
                           const int32_t* edge_ptr, int32_t* rowptr, int32_t* row, int32_t* col, uint8_t* etype,
                           int32_t* perm, int32_t* colptr, int32_t* cedge, float* inv_deg, int32_t* status,
                           int32_t max_graph_nodes, void* workspace, size_t workspace_bytes, pvs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Radius graph straight from coordinates: generate_edges of the reference
 * (preprocessing.py:68-155, the prune=False body) fused with the COO -> CSR/CSC step, so the
 * int64 edge list and the int64 one-hot never exist. Same result, array for array, as
 * pvs_graph_prepare on the reference's own output for the same atoms:
 *   inter block: pairs with 1e-7 < d < inter_radius and bp_i != bp_j (class 1), row-major;
 *   intra block: all pairs with 1e-7 < d < intra_radius (class 2 if both bp == 1, else 0), row-major;
 *   perm = position of each CSR-sorted edge in [inter block | intra block] (the reference's order).
 * d is the float64 cdist distance (same operation order, no FMA): identical `<` decisions.
 *   pos [N,3] fp32, bp [N] uint8 (0 ligand / 1 receptor), graph_ptr [B+1] int32 node offsets of the
 *   batch's graphs (pairs are only formed inside a graph).
 * Two steps because E is data dependent: _count runs the O(n_g^2) distance tests once, leaves a
 * 64-bit neighbour mask per (row, 64-column chunk) in `state` and fills rowptr/inter_ptr/intra_ptr
 * ([N+1] each); the caller reads rowptr[N] = E back, allocates, and _fill expands the masks.
 * max_graph_nodes = node count of the largest graph of the batch (sizes the masks).
 * colptr / cedge may both be NULL (forward-only use: only the backward reads the by-column lists;
 * skips the radix sort); pvs_egnn_layer_bwd then refuses the graph.
 */
size_t pvs_radius_graph_state_bytes(int32_t n_nodes, int32_t n_graphs, int32_t max_graph_nodes);
size_t pvs_radius_graph_workspace_bytes(int32_t n_nodes, int32_t n_graphs, int32_t n_edges);
int pvs_radius_graph_count(const float* pos, const uint8_t* bp, const int32_t* graph_ptr, int32_t n_graphs,
                           int32_t n_nodes, int32_t max_graph_nodes, double inter_radius, double intra_radius,
                           int32_t pair_filter /* 0: every pair; 1: only pairs that touch a ligand atom (bp == 0) */,
                           int32_t* rowptr, int32_t* inter_ptr, int32_t* intra_ptr,
                           void* state, size_t state_bytes, pvs_stream_t stream);
int pvs_radius_graph_fill(const uint8_t* bp, const int32_t* graph_ptr, int32_t n_graphs, int32_t n_nodes,
                          int32_t max_graph_nodes, int32_t n_edges,
                          const int32_t* rowptr, const int32_t* inter_ptr, const int32_t* intra_ptr,
                          int32_t* row, int32_t* col, uint8_t* etype, int32_t* perm,
                          int32_t* colptr, int32_t* cedge, float* inv_deg,
                          const void* state, size_t state_bytes,
                          void* workspace, size_t workspace_bytes, pvs_stream_t stream);

/* One sweep of min-label propagation over a CSR (labels start as node ids; repeat until *changed
 * stays 0): connected components for the `prune` option of generate_edges
 * (preprocessing.py:139-151), driven from the host side (pointvs_amd/radius_graph.py). */
int pvs_graph_min_label_step(const int32_t* rowptr, const int32_t* col, int32_t n_nodes, int32_t* labels,
                             int32_t* changed, pvs_stream_t stream);

/* Edge dropout of SartorrasEGNN.get_embeddings (egnn_satorras.py:320-323: torch_geometric's
 * dropout_adj(edges, edge_attr, p, force_undirected=True, training)): of every pair only the copy with
 * row <= col is drawn (kept with probability 1 - p), the survivors' reverses are appended, attributes repeated.
 * Philox4x32-10 keyed on (seed, step), counter = edge id: reproducible, not bit-matched to torch's generator.
 * _mark: pos [E + 1] = exclusive scan of the keep flags (pos[E] = number of survivors K, read it on the host);
 * _fill: out_index int64 [2][2K], out_attr int64 [2K][A]. */
size_t pvs_dropout_adj_workspace_bytes(int32_t n_edges);
int pvs_dropout_adj_mark(const int64_t* edge_index, int32_t n_edges, float p, uint64_t seed, uint64_t step,
                         int32_t* pos, void* workspace, size_t workspace_bytes, pvs_stream_t stream);
int pvs_dropout_adj_fill(const int64_t* edge_index, const int64_t* edge_attr, int32_t n_edge_attr,
                         int32_t n_edges, const int32_t* pos, int32_t n_kept, int64_t* out_index,
                         int64_t* out_attr, pvs_stream_t stream);
/* The same draw for a captured training step: no host read, no by-value key.
 * key_table: device uint64 [2] = {seed, step}; _key_write sets it from the host (one tiny launch, by value - issue
 * it OUTSIDE a capture, before each replay). _mark_dev is _mark reading its key there (same flags, scan and stream).
 * _fill_padded: out_index int64 [2][cap] (row stride cap), out_attr int64 [cap][A], cap even and
 * >= 2 * #{e : row[e] <= col[e]} (an upper bound of 2K known on the host). With K = pos[E], read on the device:
 * survivors in [0, K) in input order, their reverses in [K, 2K) - dropout_adj's list - and every slot j in [2K, cap)
 * a padding edge: d = j - 2K, k = (d / 2) mod (n_pad / 2), a = n_nodes + 2k, b = a + 1; (a, b) for even d, (b, a)
 * for odd d, attribute row one-hot class 0. n_pad even, >= 2: the padding nodes n_nodes .. n_nodes + n_pad - 1 are
 * the caller's to provide. Nothing is written when 2K > cap (the bound was wrong; pos[E] tells). */
int pvs_dropout_key_write(uint64_t* key_table, uint64_t seed, uint64_t step, pvs_stream_t stream);
int pvs_dropout_adj_mark_dev(const int64_t* edge_index, int32_t n_edges, float p, const uint64_t* key_table,
                             int32_t* pos, void* workspace, size_t workspace_bytes, pvs_stream_t stream);
int pvs_dropout_adj_fill_padded(const int64_t* edge_index, const int64_t* edge_attr, int32_t n_edge_attr,
                                int32_t n_edges, const int32_t* pos, int32_t cap, int32_t n_nodes, int32_t n_pad,
                                int64_t* out_index, int64_t* out_attr, pvs_stream_t stream);

/* dst[perm[e], :] = src[e, :]  (sorted -> input edge order), width floats per row.
 * Gives EGNNLayer.forward's 4th return value `edge_feat` and `att_val` in the reference's order. */
int pvs_rows_to_input_order(const float* src, float* dst, const int32_t* perm, int32_t n_edges,
                            int32_t width, pvs_stream_t stream);
/* dst[e, :] = src[perm[e], :]  (input -> sorted edge order): incoming edge_messages and their grads. */
int pvs_rows_to_sorted_order(const float* src, float* dst, const int32_t* perm, int32_t n_edges,
                             int32_t width, pvs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * EGNNLayer.forward (egnn_satorras.py:189-206): coord2radial :178-187, edge_model :123-132,
 * edge-residual :194-202, coord_model :168-176 (+unsorted_segment_mean :340-347),
 * node_model :134-166 (+unsorted_segment_sum :332-337).
 *   h [N,H], x [N,3] inputs; m_prev [E,H] sorted or NULL (edge_messages of the previous layer)
 *   h_out [N,H], x_out [N,3] (never aliases x: the reference's in-place `coord += agg` is the
 *   caller's business), m_out [E,H] sorted or NULL (skip materialising edge_feat),
 *   att_out [E] sorted (required when PVS_EDGE_ATTENTION: also consumed by the backward),
 *   node_att_out [N] or NULL, saved: pvs_egnn_layer_saved_floats() floats kept for the backward.
 * pvs_egnn_layer_workspace_bytes(desc, N, E, backward): 0 for pvs_egnn_layer_fwd, 1 for pvs_egnn_layer_bwd, 2 and 3 for
 * the first-layer reuse below: 2 is the forward's workspace plus a per-edge attention array (pvs_egnn_layer_edge_sums /
 * _fwd_partial / _fwd_partial_att), 3 is mode 2 plus the per-row factor array [N] (_edge_stats_softmax /
 * _fwd_partial_softmax).
 */
size_t pvs_egnn_layer_saved_floats(const PvsLayerDesc* desc, int32_t n_nodes, int32_t n_edges);
size_t pvs_egnn_layer_workspace_bytes(const PvsLayerDesc* desc, int32_t n_nodes, int32_t n_edges,
                                      int32_t backward);
int pvs_egnn_layer_fwd(const PvsLayerDesc* desc, const PvsGraph* graph, const PvsLayerParams* params,
                       const float* h, const float* x, const float* m_prev,
                       float* h_out, float* x_out, float* m_out, float* att_out,
                       float* node_att_out, float* saved,
                       void* workspace, size_t workspace_bytes, pvs_stream_t stream);

/* Forward-only pieces for virtual screening (`val`/inference.py loop of the
 * reference, point_neural_network_base.py:208-360): when many ligand poses are scored against one
 * receptor, the receptor-receptor messages of the FIRST layer (inputs: receptor features and
 * coordinates only) are the same for every pose.
 *   pvs_egnn_layer_edge_sums: the row-side sums of one layer's edge work over the edges of `graph`
 *     only: magg[i] = sum_j att_ij m_ij [N,H], xsum[i] = sum_j (x_i - x_j) s_ij [N,3] (no 1/deg).
 *   pvs_egnn_layer_fwd_partial: EGNNLayer.forward where `graph` holds only part of every row's edges
 *     and the rest enters as base_magg [N,H], base_xsum [N,3], base_deg [N] (edge counts as floats):
 *     M = base_magg + sums over graph, x' = x + (base_xsum + sums) / max(base_deg + deg_graph, 1).
 * No edge_residual, no softmax attention, H = 32, 64 or 128 (the MFMA edge forward: the generic kernels of H = 16 and
 * of PVS_EGNN_KERNELS=generic are refused); no backward. Workspace:
 * pvs_egnn_layer_workspace_bytes(desc, N, E, 2). */
int pvs_egnn_layer_edge_sums(const PvsLayerDesc* desc, const PvsGraph* graph, const PvsLayerParams* params,
                             const float* h, const float* x, float* magg, float* xsum,
                             void* workspace, size_t workspace_bytes, pvs_stream_t stream);
int pvs_egnn_layer_fwd_partial(const PvsLayerDesc* desc, const PvsGraph* graph, const PvsLayerParams* params,
                               const float* h, const float* x, const float* base_magg, const float* base_xsum,
                               const float* base_deg, float* h_out, float* x_out, float* node_att_out,
                               float* saved, void* workspace, size_t workspace_bytes, pvs_stream_t stream);
/* pvs_egnn_layer_fwd_partial that also hands out the layer's edge attention: att_out [>= max(E, 1)], CSR-sorted over
 * `graph` (entry e belongs to edge e of graph->row / col; with a device-side edge count the entries from that count
 * on are left as they are), or NULL: the attention stays in the workspace, which is pvs_egnn_layer_fwd_partial -
 * the same launches, the same h_out / x_out bits either way. Meaningful for a layer with PVS_EDGE_ATTENTION. */
int pvs_egnn_layer_fwd_partial_att(const PvsLayerDesc* desc, const PvsGraph* graph, const PvsLayerParams* params,
                                   const float* h, const float* x, const float* base_magg, const float* base_xsum,
                                   const float* base_deg, float* h_out, float* x_out, float* node_att_out,
                                   float* att_out, float* saved, void* workspace, size_t workspace_bytes,
                                   pvs_stream_t stream);

/* The same reuse for layers with PVS_EDGE_ATTENTION | PVS_SOFTMAX_ATT (and only for them: every other layer is refused
 * here, as softmax layers are refused by the three entries above). Row sums of two edge sets do not add under a softmax,
 * but its statistics merge exactly. For a row i and an edge set T with logits l_e = w_a.m_e + b_a:
 *   mu_T = max l_e,  S_T = sum exp(l_e - mu_T),  A_T = sum exp(l_e - mu_T) m_e / S_T      (S_T >= 1 for a set with an edge)
 * and for the base set b and the set g of `graph`, with mu = max(mu_b, mu_g), a_b = S_b exp(mu_b - mu), a_g = S_g exp(mu_g - mu):
 *   M_i = (a_b A_b + a_g A_g) / (a_b + a_g),   att_e = exp(l_e - mu_g) / S_g * a_g / (a_b + a_g)  for e in g.
 * A set without an edge in row i contributes nothing; a row without any edge has M_i = 0. The coordinate sums are not
 * attention weighted: base_xsum / base_deg are those of pvs_egnn_layer_edge_sums.
 * A BASE ROW is H + 4 floats: A_b [H] | mu_b | S_b | 0 | 0; an all-zero row means "no base". base_rows [N, H + 4] is
 * 16-byte aligned.
 *   pvs_egnn_layer_edge_stats_softmax: base rows and xsum [N,3] (no 1/deg) over the edges of `graph`; rows without an
 *     edge are all zero.
 *   pvs_egnn_layer_fwd_partial_softmax: the contract of pvs_egnn_layer_fwd_partial_att (a device-side edge count and
 *     n_norm_rows_dev are honoured, x_out must not alias x); att_out, or NULL, receives the attention of graph's edges
 *     normalised over ALL edges of their rows (entries behind a device-side count are left as they are); h_out, x_out and
 *     node_att_out have the same bits with and without it.
 * H = 32, 64 or 128 on the MFMA edge forward, no edge_residual, no backward, the same bits on every run. Workspace of both:
 * pvs_egnn_layer_workspace_bytes(desc, N, E, 3). */
int pvs_egnn_layer_edge_stats_softmax(const PvsLayerDesc* desc, const PvsGraph* graph, const PvsLayerParams* params,
                                      const float* h, const float* x, float* base_rows, float* xsum,
                                      void* workspace, size_t workspace_bytes, pvs_stream_t stream);
int pvs_egnn_layer_fwd_partial_softmax(const PvsLayerDesc* desc, const PvsGraph* graph, const PvsLayerParams* params,
                                       const float* h, const float* x, const float* base_rows, const float* base_xsum,
                                       const float* base_deg, float* h_out, float* x_out, float* node_att_out,
                                       float* att_out, float* saved, void* workspace, size_t workspace_bytes,
                                       pvs_stream_t stream);

/* The edges of `full` that touch a ligand atom (bp == 0), as a CSR over the same nodes, without a
 * host round trip: rowptr_out [N+1] (its last entry = the edge count, pass it as
 * PvsGraph.n_edges_dev), row/col/etype_out with room for `capacity` edges (the call fails through
 * *status bit 2 if they do not fit). For pvs_egnn_layer_fwd_partial. */
size_t pvs_graph_filter_workspace_bytes(int32_t n_nodes);
int pvs_graph_filter_ligand_edges(const PvsGraph* full, const uint8_t* bp, int32_t capacity,
                                  int32_t* rowptr_out, int32_t* row_out, int32_t* col_out, uint8_t* etype_out,
                                  int32_t* status, void* workspace, size_t workspace_bytes, pvs_stream_t stream);

/* The radius graphs of B rigid poses of one ligand against one receptor without re-testing the
 * receptor-receptor pairs (they are pose independent: rr_rowptr [n_rec+1] / rr_col, receptor-local
 * ids, from pvs_radius_graph_* on the receptor alone). Node layout per pose: n_lig (1..1024) ligand
 * atoms first, then the n_rec receptor atoms; lig_pos [B,n_lig,3], rec_pos [n_rec,3]. A ligand atom's contacts
 * with its own ligand are kept in ceil(n_lig / 64) mask words (the state grows by that much). Same edges,
 * classes and in-row order as generate_edges per pose. Outputs: the full CSR (rowptr [N+1], row,
 * col, etype with room for `capacity` edges, inv_deg [N]) and the CSR of its ligand-touching edges
 * (`_lig`), both with the edge count only on the device (rowptr[N]; pass it as PvsGraph.n_edges_dev:
 * forward-only use). *status bit 2 = a capacity was too small (nothing is written then). */
size_t pvs_screen_graph_state_bytes(int32_t n_poses, int32_t n_lig, int32_t n_rec);
int pvs_screen_graph_build(const float* lig_pos, const float* rec_pos, const int32_t* rr_rowptr,
                           const int32_t* rr_col, int32_t n_poses, int32_t n_lig, int32_t n_rec,
                           double inter_radius, double intra_radius, int32_t capacity, int32_t capacity_lig,
                           int32_t* rowptr, int32_t* row, int32_t* col, uint8_t* etype, float* inv_deg,
                           int32_t* rowptr_lig, int32_t* row_lig, int32_t* col_lig, uint8_t* etype_lig,
                           int32_t* status, void* state, size_t state_bytes, pvs_stream_t stream);

/* Library batches: the same graphs for a batch whose n_slots slots hold one pose each of DIFFERENT ligands
 * (0..slot_cap atoms per slot, 0 = the receptor alone) against the one receptor, described by one job
 * (PvsScreenSlotsJob below). No field depends on the batch's composition, so one captured step serves every batch of a
 * library.
 *   lig_pos [lig_cap,3]: the ligand atoms of all slots, packed; lig_ptr [n_slots+1] (device, int32, lig_ptr[0] = 0):
 *     slot p holds the atoms lig_ptr[p] .. lig_ptr[p+1]; lig_ptr[n_slots] <= lig_cap <= slot_cap * n_slots, slot_cap =
 *     1..1024 (ceil(slot_cap / 64) ligand-ligand mask words per packed atom in the state).
 *   Node layout (compact): slot p owns the nodes node_ptr[p] .. node_ptr[p+1], node_ptr[p] = lig_ptr[p] + p * n_rec,
 *     its ligand atoms first, then the n_rec receptor atoms. The nodes from node_ptr[n_slots] up to
 *     N_cap = lig_cap + n_slots * n_rec are padding: degree 0, inv_deg 1, graph id -1, zero rows in every table.
 *   Outputs as the call above over N_cap nodes (full.rowptr / lig.rowptr [N_cap+1], inv_deg [N_cap]; edges, classes and
 *     in-row order per slot those of generate_edges; both edge counts on the device; `full` and `lig` have room for
 *     their `capacity` edges), plus the node tables of the layer stack: node_ptr [n_slots+1] (= the batch's graph ptr),
 *     node_graph [N_cap], pos [N_cap,3] and, from `tables`, feats [N_cap,n_feats] (ligand rows from lig_feats
 *     [lig_cap,n_feats], receptor rows from rec_feats [n_rec,n_feats]; feats may be NULL) and the first-layer receptor
 *     sums base_magg [N_cap,hidden], base_xsum [N_cap,3], base_deg [N_cap] expanded from rec_magg / rec_xsum / rec_deg
 *     [n_rec,.] with zeros on ligand and padding rows (base_magg may be NULL: none of the three is written).
 *   *status: bit 2 = a capacity was too small (no edge is written then); bit 3 = lig_ptr is not such a table (the
 *     outputs then describe N_cap padding nodes and no edge). */
typedef struct {
    int32_t n_feats, hidden;
    const float *lig_feats, *rec_feats;
    const float *rec_magg, *rec_xsum, *rec_deg;
    float *feats, *base_magg, *base_xsum, *base_deg;
} PvsRaggedNodeTables;

/* One CSR a builder writes: rowptr [N_cap+1], row / col / etype with room for `capacity` edges. */
typedef struct PvsCsrOut { int32_t *rowptr, *row, *col; uint8_t* etype; int32_t capacity; } PvsCsrOut;

/* What a slot of the batch is. The layout is stated, never inferred from which pointers are set: a field that the
 * stated layout does not take must be NULL / 0, and a field it needs must be there.
 *
 * PVS_SLOTS_STRUCK: PVS_SLOTS_RAGGED plus rec_drop [n_slots] (int32, DEVICE): -1, or the receptor atom
 * r in 0..n_rec-1 that the slot's receptor lacks (receptor-atom and contact masking of a sweep's hits:
 * attribution_fns.py atom_masking / bond_masking remove atoms together with their edges). A struck slot owns
 * n_lig + n_rec - 1 rows - its ligand atoms, then the receptor atoms in order without r - so node_ptr[p] = lig_ptr[p] +
 * p * n_rec - (struck slots before p) and the rows from node_ptr[n_slots] on are padding. Its full CSR is the unstruck
 * slot's without every edge that touches r, ids above r moved down by one, classes and in-row order kept; inv_deg from
 * the new degrees. A receptor row that had r in its template row cannot start from the cached receptor sums: its
 * base_magg / base_xsum / base_deg are zero and its row of the ligand-touching CSR is its WHOLE row (ligand entries,
 * then the class-2 entries that remain); every other row is as without rec_drop. With every entry -1 all outputs are
 * those of PVS_SLOTS_RAGGED. *status as there; bit 3 also for an entry of rec_drop outside
 * -1..n_rec-1 (an edgeless batch). lig.capacity needs room for the whole rows of the touched receptor rows.
 *
 * PVS_SLOTS_CROPPED: PVS_SLOTS_RAGGED where slot p keeps receptor atom j only if one of the slot's ligand
 * atoms is closer to it than crop_radius (> 0) - the crop of the training loader (data_loaders.py: make_box with
 * relative_to_ligand) per pose: fp64 on the fp32 coordinates, `<` strict and without a lower bound (a coincident atom is
 * kept); an empty slot keeps nothing. keep [n_slots, ceil(n_rec / 64)] (uint64, DEVICE, an output): bit j % 64 of word
 * j / 64 of row p is set for a kept atom. A slot owns its ligand atoms, then its kept receptor atoms in receptor order,
 * compact: node_ptr[p + 1] = node_ptr[p] + n_lig_p + kept_p, padding from node_ptr[n_slots] up to N_cap = lig_cap +
 * n_slots * n_rec as above. The slot's graph is generate_edges on the cropped complex: ligand-touching edges by
 * distance, to kept atoms only (crop_radius may be below an edge radius); receptor-receptor edges from the template
 * where both ends are kept, renumbered by rank in the mask, no distance evaluated. Written: the full CSR (full.rowptr,
 * row, col, etype, inv_deg; edge count in full.rowptr[N_cap]), node_ptr, node_graph, pos, keep and tables.feats. NOT
 * written: the ligand-touching CSR (`lig` is ignored and may be all zero) and the base_* tables (ignored, whatever they
 * hold: a row at the rim of the crop has lost template neighbours, so the receptor's first-layer sums are not its
 * sums). full.capacity as for the uncropped layouts bounds the cropped graph, which is a subset. *status as above. No
 * atomics: the same bits on every run. */
enum { PVS_SLOTS_RAGGED = 0, PVS_SLOTS_STRUCK = 1, PVS_SLOTS_CROPPED = 2 };
typedef struct PvsScreenSlotsJob {
    int32_t layout;                 /* PVS_SLOTS_* */
    const float* lig_pos; const int32_t* lig_ptr; const int32_t* rec_drop;   /* rec_drop: STRUCK only */
    const float* rec_pos; const int32_t *rr_rowptr, *rr_col;    /* the template as for pvs_screen_graph_build */
    int32_t n_slots, lig_cap, n_rec, slot_cap;
    double inter_radius, intra_radius, crop_radius;                          /* crop_radius: CROPPED only */
    PvsCsrOut full, lig;            /* lig: the ligand-touching CSR; ignored by CROPPED */
    float* inv_deg; int32_t *node_ptr, *node_graph; float* pos;
    uint64_t* keep;                 /* CROPPED only */
    PvsRaggedNodeTables tables;     /* by value; all zero = none */
    int32_t* status;
} PvsScreenSlotsJob;
/* The bytes of `state` for the job's layout and counts (no pointer of the job is read); 0 for counts or a layout that
 * pvs_screen_slots_build refuses. Every refusal of the build happens on the host, before anything is launched. */
size_t pvs_screen_slots_state_bytes(const PvsScreenSlotsJob* job);
int pvs_screen_slots_build(const PvsScreenSlotsJob* job, void* state, size_t state_bytes, pvs_stream_t stream);

/* Cropped copies: PVS_SLOTS_CROPPED slots whose keep mask is decided from OTHER atoms than the slot's own - the
 * leave-out copies of a hit on its cropped complex (the reference's attribution_fns.atom_masking / bond_masking get
 * the loader's complex, cropped around the WHOLE ligand, and strike atoms out of that one; a copy is never cropped
 * again around what is left of it). `slots` is a PVS_SLOTS_CROPPED job by value (its own rec_drop stays NULL; every
 * refusal of pvs_screen_slots_build applies to it), beside it three tables:
 *   crop_pos [crop_cap,3] / crop_ptr [n_slots+1] (DEVICE, int32, crop_ptr[0] = 0): the atoms that slot p is cropped
 *     AROUND, packed like lig_pos / lig_ptr; a crop set has 0..1024 atoms, 1 <= crop_cap <= 1024 * n_slots.
 *   rec_drop [n_slots] (DEVICE, int32; NULL = all -1): -1, or the receptor atom that the slot's receptor lacks.
 * Slot p keeps receptor atom j iff some atom of crop_pos[crop_ptr[p] .. crop_ptr[p+1]) is closer to it than
 * slots.crop_radius - the decision of PVS_SLOTS_CROPPED, made by the same kernel: fp64 on the fp32 coordinates, strict,
 * no lower bound; an empty crop set keeps nothing - and j != rec_drop[p]. A rec_drop[p] that names an atom the crop does
 * not keep changes nothing. Everything else is PVS_SLOTS_CROPPED: the slot's rows are its OWN ligand atoms (slots.lig_pos
 * / lig_ptr), then the kept atoms in receptor order; ligand edges by distance to kept atoms only; template edges where
 * both ends are kept; slots.keep is an output, only the full CSR is written, the base tables are ignored. With crop_pos /
 * crop_ptr = the ligand table and no rec_drop every output is that of pvs_screen_slots_build on `slots`, bit for bit.
 * *slots.status: as there; bit 3 (an edgeless batch of padding rows) also when crop_ptr is not an ascending table from 0
 * inside crop_cap, a crop set has more than 1024 atoms or rec_drop has an entry outside -1..n_rec-1. The status word has
 * one writer and no launch clears it; no atomics: the same bits on every run. The state is that of `slots`. Under
 * GraphNorm the copies of one batch normalise each other, as in every batched route. */
typedef struct PvsScreenCopiesJob {
    PvsScreenSlotsJob slots;        /* by value; layout PVS_SLOTS_CROPPED, rec_drop NULL */
    const float* crop_pos; const int32_t* crop_ptr;
    const int32_t* rec_drop;        /* may be NULL */
    int32_t crop_cap;
} PvsScreenCopiesJob;
size_t pvs_screen_copies_state_bytes(const PvsScreenCopiesJob* job);
int pvs_screen_copies_build(const PvsScreenCopiesJob* job, void* state, size_t state_bytes, pvs_stream_t stream);

/* The keep decision of PVS_SLOTS_CROPPED for packed hits, without building anything (which receptor atoms each hit's
 * cropped complex has: receptor_atom_masking(atoms='all') of a cropped sweep). lig_pos [n_rows,3] / lig_ptr [n_hits+1]
 * (DEVICE, int32; a hit has 0..1024 atoms) against rec_pos [n_rec,3]. keep [n_hits, ceil(n_rec / 64)] uint64: bit
 * j % 64 of word j / 64 of row s is set when some atom of hit s is closer to receptor atom j than crop_radius (> 0);
 * kept_ptr [n_hits+1] int32: the exclusive scan of the hits' kept counts (the host reads kept_ptr[n_hits], one copy
 * back). A lig_ptr that does not ascend from 0 inside n_rows, or a hit of more than 1024 atoms: keep and kept_ptr all
 * zero and kept_ptr[n_hits] = -1. Two launches (the builders' keep kernel, one scan), no atomics: the same bits every
 * time. */
int pvs_crop_keep(const float* lig_pos, const int32_t* lig_ptr, int32_t n_hits, int32_t n_rows, const float* rec_pos,
                  int32_t n_rec, double crop_radius, uint64_t* keep, int32_t* kept_ptr, pvs_stream_t stream);

/* Complex batches: the node tables of B protein-ligand complexes built from a device-resident pool of structure
 * files, as the reference loader builds one sample on the host (data_loaders.py:259-309: ligand then receptor, crop of
 * the receptor to the atoms closer than `radius` to some ligand atom - fp64, scipy's cdist decision -, hydrogen filter
 * after the crop, make_bit_vector features, fp32 coordinates).
 *   pool: every unique receptor / ligand file once. *_xyz [atoms,3] fp64 as stored, *_types (smina type) and *_z
 *     (atomic number) [atoms] int32, rec_ptr [n_rec+1] / lig_ptr [n_lig+1] int32 atom offsets of the files.
 *   pairs [B,3] int32: receptor id, ligand id, offset of the sample's flags in the workspace (the running sum of
 *     ligand + receptor atom counts of the samples before it; n_atoms_in = that sum over the whole batch).
 *   lig_xform [B,3,3] fp64 or NULL: ligand coordinates become x @ M before anything else (augmented actives; products
 *     and sums rounded one by one, x0*M0j + x1*M1j, then + x2*M2j). rot [B,3,3] fp64 or NULL: applied the same way
 *     to `pos` only.
 * _count: counts [B,2] = kept ligand atoms, kept receptor atoms of every sample; one flag per input atom in the
 *   workspace. *status is reset, then bit 0 = a pair outside the pool or the workspace, bit 1 = a ligand of more than
 *   1024 atoms (the counts of such a sample are 0).
 * _fill (same pool, pairs, lig_xform, workspace; graph_ptr [B+1] = the running sum of the counts, total_nodes its
 *   last entry): x [N,F] (F = n_features + 1 compact, else 2 n_features; class = smina type, or class_of_z
 *   [128][atomic number] with numbers outside the table in class n_features; receptor classes + n_features), pos [N,3],
 *   pos_graph [N,3] or NULL (the coordinates before `rot`: what the edge list is built from), bp [N] (0 ligand,
 *   1 receptor), batch [N] int64. Node order per sample: ligand atoms in file order, then the surviving receptor atoms
 *   in file order. *status: bit 2 = a class outside the encoding (one_hot of the reference raises), bit 3 = graph_ptr
 *   does not match the counts (nothing is written outside a sample's rows).
 * pvs_complex_edges: the arrays of pvs_radius_graph_fill over the batch -> the loader's edge list, graph by graph the
 *   inter block then the intra block, each row-major (the 'generate_edges' layout): edge_index [2,E] int64, edge_attr
 *   [E,3] int64 one-hot. *status bit 4 = inconsistent tables. Bitwise reproducible; no host synchronisation in any. */
typedef struct {
    const double *rec_xyz, *lig_xyz;
    const int32_t *rec_types, *lig_types, *rec_z, *lig_z;
    const int32_t *rec_ptr, *lig_ptr;
    int32_t n_rec, n_lig;
} PvsComplexPool;
size_t pvs_complex_batch_workspace_bytes(int32_t n_samples, int32_t n_atoms_in);
int pvs_complex_batch_count(const PvsComplexPool* pool, const int32_t* pairs, const double* lig_xform,
                            int32_t n_samples, int32_t n_atoms_in, double radius, int32_t keep_hydrogens,
                            int32_t* counts, int32_t* status, void* workspace, size_t workspace_bytes,
                            pvs_stream_t stream);
int pvs_complex_batch_fill(const PvsComplexPool* pool, const int32_t* pairs, const double* lig_xform,
                           const double* rot, int32_t n_samples, int32_t n_atoms_in, int32_t total_nodes,
                           int32_t use_atomic_numbers, int32_t n_features, int32_t compact, const int32_t* class_of_z,
                           const int32_t* counts, const int32_t* graph_ptr, float* x, float* pos, float* pos_graph,
                           uint8_t* bp, int64_t* batch, int32_t* status, const void* workspace,
                           size_t workspace_bytes, pvs_stream_t stream);
int pvs_complex_edges(int32_t n_nodes, int32_t n_edges, int32_t n_graphs, const int32_t* graph_ptr,
                      const int32_t* rowptr, const int32_t* inter_ptr, const int32_t* intra_ptr, const int32_t* row,
                      const int32_t* col, const uint8_t* etype, const int32_t* perm, int64_t* edge_index,
                      int64_t* edge_attr, int32_t* status, pvs_stream_t stream);

/* Complex batches at fixed capacities (forward only): the node tables and the CSR of a batch whose sizes never reach the
 * host, so that one captured step serves every batch of a types file. Every size below is a capacity chosen by the host;
 * the launches depend on the capacities alone; no allocation, no host synchronisation, bitwise reproducible.
 * pvs_complex_batch_build_cap = pvs_complex_batch_count + the running sum of its counts + pvs_complex_batch_fill, bit for
 *   bit: pairs [B,3] as above (a static device buffer the caller rewrites), atoms_in_cap >= the batch's input atoms
 *   (workspace: pvs_complex_batch_workspace_bytes(B, atoms_in_cap)). Outputs: counts [B,2], node_ptr [B+1] (device),
 *   x [node_cap,F], pos [node_cap,3], pos_graph [node_cap,3] or NULL, bp [node_cap], node_graph [node_cap] int32 (the
 *   sample of every row). Rows at or behind node_ptr[B] are padding: zeros, node_graph -1. Every row of every output is
 *   written by every call. *status is reset, then bits 0-3 as for _count / _fill, and
 *     PVS_CAP_NODE_OVERFLOW   more nodes than node_cap: the samples that end behind node_cap are left out whole (their
 *                             rows are padding); node_ptr keeps the true offsets
 *     PVS_CAP_EMPTY_SAMPLE    a sample with no atom left after crop and hydrogen filter
 * pvs_radius_graph_build_cap = pvs_radius_graph_count + _fill over node_cap rows with graph_ptr = that device node_ptr:
 *   rowptr [node_cap+1], row / col / etype [edge_cap], inv_deg [node_cap], in-row order as _fill (inter entries by
 *   ascending column, then intra entries); no perm, no by-column lists. Rows at or behind graph_ptr[B] have degree 0,
 *   inv_deg 1 and rowptr = E, so rowptr[node_cap] is the edge count. n_edges_fwd [1] (device) is the count to hand to a
 *   forward (PvsGraph.n_edges_dev): E where row / col / etype were written, 0 on any of the three overflows below, whose
 *   row / col / etype are an earlier call's and do not belong to this rowptr. state:
 *   pvs_radius_graph_state_bytes(node_cap, n_graphs, graph_node_cap). *status is reset first when reset_status != 0
 *   (0: the word of the node call goes on), then
 *     PVS_CAP_NODE_OVERFLOW   graph_ptr is no offset table inside node_cap rows
 *     PVS_CAP_GRAPH_OVERFLOW  a graph of more than graph_node_cap nodes (either: rowptr all 0, inv_deg all 1)
 *     PVS_CAP_EDGE_OVERFLOW   more than edge_cap edges: rowptr and inv_deg hold the true counts
 *   On any of the three nothing is written to row / col / etype. No access leaves a buffer whatever the tables hold. */
#define PVS_CAP_NODE_OVERFLOW 32
#define PVS_CAP_GRAPH_OVERFLOW 64
#define PVS_CAP_EDGE_OVERFLOW 128
#define PVS_CAP_EMPTY_SAMPLE 256
int pvs_complex_batch_build_cap(const PvsComplexPool* pool, const int32_t* pairs, const double* lig_xform,
                                const double* rot, int32_t n_samples, int32_t atoms_in_cap, int32_t node_cap,
                                double radius, int32_t keep_hydrogens, int32_t use_atomic_numbers, int32_t n_features,
                                int32_t compact, const int32_t* class_of_z, int32_t* counts, int32_t* node_ptr, float* x,
                                float* pos, float* pos_graph, uint8_t* bp, int32_t* node_graph, int32_t* status,
                                void* workspace, size_t workspace_bytes, pvs_stream_t stream);
int pvs_radius_graph_build_cap(const float* pos, const uint8_t* bp, const int32_t* graph_ptr, int32_t n_graphs,
                               int32_t node_cap, int32_t graph_node_cap, double inter_radius, double intra_radius,
                               int32_t pair_filter, int32_t edge_cap, int32_t* rowptr, int32_t* row, int32_t* col,
                               uint8_t* etype, float* inv_deg, int32_t* n_edges_fwd, int32_t* status,
                               int32_t reset_status, void* state, size_t state_bytes, pvs_stream_t stream);

/* Leave-out graph batch of masking attribution (the reference's atom_masking / bond_masking loops,
 * attribution/attribution_fns.py:39-115, 356-456, which rebuild one masked edge list per atom on the host).
 * `parent`: the prepared graph of ONE complex (rowptr / col / etype; host-side edge count); drop [n_masks, 2] int32:
 * the node(s) each copy leaves out, drop[b][1] = -1 (or = drop[b][0]) for a single node. Output: the PvsGraph arrays of
 * the disjoint union of n_masks copies, copy b without its dropped nodes and every edge touching them, node ids
 * renumbered densely. The arrays equal what pvs_graph_prepare makes of the masked COO lists (same order inside a row,
 * duplicate edges kept); no sort is run: a row-sorted list with rows removed is row-sorted. Forward-only (no perm, no
 * by-column lists).
 *   total_nodes: the caller's count of output nodes (n_masks * N less one or two per copy), the size of the node arrays
 *   capacity:    room for edges in row / col / etype, <= n_masks * E; exact_edges != 0: the caller has counted the
 *                surviving edges on the host and `capacity` IS that count (any other count is an error, bit 4)
 *   rowptr [total_nodes + 1] (its last entry = the edge count, usable as PvsGraph.n_edges_dev), row / col / etype
 *   [capacity] (etype NULL exactly when the parent has none), inv_deg [total_nodes],
 *   src_node [total_nodes]: the parent node each output node is (gather features and coordinates with it),
 *   graph_ptr / graph_eptr [n_masks + 1]: first node / first edge of every copy (PvsGraph.graph_eptr).
 * *status: bit 0 = a node id outside [0, N) (second id: [-1, N)), bit 2 = more than `capacity` edges, bit 3 =
 * total_nodes does not match the table, bit 4 = exact_edges and another edge count; no edge is written then. Bitwise reproducible; no host synchronisation. */
size_t pvs_mask_graph_workspace_bytes(int32_t n_nodes, int32_t n_masks);
int pvs_mask_graph_build(const PvsGraph* parent, const int32_t* drop, int32_t n_masks, int32_t total_nodes,
                         int32_t capacity, int32_t exact_edges, int32_t* rowptr, int32_t* row, int32_t* col,
                         uint8_t* etype, float* inv_deg, int32_t* src_node, int32_t* graph_ptr, int32_t* graph_eptr,
                         int32_t* status, void* workspace, size_t workspace_bytes, pvs_stream_t stream);

/* Backward of the above (what autograd replays for the reference, SURVEY.md §8a "Backward spec").
 *   g_h_out [N,H]; g_x_out [N,3] or NULL (=0: the last layer's x is unused);
 *   g_m_out [E,H] sorted or NULL (=0); att [E] sorted as written by the forward.
 *   g_h [N,H], g_x [N,3] (NULL to skip), g_m_prev [E,H] sorted (required iff edge residual applied)
 *   grads: members may be NULL to skip (coord_* MUST be NULL-safe: they are None for the last layer).
 */
int pvs_egnn_layer_bwd(const PvsLayerDesc* desc, const PvsGraph* graph, const PvsLayerParams* params,
                       const float* h, const float* x, const float* m_prev, const float* att,
                       const float* saved,
                       const float* g_h_out, const float* g_x_out, const float* g_m_out,
                       float* g_h, float* g_x, float* g_m_prev, const PvsLayerGrads* grads,
                       void* workspace, size_t workspace_bytes, pvs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The whole EGNNLayer stack of SartorrasEGNN.get_embeddings (egnn_satorras.py:325-328, `for layer in self.layers:
 * feats, coords, edge_attributes, edge_messages = layer(...)`) as ONE call each way. The same launches as n_layers calls of
 * pvs_egnn_layer_fwd / _bwd in a row (bit for bit the same results): what it removes is the host's share - one autograd
 * node, one ctypes call and ~15 allocations per layer and direction - which is what bounds a training step at the
 * reference's default shape (32 graphs of ~500 atoms, ~70 launches of a few microseconds: SURVEY.md §8f row 2).
 * All layers share one hidden size; layers with PVS_EDGE_RESIDUAL are refused (their [E,H] messages travel from layer to
 * layer: per-layer calls). Every layer's tensors sit in caller-owned buffers at the strides of PvsStackStrides (in
 * floats, multiples of 4):
 *   h_mid [n_layers-1][>= N*H], x_mid [n_layers-1][>= N*3]: outputs of layers 0 .. n_layers-2 (= inputs of 1 .. n_layers-1);
 *   h_out [N,H], x_out [N,3]: outputs of the last layer; att [n_layers][>= max(E,1)] (NULL unless a layer has edge
 *   attention), node_att [n_layers][>= N] (may be NULL), saved [n_layers][>= pvs_egnn_layer_saved_floats()].
 * Backward: g_h_out [N,H]; g_x_out [N,3] or NULL; g_h0 [N,H]; g_x0 [N,3] or NULL to skip; grads [n_layers]
 * (members NULL to skip, as in pvs_egnn_layer_bwd). Workspace: pvs_egnn_stack_workspace_bytes (the backward's holds the
 * two ping-pong gradient rows between layers).
 */
typedef struct PvsStackStrides {
    int64_t h_mid, x_mid, att, node_att, saved;
} PvsStackStrides;
size_t pvs_egnn_stack_workspace_bytes(const PvsLayerDesc* descs, int32_t n_layers, int32_t n_nodes, int32_t n_edges,
                                      int32_t backward);
int pvs_egnn_stack_fwd(const PvsLayerDesc* descs, const PvsLayerParams* params, int32_t n_layers,
                       const PvsGraph* graph, const PvsStackStrides* strides, const float* h0, const float* x0,
                       float* h_mid, float* x_mid, float* h_out, float* x_out, float* att, float* node_att,
                       float* saved, void* workspace, size_t workspace_bytes, pvs_stream_t stream);
int pvs_egnn_stack_bwd(const PvsLayerDesc* descs, const PvsLayerParams* params, int32_t n_layers,
                       const PvsGraph* graph, const PvsStackStrides* strides, const float* h0, const float* x0,
                       const float* h_mid, const float* x_mid, const float* att, const float* saved,
                       const float* g_h_out, const float* g_x_out, float* g_h0, float* g_x0,
                       const PvsLayerGrads* grads, void* workspace, size_t workspace_bytes, pvs_stream_t stream);

/* GraphNorm's statistics as an operator (torch_geometric GraphNorm called without a batch vector, egnn_satorras.py:120):
 * stats[0:H] = mean_c over the rows of y1 [n_rows_cap, H], stats[H:2H] = mean_c of (y1 - mean_scale * mean)^2.
 * n_rows_dev NULL: over all n_rows_cap rows (>= 1), the launches a layer makes for a graph without
 * PvsGraph.n_norm_rows_dev. Otherwise a DEVICE int32 n, clamped to [0, n_rows_cap]: over the first n rows, as described at
 * that member (rows >= n never read, n = 0 gives zeros, n >= 1 the bits of the NULL call on n rows). H <= 256.
 * No atomics; the same bits every call. */
size_t pvs_graphnorm_stats_rows_workspace_bytes(int32_t n_rows_cap, int32_t H);
int pvs_graphnorm_stats_rows(const float* y1, const float* mean_scale, int32_t n_rows_cap, int32_t H,
                             const int32_t* n_rows_dev /* or NULL: n_rows_cap */, float* stats /* [2H] */,
                             void* workspace, size_t workspace_bytes, pvs_stream_t stream);

/* The same per node segment (what a layer computes under PVS_GRAPHNORM_SEGMENTS): stats [n_segments, 2H], row s = the pair of
 * the rows [seg_ptr[s], seg_ptr[s + 1]) of y1 [n_rows_cap, H] - bit for bit pvs_graphnorm_stats_rows on those rows alone.
 * seg_ptr: DEVICE int32 [n_segments + 1], read when the kernels run, every entry clamped to [0, n_rows_cap], a segment's
 * length max(0, seg_ptr[s + 1] - seg_ptr[s]); expected non-decreasing (a table that is not stays within the workspace, but
 * segments that overlap may then get each other's sums). Length 0: mean = var = 0. Rows outside every segment are never
 * read. n_segments >= 1, H <= 256. No atomics; the same bits every call. */
size_t pvs_graphnorm_stats_segments_workspace_bytes(int32_t n_rows_cap, int32_t n_segments, int32_t H);
int pvs_graphnorm_stats_segments(const float* y1, const float* mean_scale, int32_t n_rows_cap, int32_t H,
                                 const int32_t* seg_ptr /* [n_segments + 1] */, int32_t n_segments,
                                 float* stats /* [n_segments, 2H] */, void* workspace, size_t workspace_bytes,
                                 pvs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * The thin callers either side of the layer stack.
 * y = x W^T + b: PygLinearPass.forward (pnn_geometric_base.py:83-94) and each nn.Linear of the
 * feats_linear_layers head (egnn_satorras.py:304-316, egnn_multitask.py:141-146).
 */
int pvs_linear_fwd(const float* x, const float* w, const float* b /*NULL if no bias*/, float* y,
                   int32_t n_rows, int32_t n_in, int32_t n_out, pvs_stream_t stream);
size_t pvs_linear_bwd_workspace_bytes(int32_t n_rows, int32_t n_in, int32_t n_out);
int pvs_linear_bwd(const float* x, const float* w, const float* g_y,
                   float* g_x /*NULL to skip*/, float* g_w, float* g_b /*NULL if no bias*/,
                   int32_t n_rows, int32_t n_in, int32_t n_out,
                   void* workspace, size_t workspace_bytes, pvs_stream_t stream);

/* global_mean_pool(feats, batch, size) (pnn_geometric_base.py:29-33, egnn_multitask.py:158-161):
 * nodes of one graph are contiguous (PyG collation); graph_ptr [B+1] int32 node offsets. */
int pvs_mean_pool_fwd(const float* h, const int32_t* graph_ptr, float* pooled,
                      int32_t n_graphs, int32_t width, pvs_stream_t stream);
int pvs_mean_pool_bwd(const float* g_pooled, const int32_t* graph_ptr, float* g_h,
                      int32_t n_graphs, int32_t n_nodes, int32_t width, pvs_stream_t stream);

/* global_mean_pool followed by the head's first Linear (pnn_geometric_base.py:29-36: `feats_linear_layers(global_mean_pool(
 * feats, batch))`; egnn_multitask.py:158-166) in one launch, and the backward of the pair in one launch: pooled [B, width]
 * is kept by the caller for the backward; y [B, n_out] = pooled W^T + b (b NULL: no bias). width <= 1024.
 * Backward: g_h [N, width] (NULL to skip), g_w [n_out, width], g_b [n_out] (NULL if no bias). */
int pvs_pool_head_fwd(const float* h, const int32_t* graph_ptr, const float* w, const float* b, float* pooled,
                      float* y, int32_t n_graphs, int32_t width, int32_t n_out, pvs_stream_t stream);
int pvs_pool_head_bwd(const float* g_y, const float* pooled, const float* w, const int32_t* graph_ptr,
                      float* g_h, float* g_w, float* g_b, int32_t n_graphs, int32_t n_nodes, int32_t width,
                      int32_t n_out, pvs_stream_t stream);

/* The pooling once and up to PVS_MAX_POOL_HEADS heads on the pooled row in one launch, forward only (screening a
 * two-headed model: egnn_multitask.py:141-166 evaluates one head per pass, `feats_linear_layers_pose` or
 * `feats_linear_layers_affinity`, over the same pooled embedding). A head is one nn.Linear, W [n_out, width] and b [n_out]
 * (NULL: no bias), followed by nothing, nn.ReLU() or nn.Softplus() with its defaults (beta 1, threshold 20: the input
 * itself above 20); it writes the columns [col, col + n_out) of y [n_graphs, ld_y]:
 *   y[g, col + o] = act(b[o] + sum_k pooled[g, k] W[o, k]),  k ascending, one fused multiply-add per term.
 * The pooled row is formed by the code of the single-head forward above, so with PVS_HEAD_NONE a head's columns are bit
 * for bit what that entry gives with the head's weights. `heads` is a HOST array, copied into the kernel's arguments
 * (no device table: a captured launch keeps them). pooled [n_graphs, width]: NULL to skip. width <= 1024; the column
 * ranges must lie inside ld_y and must not overlap. */
enum { PVS_HEAD_NONE = 0, PVS_HEAD_RELU = 1, PVS_HEAD_SOFTPLUS = 2 };
enum { PVS_MAX_POOL_HEADS = 4 };
typedef struct PvsHead {
    const float* w;
    const float* b;
    int32_t n_out;
    int32_t act;     /* PVS_HEAD_* */
    int32_t col;     /* first column of y this head writes */
} PvsHead;
int pvs_pool_heads_fwd(const float* h, const int32_t* graph_ptr, const PvsHead* heads, int32_t n_heads, float* pooled,
                       float* y, int32_t n_graphs, int32_t width, int32_t ld_y, pvs_stream_t stream);

/* Best row of every segment (the best pose of every ligand of a sweep): scores [P, n_cols], segment s = the rows
 * [seg_ptr[s], seg_ptr[s + 1]) (seg_ptr: DEVICE, ascending, inside [0, P]). best[s] = the row, counted from the
 * segment's first, whose entry in `column` is largest; best_rows[s, :] = that row of scores. Equal values go to the
 * lower row (-0.0 and +0.0 are equal), a NaN never beats a number, -inf is a score like any other. A segment without
 * rows or with nothing but NaNs in `column` gets best = -1 and a row of NaNs. No atomics, no workspace: the result
 * does not depend on the order in which candidates meet (csrc/pose_select.h holds the relation) and is the same bits
 * every time. */
int pvs_segment_argmax(const float* scores, int32_t n_cols, int32_t column, const int32_t* seg_ptr, int32_t n_segments,
                       int32_t* best, float* best_rows, pvs_stream_t stream);

/* Leave-one-atom-out copies of a set of ligands as the slots of a pose batch (atom masking of a sweep's hits through
 * pvs_screen_slots_build: attribution_fns.py:365-431 removes an atom together with its edges, which is the
 * radius graph of the atoms that remain). lig_pos [n_rows, 3], lig_feats [n_rows, n_feats], lig_ptr [n_ligands + 1]
 * (DEVICE): ligand s has n_s = lig_ptr[s + 1] - lig_ptr[s] atoms and owns n_s + 1 consecutive copies - the whole
 * ligand, then the ligand without atom 0, without atom 1, ... (the remaining rows keep their order). Its first copy is
 * number lig_ptr[s] + s; there are lig_ptr[n_ligands] + n_ligands copies in all.
 * Slot k of the batch holds copy first_copy[0] + k (first_copy: ONE int32 in DEVICE memory, so that the host advances
 * it without a launch argument changing); a slot whose copy number is not one of the copies holds nothing. out_ptr
 * [n_slots + 1] = the prefix sum of the slots' atom counts, the rows [out_ptr[k], out_ptr[k + 1]) of out_pos / out_feats
 * = the copy's atoms; out_pos and out_feats have room for n_slots * slot_cap rows, those from out_ptr[n_slots] on are
 * left as they are.
 *   *status is stored by every launch: 0, or bit 3 (the screen builders' "not such a table") when lig_ptr does not
 *   ascend from 0 to at most n_rows or a ligand has more than slot_cap (1..1024) atoms; out_ptr is all zeros then and
 *   no row is written.
 * One launch, no atomics, no workspace: the same bits every time. */
int pvs_leave_out_ligand_pack(const float* lig_pos, const float* lig_feats, const int32_t* lig_ptr, int32_t n_ligands,
                              int32_t n_rows, int32_t n_feats, const int32_t* first_copy, int32_t n_slots,
                              int32_t slot_cap, float* out_pos, float* out_feats, int32_t* out_ptr, int32_t* status,
                              pvs_stream_t stream);

/* The ligand-receptor contacts of packed hits: lig_pos [n_rows, 3] / lig_ptr [n_hits + 1] (DEVICE) against rec_pos
 * [n_rec, 3]. (a, r) - ligand atom a counted inside its hit, receptor atom r - is a contact exactly when the pose-batch
 * builders write a class-1 edge for it: 1e-7 < d < inter_radius on the same fp64 squared distance and compares.
 * _count: pair_ptr [n_hits + 1] = the exclusive scan of the hits' contact counts (the host reads pair_ptr[n_hits], the
 * one copy back); a lig_ptr that does not ascend from 0 inside n_rows gives zeros and pair_ptr[n_hits] = -1.
 * _fill: pairs [n_pairs, 2] int32, the rows pair_ptr[s] .. pair_ptr[s + 1] = hit s's contacts sorted by a, then by r;
 * nothing is written from row n_pairs on. No atomics: the same bits every time. */
int pvs_contact_pairs_count(const float* lig_pos, const int32_t* lig_ptr, int32_t n_hits, int32_t n_rows,
                            const float* rec_pos, int32_t n_rec, double inter_radius, int32_t* pair_ptr,
                            pvs_stream_t stream);
int pvs_contact_pairs_fill(const float* lig_pos, const int32_t* lig_ptr, int32_t n_hits, int32_t n_rows,
                           const float* rec_pos, int32_t n_rec, double inter_radius, const int32_t* pair_ptr,
                           int32_t n_pairs, int32_t* pairs, pvs_stream_t stream);

/* pvs_leave_out_ligand_pack for copies that leave out one ligand-receptor pair, the slots of
 * pvs_screen_slots_build (PVS_SLOTS_STRUCK) (attribution_fns.py bond_masking; with a = -1 or r = -1 a single atom). Hit s owns the
 * rows pair_ptr[s] .. pair_ptr[s + 1] of pairs [n_pairs, 2] (a: ligand atom counted inside the hit or -1; r: receptor
 * atom or -1) and one copy more than rows: the whole ligand, then one copy per row. Its first copy is number
 * pair_ptr[s] + s. Slot k holds copy first_copy[0] + k: the hit's rows without atom a in out_pos / out_feats, out_ptr as
 * above, and rec_drop[k] = r (-1 for a whole ligand and for a slot that holds nothing).
 *   *status: 0, or bit 3 with out_ptr all zeros, rec_drop all -1 and no row written when lig_ptr or pair_ptr does not
 *   ascend from 0 (to at most n_rows / n_pairs), a ligand has more than slot_cap atoms, or a pair row of one of THIS
 *   batch's copies has a outside -1..n_s-1 or r outside -1..n_rec-1.
 * One launch, no atomics, no workspace: the same bits every time. */
int pvs_leave_out_pair_pack(const float* lig_pos, const float* lig_feats, const int32_t* lig_ptr, const int32_t* pairs,
                            const int32_t* pair_ptr, int32_t n_hits, int32_t n_rows, int32_t n_pairs, int32_t n_feats,
                            int32_t n_rec, const int32_t* first_copy, int32_t n_slots, int32_t slot_cap, float* out_pos,
                            float* out_feats, int32_t* out_ptr, int32_t* rec_drop, int32_t* status,
                            pvs_stream_t stream);

/* The PARENTS' atoms for the slots of a leave-out batch: what the slots of pvs_screen_copies_build are cropped around
 * (crop_pos / crop_ptr). lig_pos [n_rows,3] / lig_ptr [n_hits+1] as above; copy_ptr [n_hits+1] (DEVICE, int32): hit s
 * owns the copies copy_ptr[s] + s .. copy_ptr[s+1] + s, both ends included - the numbering of both packers above:
 * copy_ptr = lig_ptr for ligand-atom copies, copy_ptr = pair_ptr for pair copies. Slot k holds copy first_copy[0] + k
 * and gets the WHOLE hit's atoms, whichever atom the copy itself leaves out: the rows [out_ptr[k], out_ptr[k+1]) of
 * out_pos (room for n_slots * slot_cap rows; those from out_ptr[n_slots] on are left as they are). A slot whose copy
 * number is no copy gets none.
 *   *status is stored by every launch: 0, or bit 3 with out_ptr all zeros and no row written when lig_ptr does not
 *   ascend from 0 to at most n_rows, a hit has more than slot_cap (1..1024) atoms or copy_ptr does not ascend from 0.
 * One launch, no atomics, no workspace: the same bits every time. */
int pvs_leave_out_parent_pack(const float* lig_pos, const int32_t* lig_ptr, const int32_t* copy_ptr, int32_t n_hits,
                              int32_t n_rows, const int32_t* first_copy, int32_t n_slots, int32_t slot_cap,
                              float* out_pos, int32_t* out_ptr, int32_t* status, pvs_stream_t stream);

/* Contact attention of a pose batch (the reference's attribution/hotspot.py over attribution_fns.edge_attention,
 * :278-295: per atom the largest attention value over its ligand-receptor edges, per receptor atom the mean of these
 * over the binding events in which it has a contact), reduced on the device over the compact pose-batch layout of
 * pvs_screen_slots_build: slot p owns the rows node_ptr[p] .. node_ptr[p + 1] (node_ptr[p] = lig_ptr[p] +
 * p * n_rec; node_ptr, lig_ptr: DEVICE, [n_slots + 1]), its lig_ptr[p + 1] - lig_ptr[p] ligand atoms first, then the
 * n_rec receptor atoms. rowptr [n_nodes + 1] / etype [n_edges] are either CSR of such a batch (the ligand-touching one
 * or the full one) and att [n_edges] one attention value per edge in THAT CSR's order. An edge counts when its class
 * is 1 (ligand-receptor) wherever it stands in its row; a NaN value is skipped.
 *   lig_att [>= lig_ptr[n_slots]]: per packed ligand atom the largest counted value of its row, NaN for a row without
 *     one; the entries from lig_ptr[n_slots] on are left as they are.
 *   slot_rec_att [n_slots, n_rec]: the same for every receptor atom of every slot (an empty slot: NaN).
 *   rec_sum [n_rec] double, rec_count [n_rec] int32, rec_max [n_rec] float are READ AND UPDATED, so that a captured
 *     step accumulates over its replays: rec_sum += the slot values that are not NaN, added in slot order; rec_count +=
 *     how many there were; rec_max = the largest value so far (a NaN in rec_max means none so far: start it there).
 * Equal values are one value (+0.0 above -0.0), so no result depends on the order in which the edges of a row meet;
 * no atomics: the same bits every time, whatever the launch geometry. A slot whose two tables disagree, that has more
 * than 1024 ligand atoms or whose rows end beyond n_nodes - n_slots * n_rec ligand rows is no slot (NaN, nothing
 * accumulated); edge ranges are clamped to [0, n_edges), so a rowptr of a build that overflowed its edge buffers
 * reads nothing outside them. n_slots == 0 or n_rec == 0: nothing to do, returns 0 without a launch. Two launches. */
int pvs_contact_attention(const int32_t* rowptr, const uint8_t* etype, const float* att, int32_t n_nodes,
                          int32_t n_edges, const int32_t* node_ptr, const int32_t* lig_ptr, int32_t n_slots,
                          int32_t n_rec, float* lig_att, float* slot_rec_att, double* rec_sum, int32_t* rec_count,
                          float* rec_max, pvs_stream_t stream);

/* The heads of pvs_pool_heads_fwd on EVERY row of h [n_rows, width] instead of on a pooled row (the reference's
 * attribution_fns.cam, :312-362: the head applied to each node's final embedding), forward only:
 *   y[n, col + o] = act(b[o] + sum_k h[n, k] W[o, k]),  k ascending, one fused multiply-add per term
 * - the arithmetic of the pooled heads, instruction for instruction (csrc/head_ops.h), so a row of y is bit for bit what
 * pvs_pool_heads_fwd gives for a graph that consists of that row alone. `heads`: a HOST array of 1..PVS_MAX_POOL_HEADS
 * heads, copied into the kernel's arguments; their column ranges must lie inside ld_y and must not overlap; the other
 * columns of y [n_rows, ld_y] are left as they are. width 1..1024. n_rows == 0: returns 0 without a launch. One launch,
 * no workspace, no atomics: the same bits every time. */
int pvs_node_heads_fwd(const float* h, const PvsHead* heads, int32_t n_heads, float* y, int32_t n_rows, int32_t width,
                       int32_t ld_y, pvs_stream_t stream);

/* pvs_contact_attention's reduction over a value that every node has (the class-activation map of a pose batch), over
 * the same compact layout (node_ptr, lig_ptr: DEVICE, [n_slots + 1]; slot p: its ligand atoms, then the n_rec receptor
 * atoms). y [n_nodes, ld_y]; the value of node row r is y[r, col] with n_mean == 1 and
 * ((y[r, col] + y[r, col + 1]) + y[r, col + 2]) / 3.0f with n_mean == 3 (the reference's "three outputs are averaged",
 * in that order, an IEEE division); any other n_mean is refused, as are columns outside ld_y.
 *   lig_val [>= lig_ptr[n_slots]]: the value of every packed ligand atom; the entries from lig_ptr[n_slots] on are left
 *     as they are.
 *   slot_rec_val [n_slots, n_rec]: the value of every receptor atom of every slot that has at least one ligand atom; a
 *     row of NaN for an empty slot and for one that is no slot (pvs_contact_attention's rule: the tables disagree, more
 *     than 1024 ligand atoms, rows beyond n_nodes - n_slots * n_rec ligand rows), which writes nothing to lig_val.
 *   rec_sum / rec_count / rec_max [n_rec]: READ AND UPDATED from slot_rec_val by pvs_contact_attention's accumulation
 *     kernel itself (slot order, NaN skipped, the same order relation).
 * Nothing read from the device decides an address unchecked; every output element has one writer, no atomics: the same
 * bits every time. n_slots == 0 or n_rec == 0: returns 0 without a launch. Two launches. */
int pvs_slot_node_values(const float* y, int32_t ld_y, int32_t col, int32_t n_mean, int32_t n_nodes,
                         const int32_t* node_ptr, const int32_t* lig_ptr, int32_t n_slots, int32_t n_rec,
                         float* lig_val, float* slot_rec_val, double* rec_sum, int32_t* rec_count, float* rec_max,
                         pvs_stream_t stream);

/* pvs_contact_attention and pvs_slot_node_values over the CROPPED pose-batch layout (PVS_SLOTS_CROPPED of
 * pvs_screen_slots_build / pvs_screen_copies_build): slot p owns the rows node_ptr[p] .. node_ptr[p + 1], its
 * lig_ptr[p + 1] - lig_ptr[p] ligand atoms first, then the receptor atoms whose bit is set in keep[p, :] (DEVICE,
 * [n_slots, ceil(n_rec / 64)] words; atom j is bit j % 64 of word j / 64), in receptor order, compact: receptor atom j
 * of slot p is row node_ptr[p] + n_lig_p + (the set bits of keep[p, :] below j). Outputs have the shapes and the
 * meaning of the uncropped entries:
 *   slot_rec_att / slot_rec_val [n_slots, n_rec]: for a KEPT atom the largest counted attention value of its row (NaN
 *     without a contact) / its node value (a slot without ligand atoms: NaN, the uncropped rule); NaN for an atom that
 *     is not kept - it is no atom of that slot's complex.
 *   lig_att / lig_val [>= lig_ptr[n_slots]]: as uncropped (in a cropped CSR a ligand atom's class-1 edges reach kept
 *     atoms only); the entries from lig_ptr[n_slots] on are left as they are. The caller provides lig_ptr[n_slots]
 *     entries: no argument says how many there are, so a slot's ligand range is checked against the rows, not against
 *     this array.
 *   rec_sum / rec_count / rec_max [n_rec]: READ AND UPDATED by pvs_contact_attention's accumulation kernel itself, so
 *     rec_count[j] grows by the slots that keep j and have a value for it.
 * A slot is one iff 0 <= lig_ptr[p] <= lig_ptr[p + 1], it has at most 1024 ligand atoms, 0 <= node_ptr[p],
 * node_ptr[p + 1] <= n_nodes, node_ptr[p + 1] - node_ptr[p] == its ligand atoms + the set bits of keep[p, :], and no
 * bit at or beyond n_rec is set (csrc/contact_attention.h: pvs_cropped_slot); any other gets a row of NaN and no
 * ligand write. A cropped batch may have fewer than n_slots * n_rec rows: that is not checked. NULL arguments, negative
 * counts, columns outside ld_y and an n_mean other than 1 or 3 are refused before any launch; n_slots == 0 or
 * n_rec == 0: returns 0 without a launch. One wavefront per (slot, mask word) counts the slot's words once and gives
 * every lane its atom's row; every output element has one writer, no atomics: the same bits every time, whatever the
 * launch geometry. Two launches each. */
int pvs_contact_attention_cropped(const int32_t* rowptr, const uint8_t* etype, const float* att, int32_t n_nodes,
                                  int32_t n_edges, const int32_t* node_ptr, const int32_t* lig_ptr,
                                  const uint64_t* keep, int32_t n_slots, int32_t n_rec, float* lig_att,
                                  float* slot_rec_att, double* rec_sum, int32_t* rec_count, float* rec_max,
                                  pvs_stream_t stream);
int pvs_slot_node_values_cropped(const float* y, int32_t ld_y, int32_t col, int32_t n_mean, int32_t n_nodes,
                                 const int32_t* node_ptr, const int32_t* lig_ptr, const uint64_t* keep, int32_t n_slots,
                                 int32_t n_rec, float* lig_val, float* slot_rec_val, double* rec_sum,
                                 int32_t* rec_count, float* rec_max, pvs_stream_t stream);

/* pvs_contact_attention's accumulation kernel by itself, over rows [n_hits, n_rec] that came from elsewhere (the
 * masking scores of ScreeningSweep.receptor_hotspots(attribution='atom_masking'), laid out as NaN-filled rows):
 * rec_sum / rec_count / rec_max [n_rec] are READ AND UPDATED with the values of every column that are not NaN, in hit
 * order, with the same order relation for the maximum. NULL arguments and negative counts are refused before the
 * launch; n_hits == 0 or n_rec == 0: returns 0 without a launch. One launch, no atomics: the same bits every time. */
int pvs_hit_rows_accumulate(const float* rows, int32_t n_hits, int32_t n_rec, double* rec_sum, int32_t* rec_count,
                            float* rec_max, pvs_stream_t stream);

/* Per-hit ranks (the reference's attribution/hotspot.py with use_rank, :183-191: an atom's value in a binding event is
 * replaced by its position in that event's descending sort). rows [n_hits, n_rec]: the value of every receptor atom
 * in every hit, NaN where it has none. lig_val, lig_ptr [n_hits + 1] (DEVICE) and lig_rank: all given or all NULL;
 * given, the packed ligand values lig_val[lig_ptr[h] .. lig_ptr[h + 1]) of hit h are candidates too (the reference
 * ranks over all atoms of the complex for cam and atom_masking, over protein atoms only for edge_attention). The
 * candidates of hit h are its ligand values that are not NaN (position = packed order), then its row values that are
 * not NaN (position = n_lig + j); u stands before v iff u > v, or u == v and u's position is lower (-0.0 == +0.0, the
 * infinities are ordinary values); rank(c) = the number of candidates of the same hit that stand before c: the
 * position in a descending STABLE sort, 0 = best (csrc/hit_ranks.h).
 *   row_rank [n_hits, n_rec]: the rank as a float, NaN where rows is NaN.
 *   lig_rank [>= lig_ptr[n_hits]]: the same, parallel to lig_val; the entries from lig_ptr[n_hits] on are left as they
 *     are. The caller provides lig_val and lig_rank with lig_ptr[n_hits] entries: no argument says how many there are.
 *   rank_sum / rank_count / rank_max [n_rec]: READ AND UPDATED from row_rank by pvs_contact_attention's accumulation
 *     kernel itself (pvs_hit_rows_accumulate), in hit order.
 * A hit whose ligand range descends, is negative or has more than 1024 atoms is no hit: a row of NaN, no ligand write,
 * nothing accumulated. n_rec + 1024 >= 2^24 (a rank would not be exact in fp32), NULL rows / row_rank / accumulators
 * and negative counts are refused before any launch; n_hits == 0 or n_rec == 0: returns 0 without a launch. A
 * workgroup per (hit, 256 candidates) counts over the hit's candidates, staged through LDS; every output element has
 * one writer, no atomics, no workspace: the same bits every time, whatever the launch geometry. Two launches. */
int pvs_hit_value_ranks(const float* rows, int32_t n_hits, int32_t n_rec, const float* lig_val, const int32_t* lig_ptr,
                        float* row_rank, float* lig_rank, double* rank_sum, int32_t* rank_count, float* rank_max,
                        pvs_stream_t stream);

/* nn.BCEWithLogitsLoss() with its default mean reduction (point_neural_network_base.py:74, used at :365) over n logits:
 * loss[0] = mean(max(x, 0) - x t + log1p(exp(-|x|))), grad[i] = (sigmoid(x_i) - t_i) / n (what the backward scales by
 * the upstream gradient: pvs_scale_by_device_scalar, out[i] = a[i] * scalar[0] with the scalar in device memory). */
int pvs_bce_logits_fwd(const float* x, const float* target, int32_t n, float* loss, float* grad,
                       pvs_stream_t stream);
int pvs_scale_by_device_scalar(const float* a, const float* scalar, int32_t n, float* out, pvs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * clip_grad_value_(params, clip) + torch.optim.Adam.step() (point_neural_network_base.py:421-422)
 * for all parameters in ONE launch. table: DEVICE array of n entries; the
 * gradients are clamped in place to [-clip, clip] (clip <= 0: no clamp), then
 *   g += weight_decay * p;  m += (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g^2;
 *   p -= (lr / bias_correction1) * m / (sqrt(v) / sqrt(bias_correction2) + eps)
 * (torch's non-amsgrad, non-maximize Adam, same operation order). bias_correction = 1 - beta^step
 * is passed by the host, which owns the step counter. */
typedef struct PvsAdamEntry {
    float* param;
    float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
} PvsAdamEntry;
int pvs_adam_clip_step(const PvsAdamEntry* table, int32_t n_tensors, double lr, double beta1, double beta2,
                       float eps, float weight_decay, double bias_correction1, double bias_correction2,
                       float clip, pvs_stream_t stream);
/* (lr, the betas and the bias corrections as DOUBLES since round 6: lr / bias_correction1, sqrt(bias_correction2), 1 - beta1
 * and 1 - beta2 are formed in double and rounded once, as torch forms the scalars it hands to lerp_ / addcmul_ / addcdiv_;
 * 1.f - 0.999f is 1.3e-5 below float(0.001).)
 * The same with the step count on the DEVICE: `step` points at one fp32 value, the number of this step (>= 1; the
 * caller advances it on the stream before the call), from which the kernel forms both bias corrections (in double, from the betas as doubles: `1 - beta ** step` as the host
 * form's caller evaluates it in Python: bit for bit the host form's update). This is what
 * torch.optim.Adam(capturable=True) does (adam.py `_multi_tensor_adam`, capturable branch: step tensors on the device) so
 * that a captured training step can be replayed; nothing about the launch depends on host state that changes per step. */
int pvs_adam_clip_step_dev(const PvsAdamEntry* table, int32_t n_tensors, double lr, double beta1, double beta2,
                           float eps, float weight_decay, const float* step, float clip, pvs_stream_t stream);

/* Hyper-parameters that change from step to step (a learning-rate scheduler; OneCycleLR also cycles Adam's beta1 / SGD's
 * momentum) live in a small block of doubles in DEVICE memory, so that a captured optimiser step can be replayed at other
 * values: Adam {lr, beta1, beta2}, SGD {lr, momentum}. pvs_hyper_write stores n (1..4) doubles into such a block on the
 * stream; the values travel BY VALUE as kernel arguments - no staging buffer, no host synchronisation, and a host that
 * runs several steps ahead of the device cannot overwrite what an earlier write still has to deliver. Call it outside
 * the capture and before every replay. */
int pvs_hyper_write(double* dst, int32_t n, double v0, double v1, double v2, double v3, pvs_stream_t stream);
/* pvs_adam_clip_step_dev with lr, beta1 and beta2 read from hyper[0..2]: lr / bias_correction1, sqrt(bias_correction2),
 * 1 - beta1 and 1 - beta2 are formed in double from those doubles and rounded once, as both forms above do: with the same
 * values in the block the update is bit for bit theirs. */
int pvs_adam_clip_step_hyper(const PvsAdamEntry* table, int32_t n_tensors, const double* hyper, float eps,
                             float weight_decay, const float* step, float clip, pvs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * clip_grad_value_(params, clip) + torch.optim.SGD.step() for all parameters in ONE launch, for the settings the
 * reference constructs (point_neural_network_base.py: momentum 0.9, nesterov, weight decay; dampening 0, not maximize).
 * The gradients are clamped in place to [-clip, clip] (clip <= 0: no clamp), then, every product rounded to fp32
 * before its sum,
 *   d = g + weight_decay * p;  buf = first ? d : momentum * buf + d;  d = nesterov ? d + momentum * buf : buf;
 *   p -= lr * d
 * `first`: the tensors of this table have no momentum history yet (torch clones the gradient into a new buffer): the
 * buffers are written, not read. momentum == 0 (or a NULL momentum_buf): no buffer is touched, d = g + weight_decay * p.
 * _hyper reads lr and momentum from hyper[0..1] (pvs_hyper_write) and has no `first`: a replayed step has buffers. */
typedef struct PvsSgdEntry {
    float* param;
    float* grad;
    float* momentum_buf;
    int64_t numel;
} PvsSgdEntry;
int pvs_sgd_clip_step(const PvsSgdEntry* table, int32_t n_tensors, double lr, double momentum, float weight_decay,
                      int32_t nesterov, int32_t first, float clip, pvs_stream_t stream);
int pvs_sgd_clip_step_hyper(const PvsSgdEntry* table, int32_t n_tensors, const double* hyper, float weight_decay,
                            int32_t nesterov, float clip, pvs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * unsorted_segment_sum / unsorted_segment_mean (egnn_satorras.py:332-337 / :340-347) as standalone
 * operators (inside the layers these sums are fused into the edge kernels).
 *   data [E,C] fp32, ids [E] int64 in [0,N) -> out [N,C]; mean != 0 divides by max(count, 1).
 *   ptr_out [N+1] int32 (caller-owned) receives the segment offsets, needed by the backward
 *   g_data[e,:] = g_out[ids[e],:] (/ max(count,1)). status: device int32, bit0 = id out of range
 *   (the reference's scatter_add_ raises there; the kernels stay in bounds - such a row is summed into
 *   segment 0 by the forward and reads segment 0's gradient in the backward - and the HOST must read the
 *   status word and raise: pointvs_amd/functional.py does, at the latest in the backward).
 */
size_t pvs_segment_workspace_bytes(int32_t n_rows, int32_t n_segments);
int pvs_segment_reduce_fwd(const float* data, const int64_t* ids, int32_t n_rows, int32_t width,
                           int32_t n_segments, int32_t mean, float* out, int32_t* ptr_out,
                           int32_t* status, void* workspace, size_t workspace_bytes,
                           pvs_stream_t stream);
int pvs_segment_reduce_bwd(const float* g_out, const int64_t* ids, const int32_t* ptr, int32_t n_rows,
                           int32_t width, int32_t n_segments, int32_t mean, float* g_data, pvs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * fp64 (the reference's --double, point_vs.py: torch.set_default_dtype(torch.float64)).
 * The same operations, layouts and conventions as the fp32 entries above, on double tensors; graphs
 * (PvsGraph, pvs_graph_prepare) have no dtype and are shared. Every result is summed in one fixed
 * order (no floating-point atomics): bitwise reproducible from run to run. The mean aggregation's
 * 1 / max(deg, 1) is formed in fp64 from rowptr (PvsGraph.inv_deg is not read).
 * Layer: H = 16, 32, 64 (callers pad other widths up to 64), 0..3 edge classes, every PVS_* flag;
 * n_edges_dev graphs are refused. saved: pvs_egnn_layer_saved_doubles_f64() doubles.
 */
typedef struct PvsLayerParamsF64 {
    const double *edge_w1, *edge_b1, *edge_w2, *edge_b2;
    const double *coord_w1, *coord_b1, *coord_w2;
    const double *att_w, *att_b;
    const double *node_w1, *node_b1, *node_w2, *node_b2;
    const double *gn_weight, *gn_bias, *gn_mean_scale;
    const double *node_att_w, *node_att_b;
    const double *edge_gate, *node_gate;
} PvsLayerParamsF64;

typedef struct PvsLayerGradsF64 {
    double *edge_w1, *edge_b1, *edge_w2, *edge_b2;
    double *coord_w1, *coord_b1, *coord_w2;
    double *att_w, *att_b;
    double *node_w1, *node_b1, *node_w2, *node_b2;
    double *gn_weight, *gn_bias, *gn_mean_scale;
    double *node_att_w, *node_att_b;
    double *edge_gate, *node_gate;
} PvsLayerGradsF64;

size_t pvs_egnn_layer_saved_doubles_f64(const PvsLayerDesc* desc, int32_t n_nodes, int32_t n_edges);
size_t pvs_egnn_layer_workspace_bytes_f64(const PvsLayerDesc* desc, int32_t n_nodes, int32_t n_edges,
                                          int32_t backward);
int pvs_egnn_layer_fwd_f64(const PvsLayerDesc* desc, const PvsGraph* graph, const PvsLayerParamsF64* params,
                           const double* h, const double* x, const double* m_prev,
                           double* h_out, double* x_out, double* m_out, double* att_out,
                           double* node_att_out, double* saved,
                           void* workspace, size_t workspace_bytes, pvs_stream_t stream);
int pvs_egnn_layer_bwd_f64(const PvsLayerDesc* desc, const PvsGraph* graph, const PvsLayerParamsF64* params,
                           const double* h, const double* x, const double* m_prev, const double* att,
                           const double* saved,
                           const double* g_h_out, const double* g_x_out, const double* g_m_out,
                           double* g_h, double* g_x, double* g_m_prev, const PvsLayerGradsF64* grads,
                           void* workspace, size_t workspace_bytes, pvs_stream_t stream);

/* The model-level ops in fp64 (row permutations are bit copies: pvs_rows_to_*_order at twice the width). */
int pvs_linear_fwd_f64(const double* x, const double* w, const double* b /*NULL if no bias*/, double* y,
                       int32_t n_rows, int32_t n_in, int32_t n_out, pvs_stream_t stream);
size_t pvs_linear_bwd_workspace_bytes_f64(int32_t n_rows, int32_t n_in, int32_t n_out);
int pvs_linear_bwd_f64(const double* x, const double* w, const double* g_y,
                       double* g_x /*NULL to skip*/, double* g_w, double* g_b /*NULL if no bias*/,
                       int32_t n_rows, int32_t n_in, int32_t n_out,
                       void* workspace, size_t workspace_bytes, pvs_stream_t stream);
int pvs_mean_pool_fwd_f64(const double* h, const int32_t* graph_ptr, double* pooled,
                          int32_t n_graphs, int32_t width, pvs_stream_t stream);
int pvs_mean_pool_bwd_f64(const double* g_pooled, const int32_t* graph_ptr, double* g_h,
                          int32_t n_graphs, int32_t n_nodes, int32_t width, pvs_stream_t stream);
size_t pvs_segment_workspace_bytes_f64(int32_t n_rows, int32_t n_segments);
int pvs_segment_reduce_fwd_f64(const double* data, const int64_t* ids, int32_t n_rows, int32_t width,
                               int32_t n_segments, int32_t mean, double* out, int32_t* ptr_out,
                               int32_t* status, void* workspace, size_t workspace_bytes,
                               pvs_stream_t stream);
int pvs_segment_reduce_bwd_f64(const double* g_out, const int64_t* ids, const int32_t* ptr, int32_t n_rows,
                               int32_t width, int32_t n_segments, int32_t mean, double* g_data,
                               pvs_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Measurement hook (no reference counterpart): when enabled, the library brackets its dominant
 * kernels ("edge_fwd", "edge_bwd", "col_gather", "graph_prepare", "edge_fwd_partial", "mask_graph") with HIP events on the launch
 * stream; pvs_profile_read waits for those events and returns the summed kernel time. Used by
 * bench.py for the roofline figure; off by default (no events are created).
 * on: 0 = off; 1 = all groups; otherwise a mask, bit (k + 1) = group k in the order above (an event pair costs the
 * stream a ~6 us bubble per launch, so bench.py brackets only the dominant kernel inside its timed region).
 * Behind those six, one group per dispatch route of the dense launchers, for tests that pin a shape to its route:
 * "linear_mfma", "linear_chunk64", "linear_chunk256", "linear_generic", "tsgemm_mfma", "tsgemm_wide",
 * "tsgemm_colchunk", "tsgemm_narrow", "tsgemm_tn8", "tsgemm_tn32", "colreduce4", "colreduce", "colreduce_chunk"
 * (groups 6 .. 18), and one group per node-level launcher of a layer, for tests that pin a layer to its node route (the
 * folded node MLP or the separate tail and output stage; the fused weight-gradient pass): "node_mlp_fwd", "node_mlp_bwd",
 * "node_out_fwd", "node_out_bwd", "node_tail" (the three tail launchers), "node_wgrads" (groups 19 .. 24).
 * Groups 6 .. 24 are recorded only when their own mask bit is set; on = 1 leaves them out.
 */
int pvs_profile_enable(int on);
int pvs_profile_reset(void);
int pvs_profile_read(const char* kernel, double* total_ms, int64_t* launches);
/* The same records one by one, in launch order: ms[0 .. min(*launches, cap)) = the duration of each recorded launch of
 * the group, *launches = how many were recorded (bench.py: the launches of one step do different amounts of work - the
 * last layer's backward has no coordinate branch - and the line states the full-work average beside the overall one). */
int pvs_profile_read_each(const char* kernel, double* ms, int64_t cap, int64_t* launches);
/* Which edge-backward pair the last pvs_egnn_layer_bwd of the process launched (a layer of pvs_egnn_stack_bwd counts as
 * one): -1 none yet, 0 the general pair, 1 the first-layer pair (g_x == NULL on a plain H = 32 layer with a coordinate
 * update; PVS_EGNN_FIRST_LAYER_BWD=0 turns it off). For tests that must know which of two bit-identical routes ran. */
int pvs_edge_bwd_last_variant(void);

#ifdef __cplusplus
}
#endif
#endif /* PVS_EGNN_H */
