// C ABI of one EGNNLayer forward / backward: sequences the kernels on the caller's stream.
// Reference: EGNNLayer.forward, /root/reference/point_vs/models/geometric/egnn_satorras.py:189-206.
#include "common.h"
#include "dense_ops.h"
#include "edge_kernels.h"
#include "layer_plan.h"
#include "node_ops.h"
#include "profile.h"

#include <stdlib.h>

namespace {

struct Dims {
    int N, E, H, A, ld1, off_rho, off_q;
    bool perm;
    bool segs;      // PVS_GRAPHNORM_SEGMENTS: GraphNorm per node segment (the table: PvsGraph.n_norm_rows_dev, n_graphs entries + 1)
};

Dims make_dims(const PvsLayerDesc* d, const PvsGraph* g) {
    Dims m;
    m.N = g->n_nodes; m.E = g->n_edges; m.H = d->hidden; m.A = d->n_edge_attr;
    m.perm = d->flags & PVS_PERM_INVARIANT;
    m.segs = d->flags & PVS_GRAPHNORM_SEGMENTS;
    m.off_rho = m.perm ? m.H : 2 * m.H;
    m.off_q = m.perm ? 0 : m.H;
    m.ld1 = m.off_rho + 1 + m.A;
    return m;
}

PvsEdgeW make_edge_w(const Dims& m, const PvsLayerParams* p) {
    PvsEdgeW w;
    w.w1 = p->edge_w1; w.ld1 = m.ld1; w.off_rho = m.off_rho;
    w.w2 = p->edge_w2; w.b2 = p->edge_b2;
    w.wc1 = p->coord_w1; w.bc1 = p->coord_b1; w.wc2 = p->coord_w2;
    w.wa = p->att_w; w.ba = p->att_b; w.edge_gate = p->edge_gate; w.n_attr = m.A;
    return w;
}

PvsNodeW make_node_w(const PvsLayerDesc* d, const PvsLayerParams* p) {
    PvsNodeW w;
    const bool gn = d->flags & PVS_GRAPHNORM, na = d->flags & PVS_NODE_ATTENTION;
    w.gn_w = gn ? p->gn_weight : nullptr;
    w.gn_b = gn ? p->gn_bias : nullptr;
    w.gn_ms = gn ? p->gn_mean_scale : nullptr;
    w.natt_w = na ? p->node_att_w : nullptr;
    w.natt_b = na ? p->node_att_b : nullptr;
    w.node_gate = p->node_gate;
    return w;
}

int check_desc(const PvsLayerDesc* d, const PvsGraph* g, const PvsLayerParams* p, bool allow_dev_count = false) {
    PVS_REQUIRE(d && g && p, "NULL descriptor/graph/params");
    if (d->flags & PVS_GRAPHNORM_SEGMENTS) {      // (forward entries pass allow_dev_count: the same set takes the flag)
        PVS_REQUIRE(allow_dev_count, "PVS_GRAPHNORM_SEGMENTS is forward-only: accepted by pvs_egnn_layer_fwd, pvs_egnn_stack_fwd "
                    "and pvs_egnn_layer_fwd_partial / _fwd_partial_att / _fwd_partial_softmax, refused by the backward");
        PVS_REQUIRE(d->flags & PVS_GRAPHNORM, "PVS_GRAPHNORM_SEGMENTS is valid only together with PVS_GRAPHNORM");
        PVS_REQUIRE(g->n_norm_rows_dev, "PVS_GRAPHNORM_SEGMENTS: PvsGraph.n_norm_rows_dev must point at the segment table "
                    "[n_graphs + 1] (it is NULL)");
        PVS_REQUIRE(g->n_graphs >= 1 && g->n_graphs <= g->n_nodes, "PVS_GRAPHNORM_SEGMENTS: PvsGraph.n_graphs = %d segments "
                    "(1..n_nodes = %d)", g->n_graphs, g->n_nodes);
    }
    // 16 / 32 / 64: every kernel family; 128 (the wide layer: 64 < hidden <= 128 zero-padded by the caller): the MFMA
    // edge kernels only (up to 3 edge classes, no PVS_EGNN_KERNELS=generic)
    PVS_REQUIRE(pvs_edge_v0_supported(d->hidden) ||
                    (d->hidden == 128 && pvs_edge_family(128, d->flags, d->n_edge_attr, PVS_EDGE_BWD) != PVS_EDGE_GENERIC),
                "hidden size %d unsupported by this build (16, 32, 64; 128 on the MFMA kernels with <= 3 edge classes)",
                d->hidden);
    PVS_REQUIRE(d->n_edge_attr >= 0 && d->n_edge_attr <= PVS_MAX_EDGE_ATTR,
                "n_edge_attr %d unsupported (0..%d)", d->n_edge_attr, PVS_MAX_EDGE_ATTR);
    PVS_REQUIRE(!((d->flags & PVS_GATED_RESIDUAL) && (d->flags & PVS_REZERO)),
                "gated_residual and rezero are incompatible");
    PVS_REQUIRE(g->n_nodes > 0 && g->n_edges >= 0, "bad graph sizes");
    PVS_REQUIRE(allow_dev_count || !g->n_edges_dev, "a graph with a device-side edge count is forward-only: accepted by "
                "pvs_egnn_layer_fwd (MFMA edge kernel, m_out = NULL) and by pvs_egnn_layer_edge_sums / _edge_stats_softmax / "
                "_fwd_partial / _fwd_partial_att / _fwd_partial_softmax");
    PVS_REQUIRE(d->n_edge_attr == 0 || g->etype, "graph has no edge types but layer expects %d",
                d->n_edge_attr);
    PVS_REQUIRE(p->edge_w1 && p->edge_b1 && p->edge_w2 && p->edge_b2 && p->node_w1 && p->node_b1 &&
                p->node_w2 && p->node_b2, "missing edge/node MLP parameters");
    if (d->flags & PVS_UPDATE_COORDS)
        PVS_REQUIRE(p->coord_w1 && p->coord_b1 && p->coord_w2, "missing coord MLP parameters");
    if (d->flags & PVS_EDGE_ATTENTION) PVS_REQUIRE(p->att_w && p->att_b, "missing att_mlp");
    if (d->flags & PVS_NODE_ATTENTION)
        PVS_REQUIRE(p->node_att_w && p->node_att_b, "missing node_att_mlp");
    if (d->flags & PVS_GRAPHNORM)
        PVS_REQUIRE(p->gn_weight && p->gn_bias && p->gn_mean_scale, "missing graphnorm parameters");
    if ((d->flags & PVS_RESIDUAL) && (d->flags & (PVS_REZERO | PVS_GATED_RESIDUAL)))
        PVS_REQUIRE(p->node_gate, "missing node_gate_parameter");
    return 0;
}

struct FwdWs {
    float *PQ, *y1, *u, *o, *smax, *ssum, *shift, *slabs, *m_scratch;
    float *seg_stats, *seg_slabs;      // PVS_GRAPHNORM_SEGMENTS only (else NULL): [S, 2H] and the segments' slabs, for S <= N
};

size_t carve_fwd(PvsArena& a, const Dims& m, FwdWs* w) {
    const size_t NH = (size_t)m.N * m.H;
    FwdWs t;
    t.PQ = a.take<float>(2 * NH);
    t.y1 = a.take<float>(NH);
    t.u = a.take<float>(NH);
    t.o = a.take<float>(NH);
    t.smax = a.take<float>(m.N);
    t.ssum = a.take<float>(m.N);
    t.shift = a.take<float>(m.H);
    t.slabs = a.take<float>((size_t)pvs_colreduce_blocks(m.N) * m.H);
    // H = 128: the edge forward is two launches that hand the messages over through memory
    t.m_scratch = a.take<float>(m.H > 64 ? (size_t)(m.E > 0 ? m.E : 1) * m.H : 4);
    t.seg_stats = m.segs ? a.take<float>(2 * NH) : nullptr;
    t.seg_slabs = m.segs ? a.take<float>(pvs_colmean_segments_slabs(m.N, m.N) * m.H) : nullptr;
    if (w) *w = t;
    return a.off;
}

// The first-layer reuse (the partial-layer entries below) in its two kinds: sums of the sigmoid / plain messages that add
// over two edge sets, or softmax statistics that merge (soft = true).
// Their workspace: the forward's, the edges' attention when the caller keeps none and, for softmax, the rows' factors.
struct PartialWs {
    FwdWs w;
    float *att, *fac;      // [max(E, 1)] | [N] (soft only)
};

void carve_partial(PvsArena& a, const Dims& m, bool soft, PartialWs* t) {
    carve_fwd(a, m, &t->w);
    t->att = a.take<float>((size_t)(m.E > 0 ? m.E : 1));
    t->fac = soft ? a.take<float>((size_t)m.N) : nullptr;
}

// Modes 2 and 3 of pvs_egnn_layer_workspace_bytes: never less than carve_partial needs, but not its dry run - the arena
// aligns in front of a take, these sizes round att and fac up behind them and add slack, and callers hold such buffers.
size_t partial_workspace_bytes(const Dims& m, bool soft) {
    PvsArena a(nullptr, 0);
    return carve_fwd(a, m, nullptr) + pvs_align_up((size_t)(m.E > 0 ? m.E : 1) * sizeof(float), 256) +
           (soft ? pvs_align_up((size_t)(m.N > 0 ? m.N : 1) * sizeof(float), 256) : 0) + 512;
}

// What a layer's forward keeps for its backward in the caller's `saved` buffer: the node-level forward (N rows: small)
// instead of recomputing it.
struct SavedLayout {
    float *Magg, *stats, *PQ, *y1, *o, *u;   // [N,H] | graphnorm stats [2H] | [N,2H] | [N,H] | [N,H] | SiLU(GN(y1)) [N,H]
    static size_t floats(size_t N, size_t H) { return 6 * N * H + 2 * H; }
};
SavedLayout saved_layout(float* saved, int N, int H) {
    const size_t NH = (size_t)N * H, S = 2 * (size_t)H;
    return {saved, saved + NH, saved + NH + S, saved + 3 * NH + S, saved + 4 * NH + S, saved + 5 * NH + S};
}

// The edge forward's tensors; m_prev / m_out / att_out as the entry point has them (NULL: none)
PvsEdgeFwdIO make_fwd_io(const FwdWs& w, const float* PQ, const float* x, const float* m_prev, float* Magg, float* x_out,
                         float* m_out, float* att_out) {
    PvsEdgeFwdIO io;
    io.PQ = PQ; io.x = x; io.m_prev = m_prev; io.Magg = Magg; io.x_out = x_out; io.m_out = m_out;
    io.att_out = att_out; io.smax = w.smax; io.ssum = w.ssum; io.m_scratch = w.m_scratch;
    return io;
}

struct BwdWs {
    float *PQ, *y1, *u, *o, *g_o, *g_u, *gM, *t1, *tg, *gl, *gxagg, *softD, *gPQ, *gz1, *gd, *gx_row;
    float *eslabs, *gsum, *dslabs, *S1, *S2, *coefs, *gvec, *nslabs, *nsum, *wslabs, *wpair;
};

size_t carve_bwd(PvsArena& a, const Dims& m, BwdWs* w) {
    const size_t NH = (size_t)m.N * m.H;
    const PvsSlabLayout L = pvs_slab_layout(m.H);
    BwdWs t;
    t.PQ = a.take<float>(2 * NH);
    t.y1 = a.take<float>(NH);
    t.u = a.take<float>(NH);
    t.o = a.take<float>(NH);
    t.g_o = a.take<float>(NH);
    t.g_u = a.take<float>(NH);
    t.gM = a.take<float>(NH);
    t.t1 = a.take<float>(NH);
    t.tg = a.take<float>(NH);
    t.gl = a.take<float>(m.N);
    t.gxagg = a.take<float>(3 * (size_t)m.N);
    t.softD = a.take<float>(m.N);
    t.gPQ = a.take<float>(2 * NH);
    t.gz1 = a.take<float>((size_t)(m.E > 0 ? m.E : 1) * m.H);
    t.gd = a.take<float>(4 * (size_t)(m.E > 0 ? m.E : 1));
    t.gx_row = a.take<float>(3 * (size_t)m.N);
    t.eslabs = a.take<float>((size_t)kPvsEdgeSlabCapacity * L.total);      // one slab per workgroup of the edge backward
    t.gsum = a.take<float>(L.total);
    t.dslabs = a.take<float>((size_t)pvs_reduce_blocks(m.N) * m.H * m.H);
    t.S1 = a.take<float>(m.H);
    t.S2 = a.take<float>(m.H);
    t.coefs = a.take<float>(4 * (size_t)m.H);
    t.gvec = a.take<float>(m.H);
    t.nslabs = a.take<float>((size_t)2048 * 4 * m.H);      // one [4H] slab per workgroup of the column gather
    t.nsum = a.take<float>(4 * (size_t)m.H);
    t.wslabs = a.take<float>(pvs_node_wgrads_supported(m.H) ? pvs_node_wgrads_slab_floats(m.N, m.H) : 4);
    // H = 128: coord_mlp.0's weight staged per launch for the team backward (split A operands, or the fp32 pair)
    t.wpair = a.take<float>(m.H > 64 ? pvs_edge_bwd_wide_scratch_floats() + 2 * (size_t)m.H * m.H : 4);
    if (w) *w = t;
    return a.off;
}

// scatter the reduced edge-kernel slab into the parameter gradients
// The first `node_blocks` workgroups (if any) reduce the node-level weight-gradient slabs, 32 entries each, straight
// into the gradient tensors (no reduced copy in between, no launch of its own); the others scatter the edge sums.
__global__ void __launch_bounds__(256)
k_finalize_edge_grads(const float* __restrict__ gsum, PvsSlabLayout L, int H, int A,
                      int ld1, int off_rho, PvsLayerGrads gr, int has_coord,
                      int has_att, int has_gate, const float* __restrict__ node_gsum,
                      PvsNodeWgradOut node_out, PvsNodeWgradSlabs node_slabs, int node_blocks) {
    if ((int)blockIdx.x < node_blocks) {
        __shared__ float part[8][33];
        pvs_node_wgrads_reduce_scatter32(node_slabs, node_out, H, 32 * (int)blockIdx.x, part);
        return;
    }
    const int tid = ((int)blockIdx.x - node_blocks) * blockDim.x + threadIdx.x;
    const int stride = ((int)gridDim.x - node_blocks) * blockDim.x;
    // (the node-level weight gradients' reduced sums, when they were left for this kernel to scatter)
    if (node_gsum) pvs_node_wgrads_scatter(node_gsum, node_out, H, tid, stride);
    for (int i = tid; i < H * H; i += stride) {
        if (gr.edge_w2) gr.edge_w2[i] = gsum[L.w2 + i];
        if (has_coord && gr.coord_w1) gr.coord_w1[i] = gsum[L.wc1 + i];
    }
    for (int c = tid; c < H; c += stride) {
        if (gr.edge_b2) gr.edge_b2[c] = gsum[L.b2 + c];
        if (has_coord && gr.coord_b1) gr.coord_b1[c] = gsum[L.bc1 + c];
        if (has_coord && gr.coord_w2) gr.coord_w2[c] = gsum[L.wc2 + c];
        if (has_att && gr.att_w) gr.att_w[c] = gsum[L.wa + c];
        if (gr.edge_w1) {
            gr.edge_w1[(size_t)c * ld1 + off_rho] = gsum[L.wrho + c];
            for (int t = 0; t < A; ++t)
                gr.edge_w1[(size_t)c * ld1 + off_rho + 1 + t] = gsum[L.wattr + t * H + c];
        }
    }
    if (tid == 0) {
        // (softmax attention, has_att == 2: a softmax does not see a shift of its logits, so the gradient of the logit
        // bias is zero IDENTICALLY; the sum of the per-edge logit gradients only leaves its rounding residue there)
        if (has_att && gr.att_b) gr.att_b[0] = has_att == 2 ? 0.f : gsum[L.ba];
        if (has_gate && gr.edge_gate) gr.edge_gate[0] = gsum[L.gate];
    }
}

// The MFMA edge backward of the family `fam` (the launchers' contract: edge_kernels.h)
int pvs_launch_edge_bwd_mfma(hipStream_t s, int H, PvsEdgeFamily fam, const PvsGraph& g, const PvsEdgeW& w, uint32_t flags,
                             int att_act, const PvsEdgeBwdIO& io, int e_lo, int e_hi, int* n_slabs) {
    switch (fam) {
        case PVS_EDGE_SPLIT:
            if (H == 32) return pvs_launch_edge_bwd_f16(s, H, g, w, flags, att_act, io, e_lo, e_hi, n_slabs);
            PVS_REQUIRE(H == 64, "split-product edge backward is built for H = 32, 64 (got %d)", H);
            return pvs_launch_edge_bwd_h64(s, g, w, flags, att_act, io, e_lo, e_hi, n_slabs);
        case PVS_EDGE_EXACT: return pvs_launch_edge_bwd_exact(s, H, g, w, flags, att_act, io, e_lo, e_hi, n_slabs);
        case PVS_EDGE_WIDE: return pvs_launch_edge_bwd_wide(s, H, g, w, flags, att_act, io, e_lo, e_hi, n_slabs);
        default: break;      // (generic: pvs_launch_edge_bwd_v0, another contract)
    }
    pvs_set_error("pvs_launch_edge_bwd_mfma: family %d is not an MFMA family", (int)fam);
    return -1;
}

// y1 = [h | Magg] Wn1^T + bn1 ; (graphnorm stats) ; u = SiLU(GN(y1)) ; o = u Wn2^T + bn2 ; h_out
// = node_out(o, h). Without GraphNorm the SiLU rides on the first product's epilogue, and the plain
// (un-gated, no node attention) output stage on the second's: two launches instead of four.
// n_norm_rows_dev (PvsGraph.n_norm_rows_dev, read under GraphNorm only): the statistics run over that many leading rows.
// n_segs > 0 (PVS_GRAPHNORM_SEGMENTS): n_norm_rows_dev is the segment table [n_segs + 1] instead, every segment's pair goes
// to seg_stats [n_segs, 2H] (slabs: seg_slabs), each row is normalised with its own; `stats` is not written.
int node_mlp_forward(hipStream_t s, const Dims& m, const PvsLayerDesc* d, const PvsLayerParams* p,
                     const PvsNodeW& nw, const float* h, const float* Magg, float* y1, float* u,
                     float* o, float* stats, bool compute_stats, float* shift_tmp, float* slabs,
                     float* h_out, float* node_att_out, const int32_t* n_norm_rows_dev, int n_segs = 0,
                     float* seg_stats = nullptr, float* seg_slabs = nullptr) {
    const int H = m.H;
    const uint32_t F = d->flags;
    PvsLinearJob first = pvs_linear_job(y1, H, pvs_operand(h, H, p->node_w1, 2 * H, H), m.N, H, p->node_b1);
    first.b = pvs_operand(Magg, H, p->node_w1 + H, 2 * H, H);
    first.aux_out = u; first.ld_out = H;
    PvsLinearJob second = pvs_linear_job(o, H, pvs_operand(u, H, p->node_w2, H, H), m.N, H, p->node_b2);
    second.aux_in = h; second.ld_in = H; second.aux_out = h_out; second.ld_out = H;
    const bool can_epi = pvs_linear_epilogue_supported(first) && pvs_linear_epilogue_supported(second) &&
                         (((uintptr_t)h_out | (uintptr_t)u) & 15) == 0;
    const bool fuse_silu = can_epi && !(F & PVS_GRAPHNORM);
    const bool gated = (F & PVS_RESIDUAL) && (F & (PVS_REZERO | PVS_GATED_RESIDUAL));
    const bool fuse_out = can_epi && !(F & PVS_NODE_ATTENTION) && !gated;
    // (read at every call: layer_plan.h)
    const bool split_small = pvs_layer_switches().split_small;     // (the launches apart, for A/B)
    if (fuse_silu && !gated && !split_small && p->node_b1 && p->node_b2 &&
        pvs_node_mlp_fused_supported(H, h, Magg, y1, h_out)) {
        // no GraphNorm, no rezero / gated residual: the whole chain y1 -> u -> o -> (node gate) -> h_out in one launch
        // (dense_ops.hip: k_node_mlp_fwd)
        const bool natt = F & PVS_NODE_ATTENTION;
        return pvs_launch_node_mlp_fwd(s, H, m.N, h, Magg, p->node_w1, p->node_b1, p->node_w2, p->node_b2,
                                       (F & PVS_RESIDUAL) != 0, natt ? nw.natt_w : nullptr, natt ? nw.natt_b : nullptr,
                                       d->att_act, y1, u, o, h_out, node_att_out);
    }
    first.epi = fuse_silu ? PVS_EPI_SILU_OUT : PVS_EPI_NONE;
    PVS_TRY(pvs_launch_linear(s, first));
    if (n_segs > 0) {
        PVS_TRY(pvs_graphnorm_stats_segments_launch(s, y1, p->gn_mean_scale, m.N, H, n_norm_rows_dev, n_segs, seg_stats,
                                                    seg_slabs));
        PVS_TRY(pvs_node_tail_fwd_segments(s, y1, seg_stats, n_norm_rows_dev, n_segs, nw, m.N, H, u));
    } else {
        if ((F & PVS_GRAPHNORM) && compute_stats)
            PVS_TRY(pvs_graphnorm_stats(s, y1, p->gn_mean_scale, m.N, H, stats, shift_tmp, slabs, n_norm_rows_dev));
        if (!fuse_silu) PVS_TRY(pvs_node_tail_fwd(s, y1, stats, nw, m.N, H, u));
    }
    second.epi = !fuse_out ? PVS_EPI_NONE : (F & PVS_RESIDUAL) ? PVS_EPI_ADD_OUT : PVS_EPI_COPY_OUT;
    PVS_TRY(pvs_launch_linear(s, second));
    if (!fuse_out) PVS_TRY(pvs_node_out_fwd(s, H, o, h, nw, F, d->att_act, m.N, h_out, node_att_out));
    return 0;
}

// P and Q of a layer as ONE launch where the MFMA linear takes the shape (H = 32, 64): two groups of workgroups, one per
// 32- or 64-column half of the output, the second on the Q slice of edge_mlp.0's weight.
// `init` (MFMA edge forward only): the edge kernel never flushes rows without edges, so Magg = 0 and x_out = x (0 for
// raw sums) are written first - by a third group of workgroups of that launch, else by the edge launcher's own small
// kernel (io->init_done stays false).
int node_pre_forward(hipStream_t s, const Dims& m, const PvsLayerParams* p, const float* h,
                     float* PQ, PvsEdgeFwdIO* init = nullptr, uint32_t init_flags = 0) {
    const int H = m.H;
    const bool split_small = pvs_layer_switches().split_small;     // (the launches apart, for A/B)
    PvsLinearExt e;
    if (init) {
        e.zero_rows = init->Magg; e.zero_w = H; e.zero_ld = H;
        if (init_flags & kFwdRawXsum) e.zero3 = init->x_out;
        else if (init_flags & PVS_UPDATE_COORDS) { e.copy3_src = init->x; e.copy3_dst = init->x_out; }
    }
    const bool side_ok = init && !split_small && ((uintptr_t)init->Magg & 15) == 0;
    // P = h W1[:, 0:H]^T + b1 (row part), Q = h W1[:, off_q:off_q+H]^T (col part)
    const PvsLinearOperand row_part = pvs_operand(h, H, p->edge_w1, m.ld1, H);
    if ((H == 32 || H == 64) && !split_small && (H == 64 || !init || side_ok)) {
        // P | Q as two groups of workgroups of ONE launch (H outputs each; the second group on the Q slice of the weight, no
        // bias), the forward's clears as a third group: at H = 32, 12 us against 15-16 for workgroups twice as long that
        // also do the clears; at H = 64, as side jobs of the P workgroups they cost 11 us against 6 for a launch of their
        // own (profiles/r03_ab_small_launch_folding.txt). H = 32 with clears that cannot ride takes the two launches below.
        PvsLinearExt g2 = side_ok ? e : PvsLinearExt{};
        g2.groups = 2; g2.shift_block = H / 32; g2.bias_blocks = H / 32; g2.side_group = side_ok ? 1 : 0;
        g2.w_shift1 = (long long)m.off_q - (long long)H * m.ld1;
        PvsLinearJob pq = pvs_linear_job(PQ, 2 * H, row_part, m.N, 2 * H, p->edge_b1);
        pq.ext = &g2;
        if (pvs_linear_epilogue_supported(pq)) {
            PVS_TRY(pvs_launch_linear(s, pq));
            if (side_ok) init->init_done = true;
            return 0;
        }
    }
    PVS_TRY(pvs_launch_linear(s, pvs_linear_job(PQ, 2 * H, row_part, m.N, H, p->edge_b1)));
    PVS_TRY(pvs_launch_linear(s, pvs_linear_job(PQ + H, 2 * H, pvs_operand(h, H, p->edge_w1 + m.off_q, m.ld1, H), m.N, H)));
    return 0;
}

}  // namespace

extern "C" size_t pvs_egnn_layer_saved_floats(const PvsLayerDesc* d, int32_t N, int32_t E) {
    (void)E;
    return SavedLayout::floats((size_t)N, (size_t)d->hidden);
}

extern "C" size_t pvs_egnn_layer_workspace_bytes(const PvsLayerDesc* d, int32_t N, int32_t E,
                                                 int32_t backward) {
    PvsGraph g{};
    g.n_nodes = N; g.n_edges = E;
    Dims m = make_dims(d, &g);
    // 2: pvs_egnn_layer_edge_sums / _fwd_partial / _fwd_partial_att; 3: _edge_stats_softmax / _fwd_partial_softmax
    if (backward == 2 || backward == 3) return partial_workspace_bytes(m, backward == 3);
    PvsArena a(nullptr, 0);
    return (backward ? carve_bwd(a, m, nullptr) : carve_fwd(a, m, nullptr)) + 256;
}

extern "C" int pvs_egnn_layer_fwd(const PvsLayerDesc* d, const PvsGraph* g, const PvsLayerParams* p,
                                  const float* h, const float* x, const float* m_prev, float* h_out,
                                  float* x_out, float* m_out, float* att_out, float* node_att_out,
                                  float* saved, void* workspace, size_t workspace_bytes,
                                  pvs_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    PVS_TRY(check_desc(d, g, p, /*allow_dev_count=*/true));
    const PvsEdgeFamily fam = pvs_edge_family(d->hidden, d->flags, d->n_edge_attr, PVS_EDGE_FWD);
    const bool mfma_fwd = fam != PVS_EDGE_GENERIC;
    PVS_REQUIRE(!g->n_edges_dev || (mfma_fwd && !m_out),
                "pvs_egnn_layer_fwd: a graph with a device-side edge count needs the MFMA edge kernel and m_out = NULL");
    PVS_REQUIRE(h && x && h_out && x_out && saved, "pvs_egnn_layer_fwd: NULL tensor");
    PVS_REQUIRE(x_out != x, "pvs_egnn_layer_fwd: x_out must not alias x");
    const bool eatt = d->flags & PVS_EDGE_ATTENTION;
    PVS_REQUIRE(!eatt || att_out, "pvs_egnn_layer_fwd: att_out required with edge attention");
    const Dims m = make_dims(d, g);
    PvsArena arena(workspace, workspace_bytes);
    FwdWs w;
    carve_fwd(arena, m, &w);
    PVS_REQUIRE(arena.ok(), "pvs_egnn_layer_fwd: workspace too small (%zu < %zu)", workspace_bytes,
                arena.off);
    const int H = m.H;
    const SavedLayout sv = saved_layout(saved, m.N, H);
    const PvsEdgeW ew = make_edge_w(m, p);
    const PvsNodeW nw = make_node_w(d, p);

    PvsEdgeFwdIO io = make_fwd_io(w, sv.PQ, x, m_prev, sv.Magg, x_out, m_out, att_out);
    PVS_TRY(node_pre_forward(s, m, p, h, sv.PQ, mfma_fwd ? &io : nullptr, d->flags));
    if (mfma_fwd)
        PVS_TRY(pvs_launch_edge_fwd_mfma(s, H, fam, *g, ew, d->flags, d->att_act, io));
    else
        PVS_TRY(pvs_launch_edge_fwd_v0(s, H, *g, ew, d->flags, d->att_act, io));
    if (!(d->flags & PVS_UPDATE_COORDS))
        PVS_CHECK_HIP(hipMemcpyAsync(x_out, x, sizeof(float) * 3 * (size_t)m.N,
                                     hipMemcpyDeviceToDevice, s));
    PVS_TRY(node_mlp_forward(s, m, d, p, nw, h, sv.Magg, sv.y1, sv.u, sv.o, sv.stats, true, w.shift, w.slabs, h_out,
                             node_att_out, g->n_norm_rows_dev, m.segs ? g->n_graphs : 0, w.seg_stats, w.seg_slabs));
    return 0;
}

// ---- forward with part of every row's edges given as precomputed sums (screening: the
// receptor-receptor messages of the first layer do not depend on the ligand pose) ----
// Two kinds (soft = false / true), one host path. Sums: the rows' sums of two edge sets add; for sigmoid attention or none.
// Softmax attention: row sums of two edge sets do not add, but the softmax statistics merge exactly. For a
// row i and an edge set T with logits l_e: mu_T = max l_e, S_T = sum exp(l_e - mu_T), A_T = sum exp(l_e - mu_T) m_e / S_T -
// what the softmax MFMA forward leaves in smax / ssum / Magg at every row it flushes. A BASE ROW is H + 4 floats:
// A_b [H] | mu_b | S_b | 0 | 0; all zero: no base (S_b >= 1 for a set with an edge).
namespace {

constexpr int kBaseRowExtra = 4;      // mu, S and two zeros behind the H channels: rows stay 16-byte multiples

// Row n's coordinates, by the row's first thread of both combine kernels: x_out holds the raw sums over the graph's deg_g
// edges of the row and becomes x + (base_xsum + x_out) / max(base_deg + deg_g, 1), or x where coordinates stay
__device__ __forceinline__ void combine_partial_coords(float* __restrict__ x_out, const float* __restrict__ x,
                                                       const float* __restrict__ base_xsum,
                                                       const float* __restrict__ base_deg, int deg_g, int n, int upd) {
    if (upd) {
        const float deg = base_deg[n] + (float)deg_g;
        const float inv = 1.0f / (deg > 1.f ? deg : 1.f);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            x_out[3 * n + c] = x[3 * n + c] + (base_xsum[3 * n + c] + x_out[3 * n + c]) * inv;
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) x_out[3 * n + c] = x[3 * n + c];
    }
}

__global__ void k_combine_partial(float* __restrict__ Magg, float* __restrict__ x_out, const float* __restrict__ x,
                                  const float* __restrict__ base_magg, const float* __restrict__ base_xsum,
                                  const float* __restrict__ base_deg, const int32_t* __restrict__ rowptr,
                                  int N, int H, int upd) {
    const int qpr = H / 4;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = t / qpr, q = t - n * qpr;
    if (n >= N) return;
    float4* mp = reinterpret_cast<float4*>(Magg + (size_t)n * H + 4 * q);
    const float4 b = *reinterpret_cast<const float4*>(base_magg + (size_t)n * H + 4 * q);
    float4 m = *mp;
    m.x += b.x; m.y += b.y; m.z += b.z; m.w += b.w;
    *mp = m;
    if (q == 0) combine_partial_coords(x_out, x, base_xsum, base_deg, rowptr[n + 1] - rowptr[n], n, upd);
}

// Magg / smax / ssum of the base launch -> base rows; rows without an edge (never flushed: their statistics are whatever
// the workspace held) are decided from the degree and written as zeros
__global__ void k_pack_base_rows(const float* __restrict__ Magg, const float* __restrict__ smax,
                                 const float* __restrict__ ssum, const int32_t* __restrict__ rowptr,
                                 float* __restrict__ base_rows, int N, int H) {
    const int qpr = H / 4 + 1;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = t / qpr, q = t - n * qpr;
    if (n >= N) return;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (rowptr[n + 1] > rowptr[n]) {
        if (q < H / 4) v = *reinterpret_cast<const float4*>(Magg + (size_t)n * H + 4 * q);
        else { v.x = smax[n]; v.y = ssum[n]; }
    }
    *reinterpret_cast<float4*>(base_rows + (size_t)n * (H + kBaseRowExtra) + 4 * q) = v;
}

// One thread per row and channel quad, like k_combine_partial: Magg (A_g, normalised over the graph's edges of the row)
// becomes the mean over both sets, the coordinate update is k_combine_partial's, and the row's attention factor
// a_g / (a_b + a_g) goes to fac. The larger maximum's weight is its S itself, the other's carries the one expf.
__global__ void k_combine_partial_softmax(float* __restrict__ Magg, float* __restrict__ x_out, const float* __restrict__ x,
                                          const float* __restrict__ base_rows, const float* __restrict__ base_xsum,
                                          const float* __restrict__ base_deg, const int32_t* __restrict__ rowptr,
                                          const float* __restrict__ smax, const float* __restrict__ ssum,
                                          float* __restrict__ fac, int N, int H, int upd) {
    const int qpr = H / 4;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = t / qpr, q = t - n * qpr;
    if (n >= N) return;
    const float* brow = base_rows + (size_t)n * (H + kBaseRowExtra);
    const float4 stat = *reinterpret_cast<const float4*>(brow + H);      // mu_b, S_b, 0, 0
    const int deg_g = rowptr[n + 1] - rowptr[n];
    const bool has_b = stat.y > 0.f, has_g = deg_g > 0;
    float wb = has_b ? 1.f : 0.f, wg = has_g ? 1.f : 0.f;
    if (has_b && has_g) {
        const float mu_g = smax[n], S_g = ssum[n], d = stat.x - mu_g;
        const float f = expf(-fabsf(d));
        const float a_b = d >= 0.f ? stat.y : stat.y * f, a_g = d >= 0.f ? S_g * f : S_g;
        const float inv = 1.0f / (a_b + a_g);
        wb = a_b * inv;
        wg = a_g * inv;
    }
    float4* mp = reinterpret_cast<float4*>(Magg + (size_t)n * H + 4 * q);
    float4 m = make_float4(0.f, 0.f, 0.f, 0.f);
    if (has_g) {
        const float4 a = *mp;
        m.x = wg * a.x; m.y = wg * a.y; m.z = wg * a.z; m.w = wg * a.w;
    }
    if (has_b) {
        const float4 b = *reinterpret_cast<const float4*>(brow + 4 * q);
        m.x = fmaf(wb, b.x, m.x); m.y = fmaf(wb, b.y, m.y); m.z = fmaf(wb, b.z, m.z); m.w = fmaf(wb, b.w, m.w);
    }
    *mp = m;
    if (q == 0) {
        fac[n] = wg;
        combine_partial_coords(x_out, x, base_xsum, base_deg, deg_g, n, upd);
    }
}

// att[e] (normalised over the graph's edges of its row) -> normalised over both sets; entries behind a device-side count
// stay as they are
__global__ void k_scale_att_rows(PvsGraph g, const float* __restrict__ fac, float* __restrict__ att) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= g.n_edges || (g.n_edges_dev && e >= *g.n_edges_dev)) return;
    att[e] *= fac[g.row[e]];
}

struct PartialCall {      // what an accepted call works with
    Dims m;
    PvsEdgeFamily fam;
    PartialWs ws;
};

// Every refusal of the five entries, in the order they have always come and all before the first HIP call: the layer and
// its kind, then the entry's own arguments (tensors: none of them NULL; x_out: NULL for an entry without one; base_rows:
// looked at for soft only), then the workspace. `entry`: the name the messages carry.
int partial_checks(bool soft, const char* entry, const PvsLayerDesc* d, const PvsGraph* g, const PvsLayerParams* p,
                   bool tensors, const float* x, const float* x_out, const float* base_rows, void* workspace,
                   size_t workspace_bytes, PartialCall* c) {
    const char* what = soft ? "softmax partial forward" : "partial-sum forward";
    PVS_TRY(check_desc(d, g, p, true));
    c->fam = pvs_edge_family(d->hidden, d->flags, d->n_edge_attr, PVS_EDGE_FWD);
    PVS_REQUIRE(c->fam != PVS_EDGE_GENERIC, "%s needs the MFMA edge kernel (H = 32, 64 or 128)", what);
    const bool soft_layer = (d->flags & PVS_EDGE_ATTENTION) && (d->flags & PVS_SOFTMAX_ATT);
    PVS_REQUIRE(soft == soft_layer, "%s: %s", what,
                soft ? "for layers with edge attention and softmax attention only (the others: pvs_egnn_layer_edge_sums / "
                       "pvs_egnn_layer_fwd_partial)"
                     : "softmax attention is not supported (row sums of two edge sets do not add)");
    PVS_REQUIRE(!(d->flags & PVS_EDGE_RESIDUAL), "%s: edge_residual layers are not supported", what);
    PVS_REQUIRE(tensors, "%s: NULL tensor", entry);
    PVS_REQUIRE(x_out != x, "%s: x_out must not alias x", entry);
    PVS_REQUIRE(!soft || ((uintptr_t)base_rows & 15) == 0, "%s: base_rows must be 16-byte aligned", entry);
    c->m = make_dims(d, g);
    PvsArena arena(workspace, workspace_bytes);
    carve_partial(arena, c->m, soft, &c->ws);
    PVS_REQUIRE(arena.ok(), "%s: workspace too small (%zu < %zu)", entry, workspace_bytes, arena.off);
    return 0;
}

// P | Q into PQ with the clears, then the MFMA edge forward over g with the raw coordinate sums in x_out, timed as `tag`
int partial_edge_forward(hipStream_t s, const PartialCall& c, const PvsLayerDesc* d, const PvsGraph* g,
                         const PvsLayerParams* p, const float* h, const float* x, float* PQ, float* Magg, float* x_out,
                         float* att, int tag) {
    const PvsEdgeW ew = make_edge_w(c.m, p);
    PvsEdgeFwdIO io = make_fwd_io(c.ws.w, PQ, x, nullptr, Magg, x_out, nullptr, att);
    PVS_TRY(node_pre_forward(s, c.m, p, h, PQ, &io, d->flags | kFwdRawXsum));
    pvs_prof_set_fwd_tag(tag);
    const int rc = pvs_launch_edge_fwd_mfma(s, c.m.H, c.fam, *g, ew, d->flags | kFwdRawXsum, d->att_act, io);
    pvs_prof_set_fwd_tag(PVS_PROF_EDGE_FWD);      // (back first: a failing launch's code goes out after it)
    return rc;
}

// The base of a set of edges, once per receptor. out: magg [N, H], or base rows [N, H + 4] for soft.
int partial_base(bool soft, const char* entry, const PvsLayerDesc* d, const PvsGraph* g, const PvsLayerParams* p,
                 const float* h, const float* x, float* out, float* xsum, void* workspace, size_t workspace_bytes,
                 hipStream_t s) {
    PartialCall c;
    PVS_TRY(partial_checks(soft, entry, d, g, p, h && x && out && xsum, x, nullptr, out, workspace, workspace_bytes, &c));
    const FwdWs& w = c.ws.w;
    float* Magg = soft ? w.y1 : out;      // (A_b: [N, H] of the forward's workspace that a base has no other use for)
    PVS_TRY(partial_edge_forward(s, c, d, g, p, h, x, w.PQ, Magg, xsum, c.ws.att, PVS_PROF_EDGE_FWD));
    if (!(d->flags & PVS_UPDATE_COORDS))
        PVS_CHECK_HIP(hipMemsetAsync(xsum, 0, sizeof(float) * 3 * (size_t)c.m.N, s));
    if (soft) {
        const long long threads = (long long)c.m.N * (c.m.H / 4 + 1);
        k_pack_base_rows<<<(int)((threads + 255) / 256), 256, 0, s>>>(Magg, w.smax, w.ssum, g->rowptr, out, c.m.N, c.m.H);
        PVS_CHECK_LAUNCH();
    }
    return 0;
}

// EGNNLayer.forward over the edges of g on top of a base (base: base_magg, or base rows for soft), per batch. att_out: the
// caller keeps the layer's attention (CSR-sorted over g), NULL: it stays in the workspace (carved either way: one size)
int partial_forward(bool soft, const char* entry, const PvsLayerDesc* d, const PvsGraph* g, const PvsLayerParams* p,
                    const float* h, const float* x, const float* base, const float* base_xsum, const float* base_deg,
                    float* h_out, float* x_out, float* node_att_out, float* att_out, float* saved, void* workspace,
                    size_t workspace_bytes, hipStream_t s) {
    PartialCall c;
    PVS_TRY(partial_checks(soft, entry, d, g, p, h && x && base && base_xsum && base_deg && h_out && x_out && saved, x,
                           x_out, base, workspace, workspace_bytes, &c));
    const Dims& m = c.m;
    const FwdWs& w = c.ws.w;
    const int H = m.H, upd = (d->flags & PVS_UPDATE_COORDS) ? 1 : 0;
    const SavedLayout sv = saved_layout(saved, m.N, H);
    // (the launch is timed apart from the full-graph layers: bench.py)
    PVS_TRY(partial_edge_forward(s, c, d, g, p, h, x, sv.PQ, sv.Magg, x_out, att_out ? att_out : c.ws.att,
                                 PVS_PROF_EDGE_FWD_PARTIAL));
    const long long threads = (long long)m.N * (H / 4);
    const int blocks = (int)((threads + 255) / 256);
    if (soft)
        k_combine_partial_softmax<<<blocks, 256, 0, s>>>(sv.Magg, x_out, x, base, base_xsum, base_deg, g->rowptr, w.smax,
                                                         w.ssum, c.ws.fac, m.N, H, upd);
    else
        k_combine_partial<<<blocks, 256, 0, s>>>(sv.Magg, x_out, x, base, base_xsum, base_deg, g->rowptr, m.N, H, upd);
    PVS_CHECK_LAUNCH();
    if (soft && att_out && g->n_edges > 0) {
        k_scale_att_rows<<<(g->n_edges + 255) / 256, 256, 0, s>>>(*g, c.ws.fac, att_out);
        PVS_CHECK_LAUNCH();
    }
    return node_mlp_forward(s, m, d, p, make_node_w(d, p), h, sv.Magg, sv.y1, sv.u, sv.o, sv.stats, true, w.shift, w.slabs,
                            h_out, node_att_out, g->n_norm_rows_dev, m.segs ? g->n_graphs : 0, w.seg_stats, w.seg_slabs);
}

}  // namespace

extern "C" int pvs_egnn_layer_edge_sums(const PvsLayerDesc* d, const PvsGraph* g, const PvsLayerParams* p,
                                        const float* h, const float* x, float* magg, float* xsum,
                                        void* workspace, size_t workspace_bytes, pvs_stream_t stream_) {
    return partial_base(false, "pvs_egnn_layer_edge_sums", d, g, p, h, x, magg, xsum, workspace, workspace_bytes,
                        (hipStream_t)stream_);
}

// (reports itself as pvs_egnn_layer_fwd_partial, which it is with att_out = NULL)
extern "C" int pvs_egnn_layer_fwd_partial_att(const PvsLayerDesc* d, const PvsGraph* g, const PvsLayerParams* p,
                                              const float* h, const float* x, const float* base_magg,
                                              const float* base_xsum, const float* base_deg, float* h_out,
                                              float* x_out, float* node_att_out, float* att_out, float* saved,
                                              void* workspace, size_t workspace_bytes, pvs_stream_t stream_) {
    return partial_forward(false, "pvs_egnn_layer_fwd_partial", d, g, p, h, x, base_magg, base_xsum, base_deg, h_out,
                           x_out, node_att_out, att_out, saved, workspace, workspace_bytes, (hipStream_t)stream_);
}

extern "C" int pvs_egnn_layer_fwd_partial(const PvsLayerDesc* d, const PvsGraph* g, const PvsLayerParams* p,
                                          const float* h, const float* x, const float* base_magg,
                                          const float* base_xsum, const float* base_deg, float* h_out,
                                          float* x_out, float* node_att_out, float* saved, void* workspace,
                                          size_t workspace_bytes, pvs_stream_t stream_) {
    return pvs_egnn_layer_fwd_partial_att(d, g, p, h, x, base_magg, base_xsum, base_deg, h_out, x_out, node_att_out,
                                          nullptr, saved, workspace, workspace_bytes, stream_);
}

extern "C" int pvs_egnn_layer_edge_stats_softmax(const PvsLayerDesc* d, const PvsGraph* g, const PvsLayerParams* p,
                                                 const float* h, const float* x, float* base_rows, float* xsum,
                                                 void* workspace, size_t workspace_bytes, pvs_stream_t stream_) {
    return partial_base(true, "pvs_egnn_layer_edge_stats_softmax", d, g, p, h, x, base_rows, xsum, workspace,
                        workspace_bytes, (hipStream_t)stream_);
}

extern "C" int pvs_egnn_layer_fwd_partial_softmax(const PvsLayerDesc* d, const PvsGraph* g, const PvsLayerParams* p,
                                                  const float* h, const float* x, const float* base_rows,
                                                  const float* base_xsum, const float* base_deg, float* h_out,
                                                  float* x_out, float* node_att_out, float* att_out, float* saved,
                                                  void* workspace, size_t workspace_bytes, pvs_stream_t stream_) {
    return partial_forward(true, "pvs_egnn_layer_fwd_partial_softmax", d, g, p, h, x, base_rows, base_xsum, base_deg,
                           h_out, x_out, node_att_out, att_out, saved, workspace, workspace_bytes, (hipStream_t)stream_);
}

// ---- the backward as steps (pvs_egnn_layer_bwd below: checks, facts -> plan (layer_plan.h), these steps in order) --------
// Every launch decision is a field of the plan; a step enqueues what the plan says and decides nothing.
namespace {

// The call's tensors, and the pointers the plan settles for all steps
struct BwdCall {
    hipStream_t s;
    const PvsLayerDesc* d;
    const PvsGraph* g;
    const PvsLayerParams* p;
    Dims m;
    const float *h, *x, *m_prev, *att, *g_h_out, *g_x_out, *g_m_out;
    float *g_h, *g_x, *g_m_prev;
    PvsLayerGrads gr;
    PvsNodeW nw;
    const float* g_o;       // w.g_o, or g_h_out itself (plan.g_o_is_g_h_out)
    float* gx_row;          // w.gx_row, or NULL (plan.first_layer)
    PvsLinearExt prep;      // the per-node preparation of the edge backward as row side jobs (plan.prep says of what)
};

// What the edge step leaves for the tail, and the tail for the finalize launch
struct BwdTail {
    PvsReduce2Args edge_red;
    const float* node_gsum = nullptr;
    PvsNodeWgradSlabs node_slabs;
    PvsNodeWgradOut node_out{};
};

// o = u Wn2^T + bn2 backward: g_u = g_o Wn2 (g_o: the workspace's, or g_h_out)
PvsLinearJob bwd_gu_job(const BwdCall& c, const BwdWs& w, const SavedLayout& sv, const float* g_o) {
    const int H = c.m.H;
    PvsLinearJob gu = pvs_linear_job(w.g_u, H, pvs_operand_t(g_o, H, c.p->node_w2, H, H), c.m.N, H);
    gu.aux_in = sv.y1; gu.ld_in = H;
    return gu;
}
// y1 = h Wn1[:, :H]^T + Magg Wn1[:, H:]^T + bn1 backward (g_y1 = w.g_u): g_h (+)= g_y1 Wn1[:, :H], gM = g_y1 Wn1[:, H:]
PvsLinearJob bwd_gh1_job(const BwdCall& c, const BwdWs& w) {
    const int H = c.m.H;
    return pvs_linear_job(c.g_h, H, pvs_operand_t(w.g_u, H, c.p->node_w1, 2 * H, H), c.m.N, H);
}
PvsLinearJob bwd_gm_job(const BwdCall& c, const BwdWs& w) {
    const int H = c.m.H;
    return pvs_linear_job(w.gM, H, pvs_operand_t(w.g_u, H, c.p->node_w1 + H, 2 * H, H), c.m.N, H);
}
// both in one launch: 2H outputs over the two halves of node_mlp.0's weight, the second column block to gM (`ext`)
PvsLinearJob bwd_both_job(const BwdCall& c, const BwdWs& w, const PvsLinearExt* ext) {
    PvsLinearJob both = bwd_gh1_job(c, w);
    both.C = 2 * c.m.H;
    both.ext = ext;
    return both;
}

// 1. output stage (node gate, residual) and the node-gate gradients. The chain kernel, where the plan takes it, is this
// step's launch and does steps 2 and 3 as well.
int bwd_output_stage(const PvsBwdPlan& plan, const BwdCall& c, const BwdWs& w, const SavedLayout& sv) {
    hipStream_t s = c.s;
    const int H = c.m.H, N = c.m.N;
    const uint32_t F = c.d->flags;
    const PvsLayerGrads& gr = c.gr;
    if (plan.node_out_bwd)
        PVS_TRY(pvs_node_out_bwd(s, H, c.g_h_out, sv.o, c.h, c.nw, F, c.d->att_act, N, w.g_o, c.g_h, w.gl, w.t1,
                                 w.tg));
    if (plan.gh_gm == PVS_BWD_GHGM_CHAIN) {
        const bool natt = F & PVS_NODE_ATTENTION;
        PVS_TRY(pvs_launch_node_mlp_bwd(s, H, N, c.g_h_out, sv.o, sv.y1, c.p->node_w1, c.p->node_w2, (F & PVS_RESIDUAL) != 0,
                                        natt ? c.nw.natt_w : nullptr, natt ? c.nw.natt_b : nullptr, c.d->att_act, w.g_o, w.t1,
                                        w.gl, w.g_u, c.g_h, w.gM, &c.prep));
    }
    if (plan.own_node_att_w)
        PVS_TRY(pvs_launch_colreduce(s, PVS_COL_SUM_A, gr.node_att_w, w.t1, H, nullptr, 0, nullptr,
                                     N, H, 1.f, w.dslabs, false));
    if (plan.own_node_att_b)
        PVS_TRY(pvs_launch_colreduce(s, PVS_COL_SUM_A, gr.node_att_b, w.gl, 1, nullptr, 0, nullptr,
                                     N, 1, 1.f, w.dslabs, false));
    if (plan.own_node_gate) {
        PVS_TRY(pvs_launch_colreduce(s, PVS_COL_SUM_A, w.gvec, w.tg, H, nullptr, 0, nullptr, N, H, 1.f,
                                     w.dslabs, false));
        PVS_TRY(pvs_sum_vec(s, w.gvec, H, gr.node_gate));
    }
    return 0;
}

// 2. node MLP backward up to g_y1 (w.g_u, in place), GraphNorm included
int bwd_node_mlp_to_gy1(const PvsBwdPlan& plan, const BwdCall& c, const BwdWs& w, const SavedLayout& sv) {
    hipStream_t s = c.s;
    const int H = c.m.H, N = c.m.N;
    const PvsLayerGrads& gr = c.gr;
    const PvsGraph* g = c.g;
    const PvsNodeW& nw = c.nw;
    const float* sy1 = sv.y1;
    float* stats = sv.stats;
    if (plan.gu_product) {
        PvsLinearJob gu = bwd_gu_job(c, w, sv, c.g_o);
        gu.epi = plan.fuse_tail_bwd ? PVS_EPI_MUL_SILU_GRAD : PVS_EPI_NONE;
        PVS_TRY(pvs_launch_linear(s, gu));
    }
    if (plan.own_node_w2)
        PVS_TRY(pvs_launch_tsgemm_tn(s, gr.node_w2, H, c.g_o, H, sv.u, H, N, H, H, w.dslabs, false));
    if (plan.own_node_b2)
        PVS_TRY(pvs_launch_colreduce(s, PVS_COL_SUM_A, gr.node_b2, c.g_o, H, nullptr, 0, nullptr, N, H,
                                     1.f, w.dslabs, false));
    if (plan.tail_bwd1) PVS_TRY(pvs_node_tail_bwd1(s, w.g_u, sy1, stats, nw, N, H, w.g_u));
    if (plan.graphnorm) {
        PVS_TRY(pvs_launch_colreduce(s, PVS_COL_SUM_A, w.S1, w.g_u, H, nullptr, 0, nullptr, N, H, 1.f,
                                     w.dslabs, false));
        PVS_TRY(pvs_launch_colreduce(s, PVS_COL_SUM_AB, w.S2, w.g_u, H, sy1, H, nullptr, N, H, 1.f,
                                     w.dslabs, false));
        // (g->n_norm_rows_dev: all N rows were normalised by the statistics of the first *n_norm_rows_dev; S1 / S2 stay
        // sums over all N)
        PVS_TRY(pvs_graphnorm_bwd_coefs(s, w.S1, w.S2, stats, nw, N, H, gr.gn_weight, gr.gn_bias,
                                        gr.gn_mean_scale, w.coefs, g->n_norm_rows_dev));
        PVS_TRY(pvs_node_tail_bwd2(s, w.g_u, sy1, stats, nw, w.coefs, N, H, w.g_u, g->n_norm_rows_dev));
    }
    return 0;
}

// 3. g_h / gM from g_y1 with the per-node preparation of the edge backward (plan.prep: layer_plan.h), and the unfused
// weight gradients of node_mlp.0
int bwd_gh_gm(const PvsBwdPlan& plan, const BwdCall& c, const BwdWs& w, const SavedLayout& sv) {
    hipStream_t s = c.s;
    const int H = c.m.H, N = c.m.N;
    const PvsLayerGrads& gr = c.gr;
    const float* g_y1 = w.g_u;
    if (plan.gh_gm == PVS_BWD_GHGM_ONE_PRODUCT) {
        PvsLinearExt ext = c.prep;
        ext.y1 = w.gM; ext.ldy1 = H; ext.acc1 = 0;
        PvsLinearJob both = bwd_both_job(c, w, &ext);
        both.accumulate = plan.gh_accumulate;
        PVS_TRY(pvs_launch_linear(s, both));
    } else if (plan.gh_gm == PVS_BWD_GHGM_TWO_PRODUCTS) {
        PvsLinearJob gh1 = bwd_gh1_job(c, w);
        gh1.accumulate = plan.gh_accumulate;
        PVS_TRY(pvs_launch_linear(s, gh1));
        PvsLinearJob gm = bwd_gm_job(c, w);
        if (plan.prep == PVS_BWD_PREP_SIDE_JOB) gm.ext = &c.prep;
        PVS_TRY(pvs_launch_linear(s, gm));
    }
    if (plan.own_node_w1) {
        PVS_TRY(pvs_launch_tsgemm_tn(s, gr.node_w1, 2 * H, g_y1, H, c.h, H, N, H, H, w.dslabs, false));
        PVS_TRY(pvs_launch_tsgemm_tn(s, gr.node_w1 + H, 2 * H, g_y1, H, sv.Magg, H, N, H, H, w.dslabs,
                                     false));
    }
    if (plan.own_node_b1)
        PVS_TRY(pvs_launch_colreduce(s, PVS_COL_SUM_A, gr.node_b1, g_y1, H, nullptr, 0, nullptr, N, H,
                                     1.f, w.dslabs, false));
    return 0;
}

// 4. edge backward and column gather; leaves the two-set slab reduction as a job (tail->edge_red) and runs it where the
// plan gives it a launch of its own
int bwd_edges(const PvsBwdPlan& plan, const BwdCall& c, const BwdWs& w, const SavedLayout& sv, BwdTail* tail) {
    hipStream_t s = c.s;
    const int H = c.m.H, N = c.m.N;
    const PvsGraph* g = c.g;
    // the softmax row dots, and the per-node preparation where no earlier launch carried it as side jobs
    const PvsLinearExt none;
    const PvsLinearExt& own = plan.prep == PVS_BWD_PREP_OWN_LAUNCH ? c.prep : none;
    PVS_TRY(pvs_prep_edge_bwd(s, c.g_x_out, g->inv_deg, sv.Magg, w.gM, N, H, own.scale3_dst,
                              plan.soft_dots ? w.softD : nullptr, own.zero_rows, own.zero3));
    PvsEdgeBwdIO io;
    io.PQ = sv.PQ; io.x = c.x; io.m_prev = c.m_prev; io.att = c.att; io.gM = w.gM;
    io.gxagg = plan.coord_bwd ? w.gxagg : nullptr;
    io.softD = plan.soft_dots ? w.softD : nullptr;
    io.g_m_out = c.g_m_out; io.gPQ = w.gPQ; io.gz1 = w.gz1; io.gd = w.gd; io.gx_row = c.gx_row;
    io.g_m_prev = plan.edge_res ? c.g_m_prev : nullptr; io.slabs = w.eslabs; io.wpair = w.wpair;
    const PvsEdgeW ew = make_edge_w(c.m, c.p);
    int n_slabs = 0, n_nslabs = 0;
    if (plan.mfma_bwd)
        PVS_TRY(pvs_launch_edge_bwd_mfma(s, H, plan.fam, *g, ew, c.d->flags, c.d->att_act, io, 0, c.m.E, &n_slabs));
    else
        PVS_TRY(pvs_launch_edge_bwd_v0(s, H, *g, ew, c.d->flags, c.d->att_act, io, &n_slabs));
    // (c.gx_row is w.gx_row whenever the generic family runs: the first-layer pair belongs to the split family)
    PVS_TRY(pvs_launch_node_gather(s, H, *g, plan.mfma_bwd, w.gz1, w.gd, c.gx_row, c.g_x_out, w.gPQ, c.g_x,
                                   w.nslabs, 0, N, &n_nslabs));
    const PvsSlabLayout L = pvs_slab_layout(H);
    PvsReduce2Args& r = tail->edge_red;
    r.out_a = w.gsum; r.slabs_a = w.eslabs; r.n_a = n_slabs; r.width_a = L.total;
    r.skip_lo = L.wrho; r.skip_hi = L.wrho + 4 * H;
    r.out_b = w.gsum + L.wrho; r.slabs_b = w.nslabs; r.n_b = n_nslabs; r.width_b = 4 * H;
    if (plan.slab_reduce == PVS_BWD_REDUCE_TWO_SETS)
        PVS_TRY(pvs_launch_reduce_slabs2(s, r.out_a, r.slabs_a, r.n_a, r.width_a, r.skip_lo, r.skip_hi, r.out_b, r.slabs_b,
                                         r.n_b, r.width_b));
    else if (plan.slab_reduce == PVS_BWD_REDUCE_ONE_SET)
        PVS_TRY(pvs_launch_reduce_slabs(s, w.gsum, L.total, L.total, w.eslabs, n_slabs, L.total, false));
    return 0;
}

// 5. first edge-MLP layer at node level (P = W1a h + b1, Q = W1b h): g_h += g_P W1a + g_Q W1b, and the weight-gradient
// tail - the fused pass with the roles the plan folds into it, or the unfused products of edge_mlp.0
int bwd_weight_tail(const PvsBwdPlan& plan, const BwdCall& c, const BwdWs& w, const SavedLayout& sv, BwdTail* tail) {
    hipStream_t s = c.s;
    const Dims& m = c.m;
    const int H = m.H, N = m.N;
    const PvsLayerGrads& gr = c.gr;
    PvsGhJob ghj;
    ghj.g_h = c.g_h; ghj.gPQ = w.gPQ; ghj.W1 = c.p->edge_w1; ghj.ld1 = m.ld1; ghj.off_q = m.off_q;
    if (!plan.gh_folded) PVS_TRY(pvs_launch_linear(s, pvs_gh_linear_job(ghj, N, H)));
    if (plan.fused_wgrads) {
        PvsNodeWgradIn wi;
        wi.g_o = c.g_o; wi.g_y1 = w.g_u; wi.gPQ = w.gPQ; wi.u = sv.u; wi.h = c.h; wi.Magg = sv.Magg;
        PvsNodeWgradOut wo;
        wo.node_w2 = gr.node_w2; wo.node_w1 = gr.node_w1; wo.edge_w1 = gr.edge_w1;
        wo.node_b2 = gr.node_b2; wo.node_b1 = gr.node_b1; wo.edge_b1 = gr.edge_b1;
        wo.ld1 = m.ld1; wo.off_q = m.off_q; wo.perm = m.perm ? 1 : 0;
        if (plan.gate_in_wgrads) { wi.t1 = w.t1; wi.gl = w.gl; wo.natt_w = gr.node_att_w; wo.natt_b = gr.node_att_b; }
        if (plan.tail_folded)
            PVS_TRY(pvs_launch_node_wgrads(s, H, N, wi, wo, w.wslabs, /*scatter=*/false, nullptr, &tail->edge_red,
                                           &tail->node_slabs, plan.gh_folded ? &ghj : nullptr));
        else
            PVS_TRY(pvs_launch_node_wgrads(s, H, N, wi, wo, w.wslabs, /*scatter=*/false, &tail->node_gsum));
        tail->node_out = wo;
    }
    if (plan.own_edge_w1) {
        PVS_TRY(pvs_launch_tsgemm_tn(s, gr.edge_w1, m.ld1, w.gPQ, 2 * H, c.h, H, N, H, H, w.dslabs,
                                     false));
        PVS_TRY(pvs_launch_tsgemm_tn(s, gr.edge_w1 + m.off_q, m.ld1, w.gPQ + H, 2 * H, c.h, H, N, H, H,
                                     w.dslabs, m.perm));
    }
    if (plan.own_edge_b1)
        PVS_TRY(pvs_launch_colreduce(s, PVS_COL_SUM_A, gr.edge_b1, w.gPQ, 2 * H, nullptr, 0, nullptr,
                                     N, H, 1.f, w.dslabs, false));
    return 0;
}

// 6. scatter the reduced sums into the parameter gradients
int bwd_finalize(const PvsBwdPlan& plan, const BwdCall& c, const BwdWs& w, const BwdTail& tail) {
    hipStream_t s = c.s;
    const Dims& m = c.m;
    const int H = m.H;
    const int node_blocks = tail.node_slabs.slabs ? (tail.node_slabs.width + 31) / 32 : 0;
    k_finalize_edge_grads<<<node_blocks + (H * H / 256 > 4 ? H * H / 256 : 4), 256, 0, s>>>(
        w.gsum, pvs_slab_layout(H), H, m.A, m.ld1, m.off_rho, c.gr, plan.coord_bwd ? 1 : 0, plan.has_att,
        plan.has_gate ? 1 : 0, tail.node_gsum, tail.node_out, tail.node_slabs, node_blocks);
    PVS_CHECK_LAUNCH();
    if (plan.node_b1_from_coefs) PVS_TRY(pvs_copy_small(s, w.coefs + 3 * H, c.gr.node_b1, H));
    return 0;
}

}  // namespace

extern "C" int pvs_egnn_layer_bwd(const PvsLayerDesc* d, const PvsGraph* g, const PvsLayerParams* p,
                                  const float* h, const float* x, const float* m_prev,
                                  const float* att, const float* saved, const float* g_h_out,
                                  const float* g_x_out, const float* g_m_out, float* g_h, float* g_x,
                                  float* g_m_prev, const PvsLayerGrads* gr_, void* workspace,
                                  size_t workspace_bytes, pvs_stream_t stream_) {
    PVS_TRY(check_desc(d, g, p));
    PVS_REQUIRE(h && x && saved && g_h_out && g_h && gr_, "pvs_egnn_layer_bwd: NULL tensor");
    PVS_REQUIRE(g->n_edges == 0 || (g->colptr && g->cedge),
                "pvs_egnn_layer_bwd: graph was built without the by-column lists (forward-only)");
    const uint32_t F = d->flags;
    const bool eatt = F & PVS_EDGE_ATTENTION;
    const bool eres = (F & PVS_EDGE_RESIDUAL) && m_prev;
    PVS_REQUIRE(!eatt || att, "pvs_egnn_layer_bwd: att required with edge attention");
    PVS_REQUIRE(!eres || g_m_prev, "pvs_egnn_layer_bwd: g_m_prev required with edge residual");
    const Dims m = make_dims(d, g);
    PvsArena arena(workspace, workspace_bytes);
    BwdWs w;
    carve_bwd(arena, m, &w);
    PVS_REQUIRE(arena.ok(), "pvs_egnn_layer_bwd: workspace too small (%zu < %zu)", workspace_bytes,
                arena.off);
    const int H = m.H;
    // (PQ, y1, o and u = SiLU(GN(y1)) were kept by the forward)
    const SavedLayout sv = saved_layout(const_cast<float*>(saved), m.N, H);      // read-only here
    BwdCall c{(hipStream_t)stream_, d, g, p, m, h, x, m_prev, att, g_h_out, g_x_out, g_m_out, g_h, g_x, g_m_prev, *gr_,
              make_node_w(d, p), nullptr, nullptr, PvsLinearExt{}};
    const PvsLayerGrads& gr = c.gr;

    PvsBwdFacts f;
    f.H = H; f.flags = F; f.n_attr = m.A;
    f.has_m_prev = m_prev != nullptr; f.has_g_x_out = g_x_out != nullptr; f.has_g_x = g_x != nullptr;
    f.no_edges = m.E == 0;
    f.gr_node_w2 = gr.node_w2; f.gr_node_b2 = gr.node_b2; f.gr_node_w1 = gr.node_w1; f.gr_node_b1 = gr.node_b1;
    f.gr_edge_w1 = gr.edge_w1; f.gr_edge_b1 = gr.edge_b1;
    f.gr_node_att_w = gr.node_att_w; f.gr_node_att_b = gr.node_att_b; f.gr_node_gate = gr.node_gate;
    f.wgrads_supported = pvs_node_wgrads_supported(H);
    f.mlp_fused_ok = pvs_node_mlp_fused_supported(H, g_h_out, sv.y1, w.g_u, g_h);
    f.chain_aligned = (((uintptr_t)w.gM | (uintptr_t)w.gPQ | (uintptr_t)sv.o | (uintptr_t)w.g_o | (uintptr_t)w.t1) & 15) == 0;
    f.gu_epilogue_ok = pvs_linear_epilogue_supported(bwd_gu_job(c, w, sv, w.g_o));
    f.gu_passthrough_epilogue_ok = pvs_linear_epilogue_supported(bwd_gu_job(c, w, sv, g_h_out));
    f.gm_epilogue_ok = pvs_linear_epilogue_supported(bwd_gm_job(c, w));
    f.both_epilogue_ok = pvs_linear_epilogue_supported(bwd_both_job(c, w, &c.prep));
    f.sy1_aligned = ((uintptr_t)sv.y1 & 15) == 0;
    f.gpq_aligned = ((uintptr_t)w.gPQ & 15) == 0;
    f.gh_gpq_aligned = (((uintptr_t)g_h | (uintptr_t)w.gPQ) & 15) == 0;
    f.sw = pvs_layer_switches();
    const PvsBwdPlan plan = pvs_layer_bwd_plan(f);

    c.g_o = plan.g_o_is_g_h_out ? g_h_out : w.g_o;
    c.gx_row = plan.first_layer ? nullptr : w.gx_row;
    pvs_note_edge_bwd_variant(plan.first_layer ? PVS_EDGE_BWD_FIRST_LAYER : PVS_EDGE_BWD_GENERAL);
    if (plan.mfma_bwd) { c.prep.zero_rows = w.gPQ; c.prep.zero_w = H; c.prep.zero_ld = 2 * H; c.prep.zero3 = c.gx_row; }
    if (plan.coord_bwd) { c.prep.scale3_src = g_x_out; c.prep.scale3_by = g->inv_deg; c.prep.scale3_dst = w.gxagg; }

    BwdTail tail;
    PVS_TRY(bwd_output_stage(plan, c, w, sv));
    PVS_TRY(bwd_node_mlp_to_gy1(plan, c, w, sv));
    PVS_TRY(bwd_gh_gm(plan, c, w, sv));
    PVS_TRY(bwd_edges(plan, c, w, sv, &tail));
    PVS_TRY(bwd_weight_tail(plan, c, w, sv, &tail));
    return bwd_finalize(plan, c, w, tail);
}


// ---- the whole EGNNLayer stack as one call each way (include/pvs_egnn.h: pvs_egnn_stack_*) -------------------------------
// SartorrasEGNN.get_embeddings loops `for layer in self.layers` (egnn_satorras.py:325-328); at the reference's default shape
// (32 graphs of ~500 atoms, edge_radius 4 A) a training step is ~70 launches of a few microseconds and the HOST decides its
// length: one autograd node and one C call per layer cost more than the layer's kernels. These two entry points sequence
// the very same per-layer launches (pvs_egnn_layer_fwd / _bwd above, unchanged: results are bit for bit those of the
// per-layer calls) over caller-owned buffers that hold every layer's tensors at fixed strides.
namespace {

int check_stack(const PvsLayerDesc* descs, const PvsLayerParams* params, int32_t n_layers, const PvsGraph* g,
                const PvsStackStrides* st, const char* who) {
    PVS_REQUIRE(descs && params && g && st, "%s: NULL descriptor / parameter / graph / stride table", who);
    PVS_REQUIRE(n_layers >= 1 && n_layers <= 1024, "%s: n_layers %d out of range", who, n_layers);
    const int H = descs[0].hidden;
    for (int l = 0; l < n_layers; ++l) {
        PVS_REQUIRE(descs[l].hidden == H, "%s: layer %d has hidden size %d, layer 0 has %d (one width per stack)", who, l,
                    descs[l].hidden, H);
        PVS_REQUIRE(!(descs[l].flags & PVS_EDGE_RESIDUAL),
                    "%s: edge_residual layers hand [E,H] messages from layer to layer: use the per-layer calls", who);
    }
    const size_t N = (size_t)g->n_nodes, E = (size_t)(g->n_edges > 0 ? g->n_edges : 1);
    PVS_REQUIRE(st->h_mid >= (int64_t)(N * H) && st->x_mid >= (int64_t)(3 * N) && st->att >= (int64_t)E &&
                    st->node_att >= (int64_t)N &&
                    st->saved >= (int64_t)pvs_egnn_layer_saved_floats(&descs[0], g->n_nodes, g->n_edges),
                "%s: a stride is smaller than the tensor it separates", who);
    PVS_REQUIRE(((st->h_mid | st->x_mid | st->att | st->node_att | st->saved) & 3) == 0,
                "%s: strides must be multiples of 4 floats (16-byte rows)", who);
    return 0;
}

struct StackBwdScratch {
    float* gh[2];
    float* gx[2];
};

size_t carve_stack_bwd(PvsArena& a, int N, int H, StackBwdScratch* s) {
    StackBwdScratch t;
    for (int k = 0; k < 2; ++k) {
        t.gh[k] = a.take<float>((size_t)N * H);
        t.gx[k] = a.take<float>(3 * (size_t)N);
    }
    if (s) *s = t;
    return pvs_align_up(a.off, 256);
}

}  // namespace

extern "C" size_t pvs_egnn_stack_workspace_bytes(const PvsLayerDesc* descs, int32_t n_layers, int32_t N, int32_t E,
                                                 int32_t backward) {
    if (!descs || n_layers < 1) return 0;
    size_t layer = 0;
    for (int l = 0; l < n_layers; ++l) {
        const size_t b = pvs_egnn_layer_workspace_bytes(&descs[l], N, E, backward ? 1 : 0);
        if (b > layer) layer = b;
    }
    if (!backward) return layer;
    PvsArena a(nullptr, 0);
    return carve_stack_bwd(a, N, descs[0].hidden, nullptr) + layer;
}

extern "C" int pvs_egnn_stack_fwd(const PvsLayerDesc* descs, const PvsLayerParams* params, int32_t n_layers,
                                  const PvsGraph* g, const PvsStackStrides* st, const float* h0, const float* x0,
                                  float* h_mid, float* x_mid, float* h_out, float* x_out, float* att, float* node_att,
                                  float* saved, void* workspace, size_t workspace_bytes, pvs_stream_t stream) {
    PVS_TRY(check_stack(descs, params, n_layers, g, st, "pvs_egnn_stack_fwd"));
    PVS_REQUIRE(h0 && x0 && h_out && x_out && saved && (n_layers == 1 || (h_mid && x_mid)),
                "pvs_egnn_stack_fwd: NULL tensor");
    const float* h = h0;
    const float* x = x0;
    for (int l = 0; l < n_layers; ++l) {
        const bool last = l == n_layers - 1;
        float* ho = last ? h_out : h_mid + (size_t)l * st->h_mid;
        float* xo = last ? x_out : x_mid + (size_t)l * st->x_mid;
        PVS_REQUIRE(!(descs[l].flags & PVS_EDGE_ATTENTION) || att, "pvs_egnn_stack_fwd: att required (layer %d has edge attention)", l);
        PVS_TRY(pvs_egnn_layer_fwd(&descs[l], g, &params[l], h, x, nullptr, ho, xo, nullptr,
                                   att ? att + (size_t)l * st->att : nullptr,
                                   ((descs[l].flags & PVS_NODE_ATTENTION) && node_att) ? node_att + (size_t)l * st->node_att : nullptr,
                                   saved + (size_t)l * st->saved, workspace, workspace_bytes, stream));
        h = ho;
        x = xo;
    }
    return 0;
}

extern "C" int pvs_egnn_stack_bwd(const PvsLayerDesc* descs, const PvsLayerParams* params, int32_t n_layers,
                                  const PvsGraph* g, const PvsStackStrides* st, const float* h0, const float* x0,
                                  const float* h_mid, const float* x_mid, const float* att, const float* saved,
                                  const float* g_h_out, const float* g_x_out, float* g_h0, float* g_x0,
                                  const PvsLayerGrads* grads, void* workspace, size_t workspace_bytes,
                                  pvs_stream_t stream) {
    PVS_TRY(check_stack(descs, params, n_layers, g, st, "pvs_egnn_stack_bwd"));
    for (int l = 0; l < n_layers; ++l)
        PVS_REQUIRE(!(descs[l].flags & PVS_GRAPHNORM_SEGMENTS),
                    "pvs_egnn_stack_bwd: PVS_GRAPHNORM_SEGMENTS is forward-only (layer %d carries it)", l);
    PVS_REQUIRE(h0 && x0 && saved && g_h_out && g_h0 && grads && (n_layers == 1 || (h_mid && x_mid)),
                "pvs_egnn_stack_bwd: NULL tensor");
    PvsArena arena(workspace, workspace_bytes);
    StackBwdScratch sc;
    const size_t own = carve_stack_bwd(arena, g->n_nodes, descs[0].hidden, &sc);
    PVS_REQUIRE(own <= workspace_bytes, "pvs_egnn_stack_bwd: workspace too small (%zu < %zu)", workspace_bytes, own);
    void* layer_ws = (char*)workspace + own;
    const size_t layer_ws_bytes = workspace_bytes - own;
    const float* gh = g_h_out;
    const float* gx = g_x_out;           // NULL: nothing reads the last layer's coordinates
    for (int l = n_layers - 1; l >= 0; --l) {
        const float* h = l ? h_mid + (size_t)(l - 1) * st->h_mid : h0;
        const float* x = l ? x_mid + (size_t)(l - 1) * st->x_mid : x0;
        float* gh_in = l ? sc.gh[l & 1] : g_h0;
        float* gx_in = l ? sc.gx[l & 1] : g_x0;          // (layer 0: NULL when the caller's coordinates need no gradient)
        PVS_TRY(pvs_egnn_layer_bwd(&descs[l], g, &params[l], h, x, nullptr, att ? att + (size_t)l * st->att : nullptr,
                                   saved + (size_t)l * st->saved, gh, gx, nullptr, gh_in, gx_in, nullptr, &grads[l],
                                   layer_ws, layer_ws_bytes, stream));
        gh = gh_in;
        gx = gx_in;
    }
    return 0;
}

// ---- GraphNorm's statistics as an operator (include/pvs_egnn.h: pvs_graphnorm_stats_rows) --------------------------------
extern "C" size_t pvs_graphnorm_stats_rows_workspace_bytes(int32_t n_rows_cap, int32_t H) {
    const size_t h = (size_t)(H > 0 ? H : 0);
    return pvs_align_up(h * sizeof(float), 256) +
           pvs_align_up((size_t)pvs_colreduce_blocks(n_rows_cap) * h * sizeof(float), 256) + 256;
}

extern "C" int pvs_graphnorm_stats_rows(const float* y1, const float* mean_scale, int32_t n_rows_cap, int32_t H,
                                        const int32_t* n_rows_dev, float* stats, void* workspace, size_t workspace_bytes,
                                        pvs_stream_t stream) {
    PVS_REQUIRE(mean_scale && stats && H >= 1 && H <= 256, "pvs_graphnorm_stats_rows: needs mean_scale, stats and 1 <= H <= 256");
    PVS_REQUIRE(n_rows_cap >= (n_rows_dev ? 0 : 1) && (y1 || n_rows_cap == 0),
                "pvs_graphnorm_stats_rows: bad row count %d (the host-count route needs at least one row)", n_rows_cap);
    PvsArena arena(workspace, workspace_bytes);
    float* shift = arena.take<float>((size_t)H);
    float* slabs = arena.take<float>((size_t)pvs_colreduce_blocks(n_rows_cap) * H);
    PVS_REQUIRE(arena.ok(), "pvs_graphnorm_stats_rows: workspace too small (%zu < %zu)", workspace_bytes, arena.off);
    return pvs_graphnorm_stats((hipStream_t)stream, y1, mean_scale, n_rows_cap, H, stats, shift, slabs, n_rows_dev);
}

// ---- GraphNorm's statistics per node segment as an operator (include/pvs_egnn.h: pvs_graphnorm_stats_segments) ----------
extern "C" size_t pvs_graphnorm_stats_segments_workspace_bytes(int32_t n_rows_cap, int32_t n_segments, int32_t H) {
    const size_t h = (size_t)(H > 0 ? H : 0);
    return pvs_align_up(pvs_colmean_segments_slabs(n_rows_cap, n_segments) * h * sizeof(float), 256) + 256;
}

extern "C" int pvs_graphnorm_stats_segments(const float* y1, const float* mean_scale, int32_t n_rows_cap, int32_t H,
                                            const int32_t* seg_ptr, int32_t n_segments, float* stats, void* workspace,
                                            size_t workspace_bytes, pvs_stream_t stream) {
    PVS_REQUIRE(mean_scale && stats && H >= 1 && H <= 256,
                "pvs_graphnorm_stats_segments: needs mean_scale, stats and 1 <= H <= 256");
    PVS_REQUIRE(seg_ptr && n_segments >= 1, "pvs_graphnorm_stats_segments: needs a segment table with at least one segment");
    PVS_REQUIRE(n_rows_cap >= 0 && (y1 || n_rows_cap == 0), "pvs_graphnorm_stats_segments: bad row capacity %d", n_rows_cap);
    PvsArena arena(workspace, workspace_bytes);
    float* slabs = arena.take<float>(pvs_colmean_segments_slabs(n_rows_cap, n_segments) * (size_t)H);
    PVS_REQUIRE(arena.ok(), "pvs_graphnorm_stats_segments: workspace too small (%zu < %zu)", workspace_bytes, arena.off);
    return pvs_graphnorm_stats_segments_launch((hipStream_t)stream, y1, mean_scale, n_rows_cap, H, seg_ptr, n_segments, stats,
                                               slabs);
}
