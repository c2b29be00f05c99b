// Host-side choices of a layer call, in one place: the layer-level A/B switches and the launch set of the backward
// (layer_api.hip: pvs_egnn_layer_bwd fills the facts, gets the plan and runs its steps; no step decides anything).
// Plain C++ (no HIP types): tests/test_layer_bwd_plan_host.py compiles it alone with the host compiler.
#pragma once
#include "edge_dispatch.h"

// ---- layer-level switches --------------------------------------------------------------------------------------------
// The ONLY place that reads them (the family and first-layer switches: edge_dispatch.h):
//   PVS_EGNN_SPLIT_SMALL    every folded node-level launch apart (A/B, and the tests' reference run)
//   PVS_EGNN_SPLIT_WGRADS   the node-level weight gradients as launches of their own instead of the fused pass (A/B; the
//                           same launches serve H = 16 / 128 and callers that ask for only some gradients)
// (The A/B switches are read from the environment at EVERY call on purpose - ADVICE r03 suggested statics: the test suite
// and tools/abenv.py flip them inside one process, e.g. the exact-fp32 family against the split products on the same
// tensors. A getenv is ~0.2 us of host time; a layer call enqueues 6-9 launches of >= 3 us each.)
struct PvsLayerSwitches {
    bool split_small, split_wgrads;
};
inline PvsLayerSwitches pvs_layer_switches() {
    return PvsLayerSwitches{getenv("PVS_EGNN_SPLIT_SMALL") != nullptr, getenv("PVS_EGNN_SPLIT_WGRADS") != nullptr};
}

// ---- what the backward's decisions depend on -------------------------------------------------------------------------
// The pointer questions are answered by the call site from the real pointers (dense_ops.h); the plan sees booleans.
struct PvsBwdFacts {
    int H = 0;
    uint32_t flags = 0;
    int n_attr = 0;
    bool has_m_prev = false, has_g_x_out = false, has_g_x = false;
    bool no_edges = false;                  // E == 0
    // gradient slots of PvsLayerGrads that are non-NULL (the others go to kernels as they are)
    bool gr_node_w2 = false, gr_node_b2 = false, gr_node_w1 = false, gr_node_b1 = false, gr_edge_w1 = false,
         gr_edge_b1 = false, gr_node_att_w = false, gr_node_att_b = false, gr_node_gate = false;
    bool wgrads_supported = false;          // pvs_node_wgrads_supported(H)
    bool mlp_fused_ok = false;              // pvs_node_mlp_fused_supported(H, g_h_out, saved y1, g_u, g_h)
    bool chain_aligned = false;             // gM | gPQ | saved o | g_o | t1 on 16 bytes
    bool gu_epilogue_ok = false;            // pvs_linear_epilogue_supported of g_u = g_o Wn2 with the workspace's g_o
    bool gu_passthrough_epilogue_ok = false;    //   of the same product reading g_h_out (which of the two: the plan's
                                            //   g_o_is_g_h_out, so the call site answers for both pointers)
    bool gm_epilogue_ok = false;            //   of gM = g_y1 Wn1[:, H:]
    bool both_epilogue_ok = false;          //   of [g_h | gM] = g_y1 Wn1 as one double-width product
    bool sy1_aligned = false;               // saved y1 on 16 bytes
    bool gpq_aligned = false;               // gPQ on 16 bytes
    bool gh_gpq_aligned = false;            // g_h | gPQ on 16 bytes
    PvsLayerSwitches sw = {false, false};
};

// How g_h / gM come from g_y1
enum PvsBwdGhGm {
    PVS_BWD_GHGM_CHAIN,         // k_node_mlp_bwd: output stage, g_y1 and [g_h | gM] in one launch
    PVS_BWD_GHGM_ONE_PRODUCT,   // one double-width product, the second column block to gM (H = 32)
    PVS_BWD_GHGM_TWO_PRODUCTS,  // g_h (+)= and gM = as a launch each
};
// Where the per-node preparation of the edge backward rides: clear the row half of gPQ and gx_row (rows without edges
// are never written by the MFMA edge backward) and gxagg = g_x_out * inv_deg. Exactly one launch does it.
enum PvsBwdPrep {
    PVS_BWD_PREP_CHAIN,         // row side jobs of k_node_mlp_bwd
    PVS_BWD_PREP_SIDE_JOB,      // row side jobs of the gM product (of the double-width product where that one runs)
    PVS_BWD_PREP_OWN_LAUNCH,    // pvs_prep_edge_bwd, which otherwise forms the softmax row dots only
};
// Which launch turns the edge backward's and the column gather's slabs into gsum
enum PvsBwdSlabReduce {
    PVS_BWD_REDUCE_ONE_SET,     // generic family: pvs_launch_reduce_slabs over the edge slabs (its gather writes no slabs)
    PVS_BWD_REDUCE_TWO_SETS,    // pvs_launch_reduce_slabs2
    PVS_BWD_REDUCE_FOLDED,      // extra workgroups of the fused weight-gradient pass
};

struct PvsBwdPlan {
    // -- edge side
    PvsEdgeFamily fam = PVS_EDGE_GENERIC;
    bool mfma_bwd = false;
    bool first_layer = false;       // the first-layer pair: gx_row == NULL for the edge launcher AND the gather
    bool coord_bwd = false;         // a coordinate gradient arrives: gxagg is formed and read
    bool soft_dots = false;         // softmax attention: the row dots of pvs_prep_edge_bwd
    bool edge_res = false;          // the edge residual is live (flag and m_prev): g_m_prev is written
    // -- output stage and node-gate gradients
    bool node_out_bwd = false;      // pvs_node_out_bwd as a launch of its own (it initialises g_h)
    bool g_o_is_g_h_out = false;    // g_o = g_h_out: nothing is written for it
    bool gate_in_wgrads = false;
    bool own_node_att_w = false, own_node_att_b = false, own_node_gate = false;      // column reductions of their own
    // -- node MLP
    bool fused_wgrads = false;
    bool gu_product = false;        // g_u = g_o Wn2 as a launch of its own
    bool fuse_tail_bwd = false;     //   with g_y1 = g_u * SiLU'(y1) on its epilogue
    bool tail_bwd1 = false;         // pvs_node_tail_bwd1 as a launch of its own
    bool graphnorm = false;
    PvsBwdGhGm gh_gm = PVS_BWD_GHGM_TWO_PRODUCTS;
    bool gh_accumulate = false;     // the product(s) add to a g_h that pvs_node_out_bwd initialised
    PvsBwdPrep prep = PVS_BWD_PREP_OWN_LAUNCH;
    bool own_node_w2 = false, own_node_b2 = false, own_node_w1 = false, own_node_b1 = false, own_edge_w1 = false,
         own_edge_b1 = false;       // unfused weight gradients: products / column reductions of their own
    bool node_b1_from_coefs = false;
    // -- tail
    PvsBwdSlabReduce slab_reduce = PVS_BWD_REDUCE_ONE_SET;
    bool tail_folded = false;
    bool gh_folded = false;         // g_h += gP W1a + gQ W1b as a role of the weight-gradient launch
    int has_att = 0;                // k_finalize_edge_grads: 0 none, 1 sigmoid, 2 softmax
    bool has_gate = false;          //   the edge gate's gradient is due
};

// Every launch decision of pvs_egnn_layer_bwd, in the order of the launches they select.
inline PvsBwdPlan pvs_layer_bwd_plan(const PvsBwdFacts& f) {
    const uint32_t F = f.flags;
    const bool gn = F & PVS_GRAPHNORM, natt = F & PVS_NODE_ATTENTION;
    const bool gates = (F & PVS_RESIDUAL) && (F & (PVS_REZERO | PVS_GATED_RESIDUAL));
    const bool eatt = F & PVS_EDGE_ATTENTION, soft = F & PVS_SOFTMAX_ATT;
    const bool split_small = f.sw.split_small;      // (the launches apart, for A/B)
    PvsBwdPlan p;
    p.graphnorm = gn;
    p.edge_res = (F & PVS_EDGE_RESIDUAL) && f.has_m_prev;
    p.coord_bwd = (F & PVS_UPDATE_COORDS) && f.has_g_x_out;
    p.soft_dots = eatt && soft;
    // all node-level weight gradients in one pass at the end (H = 32, 64, the usual full set of grads)
    p.fused_wgrads = f.wgrads_supported && f.gr_node_w2 && f.gr_node_w1 && f.gr_edge_w1 && !f.sw.split_wgrads;
    p.fam = pvs_edge_family(f.H, F, f.n_attr, PVS_EDGE_BWD);
    p.mfma_bwd = p.fam != PVS_EDGE_GENERIC;
    // Nobody asks for the gradient of this layer's input coordinates (the first layer of a model, whichever entry point
    // the call came through): the first-layer pair, which neither forms nor sums it (edge_dispatch.h). gx_row == NULL is
    // how the two launchers are told.
    p.first_layer = pvs_first_layer_bwd(f.H, F, f.n_attr, f.has_m_prev, f.has_g_x_out, f.has_g_x);

    // Layers without GraphNorm and without rezero / gated residual: the output stage (node gate, residual), g_y1 and
    // [g_h | gM] as ONE launch that also carries the per-node preparation of the edge backward (dense_ops.hip:
    // k_node_mlp_bwd). Without a node gate g_o is g_h_out itself and nothing is written for it.
    const bool chain_bwd = !gn && !gates && !split_small && f.mlp_fused_ok && f.chain_aligned;
    // (no residual, no node gate: g_o = g_h_out and the residual's part of g_h is zero - nothing to launch either way)
    const bool plain_out = !(F & PVS_RESIDUAL) && !natt && !split_small;
    p.g_o_is_g_h_out = plain_out || (chain_bwd && !natt);
    p.node_out_bwd = !plain_out && !chain_bwd;
    // (the node gate's weight gradients - column sums of t1, sum of gl - ride on the fused weight-gradient pass when
    // it runs: two column reductions and their slab reductions less per layer)
    p.gate_in_wgrads = natt && p.fused_wgrads && !split_small && f.gr_node_att_w && f.gr_node_att_b;
    p.own_node_att_w = natt && !p.gate_in_wgrads && f.gr_node_att_w;
    p.own_node_att_b = natt && !p.gate_in_wgrads && f.gr_node_att_b;
    p.own_node_gate = gates && f.gr_node_gate;

    // o = u Wn2^T + bn2
    // (without GraphNorm g_y1 = g_u * SiLU'(y1) rides on this product's epilogue)
    p.gu_product = !chain_bwd;
    p.fuse_tail_bwd = !gn && (p.g_o_is_g_h_out ? f.gu_passthrough_epilogue_ok : f.gu_epilogue_ok) && f.sy1_aligned;
    p.own_node_w2 = f.gr_node_w2 && !p.fused_wgrads;
    p.own_node_b2 = f.gr_node_b2 && !p.fused_wgrads;
    // u = SiLU(GN(y1)) ; g_u becomes g_yn then g_y1 in place
    p.tail_bwd1 = !p.fuse_tail_bwd && !chain_bwd;

    // y1 = h Wn1[:, :H]^T + Magg Wn1[:, H:]^T + bn1
    // The per-node preparation of the edge backward (clear the row part of gPQ and gx_row - rows without edges are
    // never written by the MFMA edge backward -, g_x_out / deg) rides on these products as side jobs of the node rows
    // where the MFMA linear takes the shape; the softmax row dots need the finished gM and keep their own launch.
    p.gh_accumulate = !plain_out;
    const bool prep_side = !split_small && f.gpq_aligned && f.gm_epilogue_ok;
    if (chain_bwd) {
        p.gh_gm = PVS_BWD_GHGM_CHAIN;
        p.prep = PVS_BWD_PREP_CHAIN;
    } else if (f.H == 32 && prep_side && f.both_epilogue_ok) {
        // g_h (+)= and gM = in one launch: 64 outputs over the two halves of node_mlp.0's weight, the second column block
        // to gM
        p.gh_gm = PVS_BWD_GHGM_ONE_PRODUCT;
        p.prep = PVS_BWD_PREP_SIDE_JOB;
    } else {
        p.gh_gm = PVS_BWD_GHGM_TWO_PRODUCTS;
        // (MFMA path: rows without edges are never written by the edge kernel: cleared by pvs_prep_edge_bwd, unless done
        // by a side job)
        p.prep = prep_side ? PVS_BWD_PREP_SIDE_JOB : PVS_BWD_PREP_OWN_LAUNCH;
    }
    p.own_node_w1 = f.gr_node_w1 && !p.fused_wgrads;
    p.own_node_b1 = f.gr_node_b1 && !p.fused_wgrads;

    // g_wrho / g_wattr come from the node gather: its slab layout [wrho | wattr0 | wattr1 | wattr2]
    // == gsum[L.wrho .. L.wrho + 4H), which the edge slabs leave alone (one reduction for both). With the fused
    // weight-gradient pass that reduction rides on ITS launch as extra workgroups (independent work), and the
    // pass's own slab reduction on the finalize launch: three launches at the end of a layer instead of five.
    p.tail_folded = p.mfma_bwd && p.fused_wgrads && !split_small;
    p.slab_reduce = !p.mfma_bwd ? PVS_BWD_REDUCE_ONE_SET : p.tail_folded ? PVS_BWD_REDUCE_FOLDED : PVS_BWD_REDUCE_TWO_SETS;
    // first edge-MLP layer at node level: P = W1a h + b1, Q = W1b h
    // g_h += g_P W1a + g_Q W1b: one launch with the two (input, weight) pairs
    // (with the folded tail it is a role of the weight-gradient launch)
    p.gh_folded = p.tail_folded && f.gh_gpq_aligned;
    p.own_edge_w1 = f.gr_edge_w1 && !p.fused_wgrads;
    p.own_edge_b1 = f.gr_edge_b1 && !p.fused_wgrads;
    p.has_att = eatt ? (soft ? 2 : 1) : 0;
    // (a graph without edges: the caller's [0, H] m_prev has no device pointer, yet the edge gate is a parameter of the
    // layer and its gradient - the sum over no edges - is 0, not whatever the caller's buffer held)
    const bool gate_grad = p.edge_res || ((F & PVS_EDGE_RESIDUAL) && f.no_edges);
    p.has_gate = gate_grad && (F & (PVS_REZERO | PVS_GATED_RESIDUAL));
    // GraphNorm: node_mlp.0.bias from the closed form of k_gn_bwd_coefs instead of the column sum of g_y1
    p.node_b1_from_coefs = gn && f.gr_node_b1;
    return p;
}
