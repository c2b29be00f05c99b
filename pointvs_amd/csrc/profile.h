// Optional per-kernel timing with HIP events on the launch stream (bench.py's roofline leg).
#pragma once
#include <hip/hip_runtime.h>

enum { PVS_PROF_EDGE_FWD = 0, PVS_PROF_EDGE_BWD = 1, PVS_PROF_COL_GATHER = 2, PVS_PROF_PREPARE = 3,
       PVS_PROF_EDGE_FWD_PARTIAL = 4,   // the screening path's ligand-edges-only first layer
       PVS_PROF_MASK_GRAPH = 5,         // the leave-out batch builder of masking attribution
       // The dispatch routes of the dense launchers (dense_ops.hip), one id per branch, so that a test can see which
       // branch a shape took. Recorded only when their own mask bit is set: "every category" (bit 0) leaves them out.
       PVS_PROF_DENSE_FIRST = 6,
       PVS_PROF_LIN_MFMA = 6, PVS_PROF_LIN_CHUNK64 = 7, PVS_PROF_LIN_CHUNK256 = 8, PVS_PROF_LIN_GENERIC = 9,
       PVS_PROF_TS_MFMA = 10, PVS_PROF_TS_WIDE = 11, PVS_PROF_TS_COLCHUNK = 12, PVS_PROF_TS_NARROW = 13,
       PVS_PROF_TS_TN8 = 14, PVS_PROF_TS_TN32 = 15,
       PVS_PROF_COLREDUCE4 = 16, PVS_PROF_COLREDUCE = 17, PVS_PROF_COLREDUCE_CHUNK = 18,
       // The node-level launchers of a layer (dense_ops.hip: the folded node MLP and the fused weight-gradient pass;
       // node_ops.hip: the separate tail and output stage), one id per launcher, the three tail launchers under one: which
       // of the two node routes a layer call took. Recorded like the dense routes, under their own mask bit only.
       PVS_PROF_NODE_MLP_FWD = 19, PVS_PROF_NODE_MLP_BWD = 20, PVS_PROF_NODE_OUT_FWD = 21, PVS_PROF_NODE_OUT_BWD = 22,
       PVS_PROF_NODE_TAIL = 23, PVS_PROF_NODE_WGRADS = 24,
       // GraphNorm over a device row count (PvsGraph.n_norm_rows_dev): the column means over the leading rows, and the
       // tail launchers that read the count (the coefficients and the row-bounded second backward pass)
       PVS_PROF_COLREDUCE4_ROWS = 25, PVS_PROF_COLREDUCE_ROWS = 26, PVS_PROF_NODE_TAIL_ROWS = 27,
       // GraphNorm per node segment (PVS_GRAPHNORM_SEGMENTS): the column means of every segment, and the tail that picks
       // each row's pair
       PVS_PROF_COLREDUCE4_SEGS = 28, PVS_PROF_COLREDUCE_SEGS = 29, PVS_PROF_NODE_TAIL_SEGS = 30,
       PVS_PROF_COUNT = 31 };
static_assert(PVS_PROF_COUNT + 1 <= 32, "the profile mask is an unsigned with bit (id + 1) per category");

// tag the edge forward launches of the calling thread carry (layer_api: full layer vs partial layer)
void pvs_prof_set_fwd_tag(int id);
int pvs_prof_fwd_tag();

// which edge-backward pair the last pvs_egnn_layer_bwd of the process launched (pvs_edge_bwd_last_variant, pvs_egnn.h)
enum { PVS_EDGE_BWD_NONE = -1, PVS_EDGE_BWD_GENERAL = 0, PVS_EDGE_BWD_FIRST_LAYER = 1 };
void pvs_note_edge_bwd_variant(int variant);

struct PvsProfScope {
    hipStream_t s;
    void* rec;
    PvsProfScope(hipStream_t stream, int id);
    ~PvsProfScope();
};
