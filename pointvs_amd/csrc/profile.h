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
       PVS_PROF_COUNT = 19 };

// tag the edge forward launches of the calling thread carry (layer_api: full layer vs partial layer)
void pvs_prof_set_fwd_tag(int id);
int pvs_prof_fwd_tag();

struct PvsProfScope {
    hipStream_t s;
    void* rec;
    PvsProfScope(hipStream_t stream, int id);
    ~PvsProfScope();
};
