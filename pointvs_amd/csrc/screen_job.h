// What pvs_screen_slots_build refuses of a PvsScreenSlotsJob (pvs_egnn.h), in one place: the layout and the fields that
// go with it, the counts, the node tables. Every refusal is made on the host before anything is launched;
// pvs_screen_slots_state_bytes answers 0 for what the count part refuses.
// No HIP header: the host compiler builds this file alone (tests/test_screen_job_host.py).
#pragma once
#include "../../include/pvs_egnn.h"
#include "screen_slots.h"
#include <stdio.h>

constexpr const char* kPvsScreenJobWho = "pvs_screen_slots_build";

// The node tables that the job's kernels get. A cropped row has lost template neighbours, so the receptor's first-layer
// sums are not its sums: under PVS_SLOTS_CROPPED the base tables are dropped, whatever they hold.
inline PvsRaggedNodeTables pvs_screen_job_tables(const PvsScreenSlotsJob& j) {
    PvsRaggedNodeTables t = j.tables;
    if (j.layout == PVS_SLOTS_CROPPED) {
        t.hidden = 0;
        t.rec_magg = t.rec_xsum = t.rec_deg = nullptr;
        t.base_magg = t.base_xsum = t.base_deg = nullptr;
    }
    return t;
}

// nullptr for a job that the build takes, else the refusal, written into `why`. counts_only: the layout and the counts
// alone (what the state's size depends on), no pointer, radius or table.
inline const char* pvs_screen_job_refusal(const PvsScreenSlotsJob& j, bool counts_only, char* why, size_t n) {
    const char* who = kPvsScreenJobWho;
#define PVS_JOB_REFUSE(cond, ...)                   \
    do {                                            \
        if (cond) {                                 \
            snprintf(why, n, __VA_ARGS__);          \
            return why;                             \
        }                                           \
    } while (0)
    const bool struck = j.layout == PVS_SLOTS_STRUCK, cropped = j.layout == PVS_SLOTS_CROPPED;
    PVS_JOB_REFUSE(j.layout != PVS_SLOTS_RAGGED && !struck && !cropped, "%s: unknown layout %d", who, j.layout);
    if (!counts_only) {
        const struct { const char* name; const void* p; bool needed; } fields[] = {
            {"lig_pos", j.lig_pos, true}, {"lig_ptr", j.lig_ptr, true}, {"rec_drop", j.rec_drop, struck},
            {"rec_pos", j.rec_pos, true}, {"rr_rowptr", j.rr_rowptr, true}, {"rr_col", j.rr_col, true},
            {"full.rowptr", j.full.rowptr, true}, {"full.row", j.full.row, true}, {"full.col", j.full.col, true},
            {"full.etype", j.full.etype, true}, {"lig.rowptr", j.lig.rowptr, !cropped},
            {"lig.row", j.lig.row, !cropped}, {"lig.col", j.lig.col, !cropped}, {"lig.etype", j.lig.etype, !cropped},
            {"inv_deg", j.inv_deg, true}, {"node_ptr", j.node_ptr, true}, {"node_graph", j.node_graph, true},
            {"pos", j.pos, true}, {"keep", j.keep, cropped}, {"status", j.status, true}};
        for (const auto& f : fields) PVS_JOB_REFUSE(f.needed && !f.p, "%s: NULL %s", who, f.name);
        PVS_JOB_REFUSE(j.rec_drop && !struck, "%s: rec_drop goes with PVS_SLOTS_STRUCK only (layout %d)", who,
                       j.layout);
        PVS_JOB_REFUSE(j.crop_radius > 0.0 && !cropped, "%s: crop_radius goes with PVS_SLOTS_CROPPED only (layout %d)",
                       who, j.layout);
    }
    PVS_JOB_REFUSE(j.slot_cap < 1 || j.slot_cap > kPvsMaxSlotCap, "%s: slot_cap must be 1..%d (got %d)", who,
                   kPvsMaxSlotCap, j.slot_cap);
    PVS_JOB_REFUSE(j.n_slots <= 0 || j.lig_cap <= 0 || j.lig_cap > j.slot_cap * (int64_t)j.n_slots || j.n_rec <= 0,
                   "%s: needs slots, 1..%d * slots packed ligand atoms (got %d for %d) and a receptor", who, j.slot_cap,
                   j.lig_cap, j.n_slots);
    PVS_JOB_REFUSE((int64_t)j.lig_cap + (int64_t)j.n_slots * j.n_rec >= INT32_MAX, "%s: more than 2^31 nodes", who);
    if (counts_only) return nullptr;
    PVS_JOB_REFUSE(cropped && !(j.crop_radius > 0.0), "%s: crop_radius must be positive (got %g)", who, j.crop_radius);
    const PvsRaggedNodeTables t = pvs_screen_job_tables(j);
    PVS_JOB_REFUSE(t.n_feats < 0 || t.hidden < 0, "%s: negative table width", who);
    PVS_JOB_REFUSE(t.feats && !(t.lig_feats && t.rec_feats && t.n_feats > 0), "%s: feature table without sources", who);
    PVS_JOB_REFUSE(t.base_magg && !(t.rec_magg && t.rec_xsum && t.rec_deg && t.base_xsum && t.base_deg && t.hidden > 0),
                   "%s: receptor sums incomplete", who);
#undef PVS_JOB_REFUSE
    return nullptr;
}
