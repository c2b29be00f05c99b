// What pvs_screen_copies_build refuses of a PvsScreenCopiesJob (pvs_egnn.h), in one place: its own three tables first,
// then everything pvs_screen_slots_build refuses of the embedded job (screen_job.h, under that entry's name). Every
// refusal is made on the host before anything is launched; pvs_screen_copies_state_bytes answers 0 for what the count
// part refuses.
// No HIP header: the host compiler builds this file alone (tests/test_crop_copies_host.py).
#pragma once
#include "screen_job.h"

constexpr const char* kPvsScreenCopiesWho = "pvs_screen_copies_build";

// nullptr for a job that the build takes, else the refusal, written into `why`. counts_only: the layout and the counts
// alone (what the state's size depends on), no pointer, radius or table.
inline const char* pvs_screen_copies_refusal(const PvsScreenCopiesJob& j, bool counts_only, char* why, size_t n) {
    const char* who = kPvsScreenCopiesWho;
#define PVS_COPIES_REFUSE(cond, ...)                \
    do {                                            \
        if (cond) {                                 \
            snprintf(why, n, __VA_ARGS__);          \
            return why;                             \
        }                                           \
    } while (0)
    PVS_COPIES_REFUSE(j.slots.layout != PVS_SLOTS_CROPPED, "%s: the embedded job must state PVS_SLOTS_CROPPED (layout %d)",
                      who, j.slots.layout);
    if (!counts_only) {
        PVS_COPIES_REFUSE(j.slots.rec_drop, "%s: slots.rec_drop must be NULL (the copies' rec_drop is the job's own)", who);
        PVS_COPIES_REFUSE(!j.crop_pos, "%s: NULL crop_pos", who);
        PVS_COPIES_REFUSE(!j.crop_ptr, "%s: NULL crop_ptr", who);
    }
    if (const char* embedded = pvs_screen_job_refusal(j.slots, counts_only, why, n)) return embedded;
    PVS_COPIES_REFUSE(j.crop_cap < 1 || j.crop_cap > kPvsMaxSlotCap * (int64_t)j.slots.n_slots,
                      "%s: crop_cap must be 1..%d * slots (got %d for %d)", who, kPvsMaxSlotCap, j.crop_cap,
                      j.slots.n_slots);
#undef PVS_COPIES_REFUSE
    return nullptr;
}
