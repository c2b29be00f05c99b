// Which of two poses is the better one (pose_select.hip: the best pose of every ligand of a sweep). A candidate is a
// score and the row it came from; "better" is a strict order on candidates, so the winner of a set is the same
// whichever way its members are paired up - a lane's loop over rows and the butterfly over the wave's lanes may meet
// them in any order:
//   - a candidate without a row (index < 0) or with a NaN score beats nothing, and everything else beats it;
//   - the larger score wins (-inf is a score like any other, -0.0 and +0.0 are equal);
//   - equal scores go to the lower row.
// No HIP header: the host compiler builds this file alone (tests/test_two_head_screen_host.py).
#pragma once
#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#define PVS_POSE_FN __host__ __device__ inline
#else
#define PVS_POSE_FN inline
#endif

struct PvsPosePick {
    float value;
    int32_t index;      // row, counted from the segment's first; < 0: none
};

// What a segment without a usable row gives: no row, a NaN score. Every candidate that beats nothing merges to this.
PVS_POSE_FN PvsPosePick pvs_pose_none() { return PvsPosePick{NAN, -1}; }

PVS_POSE_FN bool pvs_pose_usable(PvsPosePick p) { return p.index >= 0 && !(p.value != p.value); }

// True when a is strictly better than b.
PVS_POSE_FN bool pvs_pose_better(PvsPosePick a, PvsPosePick b) {
    if (!pvs_pose_usable(a)) return false;
    if (!pvs_pose_usable(b)) return true;
    return a.value > b.value || (a.value == b.value && a.index < b.index);
}

// The better of the two; pvs_pose_none() when neither is usable (so that the merge is commutative on those too).
PVS_POSE_FN PvsPosePick pvs_pose_merge(PvsPosePick a, PvsPosePick b) {
    if (pvs_pose_better(a, b)) return a;
    if (pvs_pose_better(b, a)) return b;
    return pvs_pose_usable(a) ? a : pvs_pose_none();      // (neither better: the same candidate twice, or none usable)
}
