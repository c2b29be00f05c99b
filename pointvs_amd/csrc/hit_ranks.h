// The order relation of the per-hit ranks (hit_ranks.hip: pvs_hit_value_ranks) and which ligand ranges it accepts.
// The candidates of a hit are its ligand values (position = packed order) followed by its receptor values (position =
// n_lig + atom); u stands before v iff u > v, or u == v and u's position is lower: the position of a descending STABLE
// sort. -0.0 == +0.0, the infinities are ordinary values, a NaN is no candidate and stands before nothing.
// No HIP header: the host compiler builds this file alone.
#pragma once
#include <stdint.h>
#include "contact_attention.h"

enum { kPvsRankTile = 1024 };       // candidates of a hit that one workgroup holds in LDS at a time

// Does candidate (u, at position pu) stand before candidate (v, at position pv)? Either one NaN: no.
PVS_CONTACT_FN bool pvs_rank_before(float u, int32_t pu, float v, int32_t pv) {
    return u > v || (u == v && pu < pv);
}

// Hit h of the table lig_ptr [n_hits + 1] (NULL: no ligand values, every hit has none): its first packed ligand value
// and how many it has. n < 0: no hit - the range is negative, descends or has more than 1024 atoms.
struct PvsRankHit {
    int32_t a0, n;
};

PVS_CONTACT_FN PvsRankHit pvs_rank_hit(const int32_t* lig_ptr, int h) {
    if (!lig_ptr) return PvsRankHit{0, 0};
    const long long a0 = lig_ptr[h], a1 = lig_ptr[h + 1];
    if (a0 < 0 || a1 < a0 || a1 - a0 > kPvsContactMaxLigand) return PvsRankHit{0, -1};
    return PvsRankHit{(int32_t)a0, (int32_t)(a1 - a0)};
}
