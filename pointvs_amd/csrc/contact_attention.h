// The order relation of the contact-attention reduction (contact_attention.hip: pvs_contact_attention) and which
// slots of a pose batch it accepts. The larger value wins, a NaN never does, equal values are one value and +0.0
// stands above -0.0: a maximum under this relation is the same bits in whatever order the candidates meet, which is
// what lets the lanes of a wavefront share a row and a later launch geometry give the same result.
// No HIP header: the host compiler builds this file alone.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define PVS_CONTACT_FN __host__ __device__ inline
#else
#define PVS_CONTACT_FN inline
#endif

enum { kPvsContactMaxLigand = 1024 };       // ligand atoms of a slot (screen_slots.h: kPvsMaxSlotCap)

// max(cur, v); NaN = "nothing yet" for cur, "skip" for v.
PVS_CONTACT_FN float pvs_contact_max(float cur, float v) {
    if (v != v) return cur;
    if (cur != cur || v > cur) return v;
    return (v == cur && __builtin_signbit(cur)) ? v : cur;       // (-0.0 gives way to +0.0)
}

// Slot p of the tables node_ptr / lig_ptr [n_slots + 1]: its first packed ligand atom, its ligand atom count and its
// first row. n < 0: no slot (the tables disagree, or its rows do not fit n_nodes rows of which n_slots * n_rec are
// receptor rows).
struct PvsContactSlot {
    int32_t a0, n, node0;
};

PVS_CONTACT_FN PvsContactSlot pvs_contact_slot(const int32_t* node_ptr, const int32_t* lig_ptr, int p, int n_slots,
                                               int n_rec, int n_nodes) {
    const long long a0 = lig_ptr[p], a1 = lig_ptr[p + 1];
    const long long lig_room = (long long)n_nodes - (long long)n_slots * n_rec;
    const bool ok = a0 >= 0 && a1 >= a0 && a1 - a0 <= kPvsContactMaxLigand && a1 <= lig_room &&
                    node_ptr[p] == a0 + (long long)p * n_rec && node_ptr[p + 1] == a1 + (long long)(p + 1) * n_rec;
    if (!ok) return PvsContactSlot{0, -1, 0};
    return PvsContactSlot{(int32_t)a0, (int32_t)(a1 - a0), (int32_t)(a0 + (long long)p * n_rec)};
}
