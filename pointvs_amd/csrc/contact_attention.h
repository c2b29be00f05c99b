// The order relation of the contact-attention reduction (contact_attention.hip: pvs_contact_attention) and which
// slots of a pose batch - uncropped, and cropped through keep masks - it accepts. The larger value wins, a NaN never does, equal values are one value and +0.0
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

// ---- cropped slots (PVS_SLOTS_CROPPED): behind its ligand atoms slot p has the receptor atoms whose bit is set in its
// keep mask - ceil(n_rec / 64) words, atom j is bit j % 64 of word j / 64 - in receptor order, compact: atom j is row
// node_ptr[p] + n_lig + (the set bits below j).

// The bits of word k of a mask over n_rec atoms that stand for no atom (at or beyond n_rec).
PVS_CONTACT_FN uint64_t pvs_keep_stray_bits(uint64_t word, long long k, int n_rec) {
    const long long first = k * 64;
    if (first + 64 <= n_rec) return 0;
    if (first >= n_rec) return word;
    return word & ~((1ull << (n_rec - first)) - 1);
}

// Slot p of a cropped batch, given what its mask holds: `kept` set bits, `stray` whether one of them stands for no atom.
// n < 0: no slot - the ligand table descends or has more than 1024 atoms, the rows lie outside [0, n_nodes), or there
// are not exactly n_lig + kept of them.
PVS_CONTACT_FN PvsContactSlot pvs_cropped_slot(const int32_t* node_ptr, const int32_t* lig_ptr, int p, int n_nodes,
                                               long long kept, bool stray) {
    const long long a0 = lig_ptr[p], a1 = lig_ptr[p + 1], r0 = node_ptr[p], r1 = node_ptr[p + 1];
    const bool ok = a0 >= 0 && a1 >= a0 && a1 - a0 <= kPvsContactMaxLigand && r0 >= 0 && r1 <= n_nodes &&
                    r1 - r0 == (a1 - a0) + kept && !stray;
    if (!ok) return PvsContactSlot{0, -1, 0};
    return PvsContactSlot{(int32_t)a0, (int32_t)(a1 - a0), (int32_t)r0};
}

// The same from the mask itself, one word after the other (keep: [n_slots, ceil(n_rec / 64)]); the kernels count the
// words of a slot with the lanes of a wavefront and hand the counts to pvs_cropped_slot.
PVS_CONTACT_FN PvsContactSlot pvs_cropped_slot_of(const int32_t* node_ptr, const int32_t* lig_ptr, const uint64_t* keep,
                                                  int p, int n_rec, int n_nodes) {
    const long long n_words = ((long long)n_rec + 63) / 64;
    long long kept = 0;
    bool stray = false;
    for (long long k = 0; k < n_words; ++k) {
        const uint64_t word = keep[p * n_words + k];
        kept += __builtin_popcountll(word);
        stray = stray || pvs_keep_stray_bits(word, k, n_rec) != 0;
    }
    return pvs_cropped_slot(node_ptr, lig_ptr, p, n_nodes, kept, stray);
}
