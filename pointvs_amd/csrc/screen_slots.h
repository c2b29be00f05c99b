// Where the slots of a pose batch live (screen_graph.hip), and the table bisection the graph builders share.
// A slot holds one pose: its ligand atoms, then the receptor's n_rec atoms (struck slots: all but one of them; cropped
// slots, at the end of this file: any subset of them). The layouts answer the same questions
// (how many packed ligand atoms and node rows there are; which slot a packed atom or a row belongs to), so that the
// builder's kernels exist once: uniform (B poses of one n_lig-atom ligand, by arithmetic) and ragged (one pose of any
// ligand of 0..slot_cap atoms per slot, from the device tables lig_ptr / node_ptr / slot_of). A ligand atom's contacts
// with the other atoms of its slot are a bit mask of words() 64-bit words (atom k of the slot: bit k % 64 of word
// k / 64); the word and bit arithmetic of those masks lives here too. No HIP header: the host compiler builds this
// file alone (tests/test_screen_slots_host.py, tests/test_screen_words_host.py).
#pragma once
#include <stddef.h>
#include <stdint.h>

#ifdef __HIPCC__
#define PVS_SLOTS_FN __host__ __device__ inline
#else
#define PVS_SLOTS_FN inline
#endif

// The last k in [0, n) with table[k] <= i, for an ascending table with table[0] <= i (0 otherwise; of equal entries
// the last one wins, so empty slots / graphs never own a row).
PVS_SLOTS_FN int pvs_last_le(const int32_t* table, int n, int i) {
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (table[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

constexpr int kPvsBadTable = 8;     // *status bit 3: lig_ptr is not a table of 0..slot_cap-atom slots inside L_cap
constexpr int kPvsMaxSlotCap = 1024;        // the most ligand atoms a slot holds: 16 mask words

// Ligand-side masks: how many 64-bit words hold one bit per atom of a slot of up to `cap` atoms, and where the slot's
// k-th atom has its bit.
PVS_SLOTS_FN int pvs_slot_words(int cap) { return (cap + 63) >> 6; }
PVS_SLOTS_FN int pvs_slot_word(int k) { return k >> 6; }
PVS_SLOTS_FN int pvs_slot_bit(int k) { return k & 63; }

// The number of set bits of the multi-word mask m before bit `bit` (0..63) of word `word`: where the wave's lane `bit`
// of trip `word` writes its entry when every set bit of m becomes one entry, ascending (k_fill).
PVS_SLOTS_FN int pvs_mask_rank(const unsigned long long* m, int word, int bit) {
    int rank = 0;
    for (int w = 0; w < word; ++w) rank += __builtin_popcountll(m[w]);
    return rank + __builtin_popcountll(m[word] & ((1ull << bit) - 1ull));
}

// What a layout says about a packed ligand atom or a node row. Not valid: the other fields are zero (a row's slot: -1).
struct PvsSlotAtom {
    bool valid;
    int a0, n_lig;                  // the slot's first packed atom and its atom count
};
struct PvsSlotRow {
    bool valid;
    int slot, a0, n_lig;
    int node0, local;               // the slot's first row; this row inside the slot (< n_lig: ligand atom, else receptor)
    int drop = -1;                  // the receptor atom that the slot's receptor lacks (PvsStruckSlots); -1: none
};

// B poses of one ligand: slot p owns the atoms p * n_lig .. and the rows p * (n_lig + n_rec) ..; every row is valid.
struct PvsUniformSlots {
    int B, n_lig, n_rec;
    PVS_SLOTS_FN int words() const { return pvs_slot_words(n_lig); }
    PVS_SLOTS_FN int atoms() const { return B * n_lig; }
    PVS_SLOTS_FN int rows() const { return B * (n_lig + n_rec); }
    PVS_SLOTS_FN PvsSlotAtom atom(int q) const { return {true, q / n_lig * n_lig, n_lig}; }
    PVS_SLOTS_FN PvsSlotRow row(int g) const {
        const int n = n_lig + n_rec, p = g / n;
        return {true, p, p * n_lig, n_lig, p * n, g - p * n};
    }
};

// One pose of any ligand per slot: slot p owns the atoms lig_ptr[p] .. lig_ptr[p+1] and the rows node_ptr[p] ..
// node_ptr[p+1] (node_ptr[p] = lig_ptr[p] + p * n_rec). Not valid: the atoms from lig_ptr[B], the rows from
// node_ptr[B] (padding up to L_cap / L_cap + B * n_rec), and everything while *status has kPvsBadTable. slot_cap: the
// most atoms a slot of a valid table holds (k_slots checks it).
struct PvsRaggedSlots {
    const int32_t *lig_ptr, *node_ptr, *slot_of, *status;
    int B, L_cap, n_rec;
    int slot_cap = 64;
    PVS_SLOTS_FN int words() const { return pvs_slot_words(slot_cap); }
    PVS_SLOTS_FN int atoms() const { return L_cap; }
    PVS_SLOTS_FN int rows() const { return L_cap + B * n_rec; }
    PVS_SLOTS_FN PvsSlotAtom atom(int q) const {
        if ((*status & kPvsBadTable) || q >= lig_ptr[B]) return {false, 0, 0};
        const int p = slot_of[q], a0 = lig_ptr[p];
        return {true, a0, lig_ptr[p + 1] - a0};
    }
    PVS_SLOTS_FN PvsSlotRow row(int g) const {
        if (g >= node_ptr[B] || (*status & kPvsBadTable)) return {false, -1, 0, 0, 0, 0};
        const int p = pvs_last_le(node_ptr, B, g), a0 = lig_ptr[p], node0 = node_ptr[p];
        return {true, p, a0, lig_ptr[p + 1] - a0, node0, g - node0};
    }
};

// ---- struck slots: a slot's receptor may lack one atom (rec_drop[p] = r in 0..n_rec-1; -1: the whole receptor) ----
// The receptor atoms of a struck slot keep their order with r left out, so the slot owns n_lig + n_rec - 1 rows and
// node_ptr[p] = lig_ptr[p] + p * n_rec - (struck slots before p). A row's `local` counts the slot's rows as they are
// (compact); pvs_struck_receptor turns the receptor part of it back into the receptor's own numbering.

// A valid entry of rec_drop.
PVS_SLOTS_FN bool pvs_rec_drop_ok(int drop, int n_rec) { return drop >= -1 && drop < n_rec; }

// The receptor atom behind the k-th receptor row of a slot without atom `drop`, and the row of receptor atom i (i !=
// drop) in such a slot.
PVS_SLOTS_FN int pvs_struck_receptor(int k, int drop) { return k + ((drop >= 0 && k >= drop) ? 1 : 0); }
PVS_SLOTS_FN int pvs_struck_row(int i, int drop) { return i - ((drop >= 0 && i > drop) ? 1 : 0); }

// Where `v` stands in the ascending row col[0 .. n); -1 when it is not there (a receptor row of the template CSR: is
// the struck atom one of its neighbours, and at which place).
PVS_SLOTS_FN int pvs_find_ascending(const int32_t* col, int n, int v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[mid] < v) lo = mid + 1; else hi = mid;
    }
    return (lo < n && col[lo] == v) ? lo : -1;
}

// The ragged layout with rec_drop [B]: the same questions, and per row the atom its slot lacks. Not valid: as for
// PvsRaggedSlots (kPvsBadTable also stands for a rec_drop entry outside -1..n_rec-1; k_slots_struck checks it).
struct PvsStruckSlots {
    const int32_t *lig_ptr, *node_ptr, *slot_of, *status, *rec_drop;
    int B, L_cap, n_rec;
    int slot_cap = 64;
    PVS_SLOTS_FN int words() const { return pvs_slot_words(slot_cap); }
    PVS_SLOTS_FN int atoms() const { return L_cap; }
    PVS_SLOTS_FN int rows() const { return L_cap + B * n_rec; }
    PVS_SLOTS_FN PvsSlotAtom atom(int q) const {
        if ((*status & kPvsBadTable) || q >= lig_ptr[B]) return {false, 0, 0};
        const int p = slot_of[q], a0 = lig_ptr[p];
        return {true, a0, lig_ptr[p + 1] - a0};
    }
    PVS_SLOTS_FN int drop_of_atom(int q) const { return rec_drop[slot_of[q]]; }       // (of a valid atom)
    PVS_SLOTS_FN PvsSlotRow row(int g) const {
        if (g >= node_ptr[B] || (*status & kPvsBadTable)) return {false, -1, 0, 0, 0, 0};
        const int p = pvs_last_le(node_ptr, B, g), a0 = lig_ptr[p], node0 = node_ptr[p];
        return {true, p, a0, lig_ptr[p + 1] - a0, node0, g - node0, rec_drop[p]};
    }
};

// ---- cropped slots: a slot's receptor is the subset of the receptor's atoms that a keep mask names ----
// keep [B, W] 64-bit words, W = pvs_rec_words(n_rec): bit j % 64 of word j / 64 of slot p is set when receptor atom j is
// one of the slot's rows (the bits from n_rec on are clear). The kept atoms keep their order, compact, behind the slot's
// ligand atoms, so the slot owns n_lig + kept rows and node_ptr[p + 1] = node_ptr[p] + n_lig_p + kept_p. keep_rank
// [B, W + 1]: per slot the kept atoms in the words before word w (entry W: the slot's kept count), which makes both
// mappings between receptor rows and receptor atoms one table read and one word of bit arithmetic.

PVS_SLOTS_FN int pvs_rec_words(int n_rec) { return (n_rec + 63) >> 6; }

// The place of the n-th set bit of `word`, n = 0 .. popcount(word) - 1 (six halvings).
PVS_SLOTS_FN int pvs_select64(unsigned long long word, int n) {
    int at = 0;
    for (int width = 32; width; width >>= 1) {
        const int c = __builtin_popcountll((word >> at) & ((1ull << width) - 1ull));
        if (n >= c) { n -= c; at += width; }
    }
    return at;
}

// The ragged layout with keep / keep_rank: the same questions (a row's `local` counts the slot's rows as they are,
// compact), and the two mappings of a slot's receptor part. Not valid: as for PvsRaggedSlots.
struct PvsCroppedSlots {
    const int32_t *lig_ptr, *node_ptr, *slot_of, *status;
    const unsigned long long* keep;
    const int32_t* keep_rank;
    int B, L_cap, n_rec;
    int slot_cap = 64;
    PVS_SLOTS_FN int words() const { return pvs_slot_words(slot_cap); }
    PVS_SLOTS_FN int rec_words() const { return pvs_rec_words(n_rec); }
    PVS_SLOTS_FN int atoms() const { return L_cap; }
    PVS_SLOTS_FN int rows() const { return L_cap + B * n_rec; }       // (the room: a slot that keeps every atom)
    PVS_SLOTS_FN PvsSlotAtom atom(int q) const {
        if ((*status & kPvsBadTable) || q >= lig_ptr[B]) return {false, 0, 0};
        const int p = slot_of[q], a0 = lig_ptr[p];
        return {true, a0, lig_ptr[p + 1] - a0};
    }
    PVS_SLOTS_FN PvsSlotRow row(int g) const {
        if (g >= node_ptr[B] || (*status & kPvsBadTable)) return {false, -1, 0, 0, 0, 0};
        const int p = pvs_last_le(node_ptr, B, g), a0 = lig_ptr[p], node0 = node_ptr[p];
        return {true, p, a0, lig_ptr[p + 1] - a0, node0, g - node0};
    }
    // word c of the keep mask of the slot that owns the (valid) packed atom q
    PVS_SLOTS_FN unsigned long long keep_word_of_atom(int q, int c) const {
        return keep[(size_t)slot_of[q] * rec_words() + c];
    }
    PVS_SLOTS_FN bool kept(int p, int j) const { return (keep[(size_t)p * rec_words() + (j >> 6)] >> (j & 63)) & 1ull; }
    PVS_SLOTS_FN int kept_count(int p) const { return keep_rank[(size_t)p * (rec_words() + 1) + rec_words()]; }
    // select: the receptor atom behind the k-th receptor row of slot p, k = 0 .. kept_count(p) - 1 (of words with
    // equal ranks the last one wins: the one that is not empty)
    PVS_SLOTS_FN int receptor(int p, int k) const {
        const int W = rec_words();
        const int32_t* rank = keep_rank + (size_t)p * (W + 1);
        const int w = pvs_last_le(rank, W, k);
        return 64 * w + pvs_select64(keep[(size_t)p * W + w], k - rank[w]);
    }
    // rank: the receptor row (0 .. kept_count(p) - 1) of the kept receptor atom j in slot p; for an atom that is not
    // kept, the row the next kept atom has
    PVS_SLOTS_FN int receptor_row(int p, int j) const {
        const int W = rec_words(), w = j >> 6;
        return keep_rank[(size_t)p * (W + 1) + w] +
               __builtin_popcountll(keep[(size_t)p * W + w] & ((1ull << (j & 63)) - 1ull));
    }
};
