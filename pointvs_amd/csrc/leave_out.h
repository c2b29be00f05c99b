// Which rows a leave-one-atom-out copy of a ligand holds (leave_out.hip: the hits of a sweep as pose-batch slots).
// Ligand s of the table lig_ptr [S + 1] has n_s = lig_ptr[s + 1] - lig_ptr[s] atoms and owns n_s + 1 consecutive
// copies: the whole ligand first, then the ligand without atom 0, without atom 1, ... Its first copy is number
// lig_ptr[s] + s - strictly ascending in s, so a copy number is bisected for its ligand without any further table -
// and there are lig_ptr[S] + S copies in all. Copy numbers are 64-bit: first copy + slot may pass 2^31.
// No HIP header: the host compiler builds this file alone (tests/test_leave_out_plan_host.py).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define PVS_LEAVE_OUT_FN __host__ __device__ inline
#else
#define PVS_LEAVE_OUT_FN inline
#endif

// The copy's rows: row i is source row first + i + (skip >= 0 && i >= skip), i < n. A copy number outside
// [0, lig_ptr[S] + S) holds nothing.
struct PvsLeaveOutCopy {
    int32_t first;      // the ligand's first source row
    int32_t n;          // rows of the copy
    int32_t skip;       // the atom left out, counted from `first`; -1: none
};

// lig_ptr must be ascending from 0 (pvs_leave_out_table_ok of every entry).
PVS_LEAVE_OUT_FN PvsLeaveOutCopy pvs_leave_out_copy(const int32_t* lig_ptr, int S, long long copy) {
    if (S < 1 || copy < 0 || copy >= (long long)lig_ptr[S] + S) return PvsLeaveOutCopy{0, 0, -1};
    int lo = 0, hi = S;         // the last s with lig_ptr[s] + s <= copy
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long long)lig_ptr[mid] + mid <= copy) lo = mid; else hi = mid;
    }
    const int32_t first = lig_ptr[lo], n = lig_ptr[lo + 1] - first;
    const int32_t which = (int32_t)(copy - ((long long)first + lo));        // 0 .. n
    return which == 0 ? PvsLeaveOutCopy{first, n, -1} : PvsLeaveOutCopy{first, n - 1, which - 1};
}

// Entry t (0 .. S) of a table of ligands of 0..slot_cap atoms inside n_rows source rows.
PVS_LEAVE_OUT_FN bool pvs_leave_out_table_ok(const int32_t* lig_ptr, int S, int t, int slot_cap, int n_rows) {
    if (t == 0 && lig_ptr[0] != 0) return false;
    if (t == S) return lig_ptr[S] <= n_rows;
    const long long n = (long long)lig_ptr[t + 1] - lig_ptr[t];
    return n >= 0 && n <= slot_cap;
}

// ---- copies that leave out one ligand-receptor pair (pvs_leave_out_pair_pack) ----
// Hit s owns the rows pair_ptr[s] .. pair_ptr[s + 1] of a pair table [K, 2] (ligand atom a counted inside the hit or -1,
// receptor atom r or -1) and pair_ptr[s + 1] - pair_ptr[s] + 1 consecutive copies: the whole ligand first, then one per
// row of its table. Its first copy is number pair_ptr[s] + s: the arithmetic above with pair_ptr in the place of
// lig_ptr, and pair_ptr[S] + S copies in all.
struct PvsPairCopy {
    int32_t hit;        // -1: a copy number outside [0, pair_ptr[S] + S) holds nothing
    int32_t pair;       // the row of the pair table that the copy leaves out; -1: the whole ligand
};

// pair_ptr must be ascending from 0 (pvs_pair_table_ok of every entry).
PVS_LEAVE_OUT_FN PvsPairCopy pvs_pair_copy(const int32_t* pair_ptr, int S, long long copy) {
    if (S < 1 || copy < 0 || copy >= (long long)pair_ptr[S] + S) return PvsPairCopy{-1, -1};
    int lo = 0, hi = S;         // the last s with pair_ptr[s] + s <= copy
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long long)pair_ptr[mid] + mid <= copy) lo = mid; else hi = mid;
    }
    const int32_t which = (int32_t)(copy - ((long long)pair_ptr[lo] + lo));      // 0 .. the hit's pair count
    return PvsPairCopy{lo, which == 0 ? -1 : pair_ptr[lo] + which - 1};
}

// Entry t (0 .. S) of a table of pair rows inside K.
PVS_LEAVE_OUT_FN bool pvs_pair_table_ok(const int32_t* pair_ptr, int S, int t, int K) {
    if (t == 0 && pair_ptr[0] != 0) return false;
    if (t == S) return pair_ptr[S] <= K;
    return pair_ptr[t + 1] >= pair_ptr[t];
}

// One row (a, r) of the table of a hit of n atoms against n_rec receptor atoms.
PVS_LEAVE_OUT_FN bool pvs_pair_ok(int a, int r, int n, int n_rec) { return a >= -1 && a < n && r >= -1 && r < n_rec; }
