// Leave-one-atom-out copies of a set of ligands as the slots of a pose batch (pvs_leave_out_ligand_pack): what turns the
// hits of a sweep into LibraryScreen batches without a host loop per atom. Beside it the same for copies that leave out
// one ligand-receptor pair (pvs_leave_out_pair_pack: the struck slots of screen_graph.hip) and the lister of those
// pairs (pvs_contact_pairs_count / _fill).
#include "common.h"
#include "leave_out.h"
#include "radius_common.h"
#include "screen_slots.h"

namespace {
constexpr int kPackThreads = 256;

// One workgroup per slot. Every workgroup checks the whole table (a few KiB from L2; all come to the same verdict, so
// no workgroup waits for another), sums the sizes of the slots before its own (integer sums: any order gives the same
// bits), stores its entry of out_ptr and copies its rows. No atomics, nothing shared between workgroups.
__global__ void __launch_bounds__(kPackThreads)
k_leave_out_pack(const float* __restrict__ lig_pos, const float* __restrict__ lig_feats,
                 const int32_t* __restrict__ lig_ptr, int S, int n_rows, int F,
                 const int32_t* __restrict__ first_copy, int n_slots, int slot_cap, float* __restrict__ out_pos,
                 float* __restrict__ out_feats, int32_t* __restrict__ out_ptr, int32_t* __restrict__ status) {
    __shared__ int wave_sum[kPackThreads / PVS_WAVE];
    const int k = blockIdx.x, tid = threadIdx.x;
    const bool last = k == n_slots - 1;
    int bad = 0;
    for (int t = tid; t <= S; t += kPackThreads) bad |= !pvs_leave_out_table_ok(lig_ptr, S, t, slot_cap, n_rows);
    if (__syncthreads_or(bad)) {
        if (tid == 0) {
            out_ptr[k] = 0;
            if (last) out_ptr[n_slots] = 0;
            if (k == 0) *status = kPvsBadTable;
        }
        return;
    }
    const long long c0 = first_copy[0];
    int before = 0;
    for (int t = tid; t < k; t += kPackThreads) before += pvs_leave_out_copy(lig_ptr, S, c0 + t).n;
#pragma unroll
    for (int o = 1; o < PVS_WAVE; o <<= 1) before += __shfl_xor(before, o, PVS_WAVE);
    if (tid % PVS_WAVE == 0) wave_sum[tid / PVS_WAVE] = before;
    __syncthreads();
    int at = 0;
#pragma unroll
    for (int w = 0; w < kPackThreads / PVS_WAVE; ++w) at += wave_sum[w];
    const PvsLeaveOutCopy me = pvs_leave_out_copy(lig_ptr, S, c0 + k);
    if (tid == 0) {
        out_ptr[k] = at;
        if (last) out_ptr[n_slots] = at + me.n;
        if (k == 0) *status = 0;
    }
    // row i of the copy <- source row i, or i + 1 from the atom left out on
    const float* src_pos = lig_pos + (size_t)me.first * 3;
    float* dst_pos = out_pos + (size_t)at * 3;
    for (int e = tid; e < me.n * 3; e += kPackThreads) {
        const int i = e / 3;
        dst_pos[e] = src_pos[e + (me.skip >= 0 && i >= me.skip ? 3 : 0)];
    }
    const float* src_feats = lig_feats + (size_t)me.first * F;
    float* dst_feats = out_feats + (size_t)at * F;
    for (int e = tid; e < me.n * F; e += kPackThreads) {
        const int i = e / F;
        dst_feats[e] = src_feats[e + (me.skip >= 0 && i >= me.skip ? F : 0)];
    }
}

// The same for copies that leave out one ligand-receptor pair (leave_out.h: PvsPairCopy): one workgroup per slot, every
// workgroup checks both tables whole and the pair rows of the batch's own copies (the rows its sizes come from; a bad
// row elsewhere in the table is refused by the batch that holds its copy), sums the sizes of the slots before its own,
// stores its entries of out_ptr and rec_drop and copies its rows. No atomics, nothing shared between workgroups.
__global__ void __launch_bounds__(kPackThreads)
k_leave_out_pair_pack(const float* __restrict__ lig_pos, const float* __restrict__ lig_feats,
                      const int32_t* __restrict__ lig_ptr, const int32_t* __restrict__ pairs,
                      const int32_t* __restrict__ pair_ptr, int S, int n_rows, int K, int F, int n_rec,
                      const int32_t* __restrict__ first_copy, int n_slots, int slot_cap, float* __restrict__ out_pos,
                      float* __restrict__ out_feats, int32_t* __restrict__ out_ptr, int32_t* __restrict__ rec_drop,
                      int32_t* __restrict__ status) {
    __shared__ int wave_sum[kPackThreads / PVS_WAVE];
    const int k = blockIdx.x, tid = threadIdx.x;
    const bool last = k == n_slots - 1;
    auto refuse = [&]() {
        if (tid == 0) {
            out_ptr[k] = 0;
            rec_drop[k] = -1;
            if (last) out_ptr[n_slots] = 0;
            if (k == 0) *status = kPvsBadTable;
        }
    };
    int bad = 0;
    for (int t = tid; t <= S; t += kPackThreads)
        bad |= !pvs_leave_out_table_ok(lig_ptr, S, t, slot_cap, n_rows) || !pvs_pair_table_ok(pair_ptr, S, t, K);
    if (__syncthreads_or(bad)) { refuse(); return; }
    // the batch's copies: their pair rows checked, the sizes of those before this slot summed
    const long long c0 = first_copy[0];
    int before = 0;
    for (int t = tid; t < n_slots; t += kPackThreads) {
        const PvsPairCopy c = pvs_pair_copy(pair_ptr, S, c0 + t);
        if (c.hit < 0) continue;
        int n = lig_ptr[c.hit + 1] - lig_ptr[c.hit];
        if (c.pair >= 0) {
            const int a = pairs[2 * (size_t)c.pair], r = pairs[2 * (size_t)c.pair + 1];
            bad |= !pvs_pair_ok(a, r, n, n_rec);
            n -= a >= 0 ? 1 : 0;
        }
        if (t < k) before += n;
    }
    if (__syncthreads_or(bad)) { refuse(); return; }
#pragma unroll
    for (int o = 1; o < PVS_WAVE; o <<= 1) before += __shfl_xor(before, o, PVS_WAVE);
    if (tid % PVS_WAVE == 0) wave_sum[tid / PVS_WAVE] = before;
    __syncthreads();
    int at = 0;
#pragma unroll
    for (int w = 0; w < kPackThreads / PVS_WAVE; ++w) at += wave_sum[w];
    const PvsPairCopy me = pvs_pair_copy(pair_ptr, S, c0 + k);
    int first = 0, n = 0, skip = -1, drop = -1;
    if (me.hit >= 0) {
        first = lig_ptr[me.hit];
        n = lig_ptr[me.hit + 1] - first;
        if (me.pair >= 0) {
            skip = pairs[2 * (size_t)me.pair];
            drop = pairs[2 * (size_t)me.pair + 1];
            n -= skip >= 0 ? 1 : 0;
        }
    }
    if (tid == 0) {
        out_ptr[k] = at;
        rec_drop[k] = drop;
        if (last) out_ptr[n_slots] = at + n;
        if (k == 0) *status = 0;
    }
    // row i of the copy <- source row i, or i + 1 from the atom left out on
    const float* src_pos = lig_pos + (size_t)first * 3;
    float* dst_pos = out_pos + (size_t)at * 3;
    for (int e = tid; e < n * 3; e += kPackThreads) {
        const int i = e / 3;
        dst_pos[e] = src_pos[e + (skip >= 0 && i >= skip ? 3 : 0)];
    }
    const float* src_feats = lig_feats + (size_t)first * F;
    float* dst_feats = out_feats + (size_t)at * F;
    for (int e = tid; e < n * F; e += kPackThreads) {
        const int i = e / F;
        dst_feats[e] = src_feats[e + (skip >= 0 && i >= skip ? F : 0)];
    }
}

// The PARENTS of a leave-out batch's copies (what a cropped copy is cropped around): slot k <- the whole hit that owns
// copy first_copy + k in the numbering of copy_ptr (lig_ptr for ligand-atom copies, pair_ptr for pair copies: hit s owns
// copy_ptr[s] + s ..; pvs_pair_copy's bisection is that arithmetic). One workgroup per slot, as the packers above: every
// workgroup checks both tables whole, sums the parents' sizes of the slots before its own, stores its entry of out_ptr
// and copies its rows. No atomics, nothing shared between workgroups.
__global__ void __launch_bounds__(kPackThreads)
k_leave_out_parent_pack(const float* __restrict__ lig_pos, const int32_t* __restrict__ lig_ptr,
                        const int32_t* __restrict__ copy_ptr, int S, int n_rows,
                        const int32_t* __restrict__ first_copy, int n_slots, int slot_cap,
                        float* __restrict__ out_pos, int32_t* __restrict__ out_ptr, int32_t* __restrict__ status) {
    __shared__ int wave_sum[kPackThreads / PVS_WAVE];
    const int k = blockIdx.x, tid = threadIdx.x;
    const bool last = k == n_slots - 1;
    int bad = 0;
    for (int t = tid; t <= S; t += kPackThreads)
        bad |= !pvs_leave_out_table_ok(lig_ptr, S, t, slot_cap, n_rows) || !pvs_pair_table_ok(copy_ptr, S, t, INT32_MAX);
    if (__syncthreads_or(bad)) {
        if (tid == 0) {
            out_ptr[k] = 0;
            if (last) out_ptr[n_slots] = 0;
            if (k == 0) *status = kPvsBadTable;
        }
        return;
    }
    const long long c0 = first_copy[0];
    auto parent_atoms = [&](long long copy) {
        const int hit = pvs_pair_copy(copy_ptr, S, copy).hit;
        return hit < 0 ? 0 : lig_ptr[hit + 1] - lig_ptr[hit];
    };
    int before = 0;
    for (int t = tid; t < k; t += kPackThreads) before += parent_atoms(c0 + t);
#pragma unroll
    for (int o = 1; o < PVS_WAVE; o <<= 1) before += __shfl_xor(before, o, PVS_WAVE);
    if (tid % PVS_WAVE == 0) wave_sum[tid / PVS_WAVE] = before;
    __syncthreads();
    int at = 0;
#pragma unroll
    for (int w = 0; w < kPackThreads / PVS_WAVE; ++w) at += wave_sum[w];
    const int hit = pvs_pair_copy(copy_ptr, S, c0 + k).hit;
    const int first = hit < 0 ? 0 : lig_ptr[hit], n = hit < 0 ? 0 : lig_ptr[hit + 1] - first;
    if (tid == 0) {
        out_ptr[k] = at;
        if (last) out_ptr[n_slots] = at + n;
        if (k == 0) *status = 0;
    }
    const float* src = lig_pos + (size_t)first * 3;
    float* dst = out_pos + (size_t)at * 3;
    for (int e = tid; e < n * 3; e += kPackThreads) dst[e] = src[e];
}

// ---- the contacts of packed hits with the receptor: the pairs the pose-batch builder gives a class-1 edge ----
// Wave per hit; atom by atom and 64 receptor atoms per trip, so a ballot's set bits are the atom's contacts in
// ascending receptor order and the hit's pairs come out sorted by (a, r). fp64 distances and compares as k_contacts.
template <class Sink>
__device__ __forceinline__ int hit_contacts(const float* __restrict__ lig_pos, int a0, int n, const float* __restrict__
                                            rec_pos, int n_rec, Radius r_inter, Radius r_zero, int lane, Sink sink) {
    int count = 0;
    const unsigned long long lower = (1ull << lane) - 1ull;
    for (int a = 0; a < n; ++a) {
        const float* la = lig_pos + (size_t)(a0 + a) * 3;
        const double xa = la[0], ya = la[1], za = la[2];
        for (int c = 0; c < n_rec; c += 64) {
            const int i = c + lane;
            bool on = false;
            if (i < n_rec) {
                const double s = pvs_sqdist(xa, ya, za, (double)rec_pos[3 * i], (double)rec_pos[3 * i + 1],
                                            (double)rec_pos[3 * i + 2]);
                on = above(s, r_zero) && below(s, r_inter);
            }
            const unsigned long long b = __ballot(on);
            if (on) sink(count + __popcll(b & lower), a, i);
            count += __popcll(b);
        }
    }
    return count;
}

__device__ __forceinline__ bool hit_ok(const int32_t* __restrict__ lig_ptr, int s, int n_rows) {
    const int a0 = lig_ptr[s], a1 = lig_ptr[s + 1];
    return a0 >= 0 && a1 >= a0 && a1 <= n_rows;
}

// counts[s] of every hit (0 for a hit whose lig_ptr entries are no range of rows)
__global__ void __launch_bounds__(256)
k_contact_count(const float* __restrict__ lig_pos, const int32_t* __restrict__ lig_ptr, int S, int n_rows,
                const float* __restrict__ rec_pos, int n_rec, Radius r_inter, Radius r_zero,
                int32_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int s = (blockIdx.x * 256 + threadIdx.x) >> 6;
    if (s >= S) return;
    int n = 0;
    if (hit_ok(lig_ptr, s, n_rows))
        n = hit_contacts(lig_pos, lig_ptr[s], lig_ptr[s + 1] - lig_ptr[s], rec_pos, n_rec, r_inter, r_zero, lane,
                         [](int, int, int) {});
    if (lane == 0) counts[s] = n;
}

// One workgroup: pair_ptr [S + 1] <- the exclusive scan of the counts it holds in [0, S), in place (thread t owns a
// contiguous run of entries). A lig_ptr that is no ascending table from 0 inside n_rows: zeros and pair_ptr[S] = -1.
__global__ void __launch_bounds__(256)
k_contact_scan(const int32_t* __restrict__ lig_ptr, int S, int n_rows, int32_t* __restrict__ pair_ptr) {
    __shared__ long long part[256];
    const int tid = threadIdx.x, per = (S + 255) / 256;
    const int lo = min(S, tid * per), hi = min(S, lo + per);
    int bad = tid == 0 && lig_ptr[0] != 0;
    long long sum = 0;
    for (int s = lo; s < hi; ++s) {
        bad |= !hit_ok(lig_ptr, s, n_rows);
        sum += pair_ptr[s];
    }
    part[tid] = sum;
    bad = __syncthreads_or(bad);
    long long at = 0, total = 0;
    for (int t = 0; t < 256; ++t) {
        if (t < tid) at += part[t];
        total += part[t];
    }
    bad = bad || total > 0x7fffffffll;
    for (int s = lo; s < hi; ++s) {
        const int n = pair_ptr[s];
        pair_ptr[s] = bad ? 0 : (int32_t)at;
        at += n;
    }
    if (tid == 0) pair_ptr[S] = bad ? -1 : (int32_t)total;
}

__global__ void __launch_bounds__(256)
k_contact_fill(const float* __restrict__ lig_pos, const int32_t* __restrict__ lig_ptr, int S, int n_rows,
               const float* __restrict__ rec_pos, int n_rec, Radius r_inter, Radius r_zero,
               const int32_t* __restrict__ pair_ptr, int K, int32_t* __restrict__ pairs) {
    const int lane = threadIdx.x & 63;
    const int s = (blockIdx.x * 256 + threadIdx.x) >> 6;
    if (s >= S || pair_ptr[S] < 0 || !hit_ok(lig_ptr, s, n_rows)) return;
    const int p0 = pair_ptr[s], room = min(pair_ptr[s + 1], K) - p0;      // (never past the hit's own rows, nor past K)
    if (p0 < 0 || room <= 0) return;
    hit_contacts(lig_pos, lig_ptr[s], lig_ptr[s + 1] - lig_ptr[s], rec_pos, n_rec, r_inter, r_zero, lane,
                 [&](int k, int a, int r) {
                     if (k < room) { pairs[2 * (size_t)(p0 + k)] = a; pairs[2 * (size_t)(p0 + k) + 1] = r; }
                 });
}
}  // namespace

extern "C" int pvs_contact_pairs_count(const float* lig_pos, const int32_t* lig_ptr, int32_t n_hits, int32_t n_rows,
                                       const float* rec_pos, int32_t n_rec, double inter_radius, int32_t* pair_ptr,
                                       pvs_stream_t stream) {
    PVS_REQUIRE(n_hits >= 0 && n_rows >= 0 && n_rec >= 1, "contact_pairs_count: %d hits, %d rows, %d receptor atoms",
                n_hits, n_rows, n_rec);
    PVS_REQUIRE(lig_ptr && rec_pos && pair_ptr && (n_rows == 0 || lig_pos), "contact_pairs_count: NULL argument");
    hipStream_t s = (hipStream_t)stream;
    if (n_hits > 0) {
        k_contact_count<<<(n_hits + 3) / 4, 256, 0, s>>>(lig_pos, lig_ptr, n_hits, n_rows, rec_pos, n_rec,
                                                         make_radius(inter_radius), make_radius(1e-7), pair_ptr);
        PVS_CHECK_LAUNCH();
    }
    k_contact_scan<<<1, 256, 0, s>>>(lig_ptr, n_hits, n_rows, pair_ptr);
    PVS_CHECK_LAUNCH();
    return 0;
}

extern "C" int pvs_contact_pairs_fill(const float* lig_pos, const int32_t* lig_ptr, int32_t n_hits, int32_t n_rows,
                                      const float* rec_pos, int32_t n_rec, double inter_radius,
                                      const int32_t* pair_ptr, int32_t n_pairs, int32_t* pairs, pvs_stream_t stream) {
    PVS_REQUIRE(n_hits >= 0 && n_rows >= 0 && n_rec >= 1 && n_pairs >= 0,
                "contact_pairs_fill: %d hits, %d rows, %d receptor atoms, %d pairs", n_hits, n_rows, n_rec, n_pairs);
    PVS_REQUIRE(lig_ptr && rec_pos && pair_ptr && (n_rows == 0 || lig_pos) && (n_pairs == 0 || pairs),
                "contact_pairs_fill: NULL argument");
    if (n_hits == 0 || n_pairs == 0) return 0;
    k_contact_fill<<<(n_hits + 3) / 4, 256, 0, (hipStream_t)stream>>>(lig_pos, lig_ptr, n_hits, n_rows, rec_pos, n_rec,
                                                                      make_radius(inter_radius), make_radius(1e-7),
                                                                      pair_ptr, n_pairs, pairs);
    PVS_CHECK_LAUNCH();
    return 0;
}

extern "C" int pvs_leave_out_pair_pack(const float* lig_pos, const float* lig_feats, const int32_t* lig_ptr,
                                       const int32_t* pairs, const int32_t* pair_ptr, int32_t n_hits, int32_t n_rows,
                                       int32_t n_pairs, int32_t n_feats, int32_t n_rec, const int32_t* first_copy,
                                       int32_t n_slots, int32_t slot_cap, float* out_pos, float* out_feats,
                                       int32_t* out_ptr, int32_t* rec_drop, int32_t* status, pvs_stream_t stream) {
    PVS_REQUIRE(n_hits >= 0 && n_rows >= 0 && n_pairs >= 0 && n_feats >= 1 && n_rec >= 1,
                "leave_out_pair_pack: %d hits, %d rows, %d pairs, %d features, %d receptor atoms", n_hits, n_rows,
                n_pairs, n_feats, n_rec);
    PVS_REQUIRE(n_slots >= 1 && slot_cap >= 1 && slot_cap <= kPvsMaxSlotCap,
                "leave_out_pair_pack: %d slots of up to %d atoms (1..%d)", n_slots, slot_cap, kPvsMaxSlotCap);
    PVS_REQUIRE((long long)n_slots * slot_cap * n_feats < (1ll << 31) && (long long)n_pairs + n_hits < (1ll << 31),
                "leave_out_pair_pack: %d slots x %d atoms x %d features, or %d pairs + %d hits, pass 2^31", n_slots,
                slot_cap, n_feats, n_pairs, n_hits);
    PVS_REQUIRE(lig_ptr && pair_ptr && first_copy && out_pos && out_feats && out_ptr && rec_drop && status &&
                (n_rows == 0 || (lig_pos && lig_feats)) && (n_pairs == 0 || pairs), "leave_out_pair_pack: NULL argument");
    k_leave_out_pair_pack<<<n_slots, kPackThreads, 0, (hipStream_t)stream>>>(
        lig_pos, lig_feats, lig_ptr, pairs, pair_ptr, n_hits, n_rows, n_pairs, n_feats, n_rec, first_copy, n_slots,
        slot_cap, out_pos, out_feats, out_ptr, rec_drop, status);
    PVS_CHECK_LAUNCH();
    return 0;
}

extern "C" int pvs_leave_out_ligand_pack(const float* lig_pos, const float* lig_feats, const int32_t* lig_ptr,
                                         int32_t n_ligands, int32_t n_rows, int32_t n_feats,
                                         const int32_t* first_copy, int32_t n_slots, int32_t slot_cap, float* out_pos,
                                         float* out_feats, int32_t* out_ptr, int32_t* status, pvs_stream_t stream) {
    PVS_REQUIRE(n_ligands >= 0 && n_rows >= 0 && n_feats >= 1, "leave_out_ligand_pack: %d ligands, %d rows, %d features",
                n_ligands, n_rows, n_feats);
    PVS_REQUIRE(n_slots >= 1 && slot_cap >= 1 && slot_cap <= kPvsMaxSlotCap,
                "leave_out_ligand_pack: %d slots of up to %d atoms (1..%d)", n_slots, slot_cap, kPvsMaxSlotCap);
    PVS_REQUIRE((long long)n_slots * slot_cap * n_feats < (1ll << 31) && (long long)n_rows + n_ligands < (1ll << 31),
                "leave_out_ligand_pack: %d slots x %d atoms x %d features, or %d rows + %d ligands, pass 2^31", n_slots,
                slot_cap, n_feats, n_rows, n_ligands);
    PVS_REQUIRE(lig_ptr && first_copy && out_pos && out_feats && out_ptr && status && (n_rows == 0 || (lig_pos && lig_feats)),
                "leave_out_ligand_pack: NULL argument");
    k_leave_out_pack<<<n_slots, kPackThreads, 0, (hipStream_t)stream>>>(lig_pos, lig_feats, lig_ptr, n_ligands, n_rows,
                                                                        n_feats, first_copy, n_slots, slot_cap, out_pos,
                                                                        out_feats, out_ptr, status);
    PVS_CHECK_LAUNCH();
    return 0;
}

extern "C" int pvs_leave_out_parent_pack(const float* lig_pos, const int32_t* lig_ptr, const int32_t* copy_ptr,
                                         int32_t n_hits, int32_t n_rows, const int32_t* first_copy, int32_t n_slots,
                                         int32_t slot_cap, float* out_pos, int32_t* out_ptr, int32_t* status,
                                         pvs_stream_t stream) {
    PVS_REQUIRE(n_hits >= 0 && n_rows >= 0, "leave_out_parent_pack: %d hits, %d rows", n_hits, n_rows);
    PVS_REQUIRE(n_slots >= 1 && slot_cap >= 1 && slot_cap <= kPvsMaxSlotCap,
                "leave_out_parent_pack: %d slots of up to %d atoms (1..%d)", n_slots, slot_cap, kPvsMaxSlotCap);
    PVS_REQUIRE((long long)n_slots * slot_cap * 3 < (1ll << 31), "leave_out_parent_pack: %d slots x %d atoms pass 2^31",
                n_slots, slot_cap);
    PVS_REQUIRE(lig_ptr && copy_ptr && first_copy && out_pos && out_ptr && status && (n_rows == 0 || lig_pos),
                "leave_out_parent_pack: NULL argument");
    k_leave_out_parent_pack<<<n_slots, kPackThreads, 0, (hipStream_t)stream>>>(
        lig_pos, lig_ptr, copy_ptr, n_hits, n_rows, first_copy, n_slots, slot_cap, out_pos, out_ptr, status);
    PVS_CHECK_LAUNCH();
    return 0;
}
