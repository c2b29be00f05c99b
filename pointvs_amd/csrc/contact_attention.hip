// Contact attention of a pose batch (pvs_contact_attention): per atom the largest attention value over its
// ligand-receptor edges, per receptor atom the sum / count / maximum of these over the slots, kept on the device across
// the steps of a sweep (screening.py: LibraryScreen(contact_attention=...), ScreeningSweep.receptor_hotspots).
// The same reduction over a value every node has (pvs_slot_node_values: a column of the per-node heads, the
// class-activation map of LibraryScreen(cam=...)): other per-slot values, the one accumulation kernel.
#include <math.h>
#include "common.h"
#include "contact_attention.h"

namespace {
constexpr int kRowThreads = 256;
constexpr int kRecLanes = 16;           // lanes that share a receptor row (few ligand contacts; in the full CSR a few hundred edges)
constexpr int kLigBlocksPerSlot = 4;    // workgroups whose wavefronts stride over the ligand rows of one slot
constexpr int kLigWavesPerSlot = kLigBlocksPerSlot * kRowThreads / PVS_WAVE;

// The row's maximum over its class-1 edges in every one of the LANES consecutive lanes that share the row (lane: this
// lane's place among them). All LANES lanes must be here together. Edge ranges are clamped to the arrays.
// range_contact_max: the same over the edges [e0, e1) of a row that the caller has clamped (e0 == e1: NaN).
template <int LANES>
__device__ __forceinline__ float range_contact_max(const uint8_t* __restrict__ etype, const float* __restrict__ att,
                                                   int e0, int e1, int lane) {
    float cur = NAN;
    for (int k = lane; k < e1 - e0; k += LANES)
        if (etype[e0 + k] == 1) cur = pvs_contact_max(cur, att[e0 + k]);
#pragma unroll
    for (int o = 1; o < LANES; o <<= 1) cur = pvs_contact_max(cur, __shfl_xor(cur, o, PVS_WAVE));
    return cur;
}

template <int LANES>
__device__ __forceinline__ float row_contact_max(const int32_t* __restrict__ rowptr, const uint8_t* __restrict__ etype,
                                                 const float* __restrict__ att, int n_edges, int row, int lane) {
    return range_contact_max<LANES>(etype, att, max(rowptr[row], 0), min(rowptr[row + 1], n_edges), lane);
}

// The first rec_blocks workgroups: kRecLanes lanes per (slot, receptor atom), in that order. The workgroups behind
// them: kLigBlocksPerSlot per slot, one wavefront per ligand row, striding over the slot's rows (the host does not know
// how many there are). Every output element has one writer; nothing is shared between wavefronts.
__global__ void __launch_bounds__(kRowThreads)
k_contact_rows(const int32_t* __restrict__ rowptr, const uint8_t* __restrict__ etype, const float* __restrict__ att,
               int n_nodes, int n_edges, const int32_t* __restrict__ node_ptr, const int32_t* __restrict__ lig_ptr,
               int n_slots, int n_rec, int rec_blocks, float* __restrict__ lig_att, float* __restrict__ slot_rec_att) {
    if ((int)blockIdx.x < rec_blocks) {
        const long long idx = ((long long)blockIdx.x * kRowThreads + threadIdx.x) / kRecLanes;
        if (idx >= (long long)n_slots * n_rec) return;       // (all kRecLanes lanes of the row)
        const int p = (int)(idx / n_rec), j = (int)(idx - (long long)p * n_rec);
        const PvsContactSlot s = pvs_contact_slot(node_ptr, lig_ptr, p, n_slots, n_rec, n_nodes);
        float v = NAN;
        if (s.n >= 0) v = row_contact_max<kRecLanes>(rowptr, etype, att, n_edges, s.node0 + s.n + j, threadIdx.x % kRecLanes);
        if (threadIdx.x % kRecLanes == 0) slot_rec_att[idx] = v;
        return;
    }
    const int b = (int)blockIdx.x - rec_blocks, p = b / kLigBlocksPerSlot;
    const int wave = (b % kLigBlocksPerSlot) * (kRowThreads / PVS_WAVE) + threadIdx.x / PVS_WAVE;
    const int lane = threadIdx.x % PVS_WAVE;
    const PvsContactSlot s = pvs_contact_slot(node_ptr, lig_ptr, p, n_slots, n_rec, n_nodes);
    for (int i = wave; i < s.n; i += kLigWavesPerSlot) {      // (wave-uniform; no slot: n < 0)
        const float v = row_contact_max<PVS_WAVE>(rowptr, etype, att, n_edges, s.node0 + i, lane);
        if (lane == 0) lig_att[s.a0 + i] = v;
    }
}

// One thread per receptor atom: its slot values in slot order into the running sum / count / maximum.
__global__ void __launch_bounds__(kRowThreads)
k_contact_accumulate(const float* __restrict__ slot_rec_att, int n_slots, int n_rec, double* __restrict__ rec_sum,
                     int32_t* __restrict__ rec_count, float* __restrict__ rec_max) {
    const int j = blockIdx.x * kRowThreads + threadIdx.x;
    if (j >= n_rec) return;
    double sum = rec_sum[j];
    int32_t count = rec_count[j];
    float top = rec_max[j];
    for (int p = 0; p < n_slots; ++p) {
        const float v = slot_rec_att[(size_t)p * n_rec + j];
        if (v == v) {
            sum += (double)v;
            ++count;
        }
        top = pvs_contact_max(top, v);
    }
    rec_sum[j] = sum;
    rec_count[j] = count;
    rec_max[j] = top;
}
// The value of node row r for pvs_slot_node_values: one column of y, or the mean of three - ((a + b) + c) / 3, an IEEE
// division (hipcc's default for fp32).
__device__ __forceinline__ float node_value(const float* __restrict__ y, int ld_y, int col, int n_mean, int r) {
    const float* p = y + (size_t)r * ld_y + col;
    return n_mean == 3 ? ((p[0] + p[1]) + p[2]) / 3.0f : p[0];
}

// The first rec_blocks workgroups: one thread per (slot, receptor atom), in that order. The workgroups behind them: one
// per slot, its threads striding over the slot's ligand rows (the host does not know how many there are). A slot's rows
// lie inside the n_nodes rows of y when pvs_contact_slot accepts it. Every output element has one writer.
__global__ void __launch_bounds__(kRowThreads)
k_slot_node_values(const float* __restrict__ y, int ld_y, int col, int n_mean, int n_nodes,
                   const int32_t* __restrict__ node_ptr, const int32_t* __restrict__ lig_ptr, int n_slots, int n_rec,
                   int rec_blocks, float* __restrict__ lig_val, float* __restrict__ slot_rec_val) {
    if ((int)blockIdx.x < rec_blocks) {
        const long long idx = (long long)blockIdx.x * kRowThreads + threadIdx.x;
        if (idx >= (long long)n_slots * n_rec) return;
        const int p = (int)(idx / n_rec), j = (int)(idx - (long long)p * n_rec);
        const PvsContactSlot s = pvs_contact_slot(node_ptr, lig_ptr, p, n_slots, n_rec, n_nodes);
        slot_rec_val[idx] = s.n > 0 ? node_value(y, ld_y, col, n_mean, s.node0 + s.n + j) : NAN;
        return;
    }
    const int p = (int)blockIdx.x - rec_blocks;
    const PvsContactSlot s = pvs_contact_slot(node_ptr, lig_ptr, p, n_slots, n_rec, n_nodes);
    for (int i = threadIdx.x; i < s.n; i += kRowThreads)      // (no slot: n < 0)
        lig_val[s.a0 + i] = node_value(y, ld_y, col, n_mean, s.node0 + i);
}

// ---- cropped slots: a receptor atom's row goes through the slot's keep mask (contact_attention.h) ----

// What one wavefront learns of slot p's mask, every lane the same: the set bits in the words before word w (`below`),
// in all n_words words (`kept`), and whether a bit stands for no atom. The lanes stride over the words once; integer
// sums, so the lane order means nothing. All 64 lanes must be here together.
struct KeepCensus {
    int below, kept;
    bool stray;
};

__device__ __forceinline__ KeepCensus keep_census(const uint64_t* __restrict__ keep_row, int n_words, int n_rec, int w,
                                                  int lane) {
    int below = 0, kept = 0, stray = 0;
    for (int k = lane; k < n_words; k += PVS_WAVE) {
        const uint64_t word = keep_row[k];
        const int c = __popcll(word);
        kept += c;
        if (k < w) below += c;
        stray |= pvs_keep_stray_bits(word, k, n_rec) != 0;
    }
#pragma unroll
    for (int o = 1; o < PVS_WAVE; o <<= 1) {
        below += __shfl_xor(below, o, PVS_WAVE);
        kept += __shfl_xor(kept, o, PVS_WAVE);
        stray |= __shfl_xor(stray, o, PVS_WAVE);
    }
    return KeepCensus{below, kept, stray != 0};
}

constexpr int kWavesPerBlock = kRowThreads / PVS_WAVE;
constexpr int kRowsPerPass = PVS_WAVE / kRecLanes;      // receptor rows that one wavefront reduces at a time

// The first rec_blocks workgroups: one per (slot, mask word); in each of its wavefronts lane l is receptor atom
// 64 w + l. The KEPT atoms of the word own consecutive rows, first_row + 0 .. first_row + popcount(word) - 1, reduced
// kRowsPerPass at a time with kRecLanes lanes each: pass t is wavefront t % kWavesPerBlock's (a row's edges are a
// chain of dependent loads, so the passes of a word run side by side, not one after the other), and after a pass each
// atom lane picks the value of its own rank out of the lane group that holds it. An atom is stored by the wavefront
// that had its pass; atoms that are not kept, and every atom of a slot that is none: NaN, by wavefront 0. The
// workgroups behind them: k_contact_rows' ligand part with the cropped slot.
__global__ void __launch_bounds__(kRowThreads)
k_cropped_contact_rows(const int32_t* __restrict__ rowptr, const uint8_t* __restrict__ etype,
                       const float* __restrict__ att, int n_nodes, int n_edges, const int32_t* __restrict__ node_ptr,
                       const int32_t* __restrict__ lig_ptr, const uint64_t* __restrict__ keep, int n_slots, int n_rec,
                       int n_words, int rec_blocks, float* __restrict__ lig_att, float* __restrict__ slot_rec_att) {
    const int lane = threadIdx.x % PVS_WAVE;
    if ((int)blockIdx.x < rec_blocks) {
        const int p = (int)blockIdx.x / n_words, w = (int)blockIdx.x - p * n_words, q = threadIdx.x / PVS_WAVE;
        const uint64_t* keep_row = keep + (size_t)p * n_words;
        const KeepCensus c = keep_census(keep_row, n_words, n_rec, w, lane);
        const PvsContactSlot s = pvs_cropped_slot(node_ptr, lig_ptr, p, n_nodes, c.kept, c.stray);
        const uint64_t word = s.n >= 0 ? keep_row[w] : 0;
        const int here = __popcll(word), first_row = s.node0 + s.n + c.below;
        const bool mine = (word >> lane) & 1;
        const int rank = __popcll(word & ((1ull << lane) - 1));      // (of atom `lane` among the word's kept atoms)
        float v = NAN;
        for (int r0 = q * kRowsPerPass; r0 < here; r0 += kWavesPerBlock * kRowsPerPass) {       // (wave-uniform)
            const int r = r0 + lane / kRecLanes;
            int e0 = 0, e1 = 0;                                  // (a lane group beyond the last kept atom: no edges)
            if (r < here) e0 = max(rowptr[first_row + r], 0), e1 = min(rowptr[first_row + r + 1], n_edges);
            const float top = range_contact_max<kRecLanes>(etype, att, e0, e1, lane % kRecLanes);
            const float got = __shfl(top, (rank % kRowsPerPass) * kRecLanes, PVS_WAVE);
            if (mine && rank - r0 >= 0 && rank - r0 < kRowsPerPass) v = got;
        }
        const bool writer = mine ? (rank / kRowsPerPass) % kWavesPerBlock == q : q == 0;
        const long long j = (long long)w * PVS_WAVE + lane;
        if (writer && j < n_rec) slot_rec_att[(size_t)p * n_rec + j] = v;
        return;
    }
    const int b = (int)blockIdx.x - rec_blocks, p = b / kLigBlocksPerSlot;
    const int wave = (b % kLigBlocksPerSlot) * kWavesPerBlock + threadIdx.x / PVS_WAVE;
    const KeepCensus c = keep_census(keep + (size_t)p * n_words, n_words, n_rec, 0, lane);
    const PvsContactSlot s = pvs_cropped_slot(node_ptr, lig_ptr, p, n_nodes, c.kept, c.stray);
    for (int i = wave; i < s.n; i += kLigWavesPerSlot) {      // (wave-uniform; no slot: n < 0)
        const float v = row_contact_max<PVS_WAVE>(rowptr, etype, att, n_edges, s.node0 + i, lane);
        if (lane == 0) lig_att[s.a0 + i] = v;
    }
}

// The first rec_blocks workgroups: one wavefront per (slot, mask word), lane l is receptor atom 64 w + l: the kept
// lanes read consecutive rows of y, all lanes store 64 consecutive floats (NaN for an atom that is not kept, for a slot
// without ligand atoms and for one that is none). The workgroups behind them: k_slot_node_values' ligand part with the
// cropped slot. Every output element has one writer.
__global__ void __launch_bounds__(kRowThreads)
k_cropped_node_values(const float* __restrict__ y, int ld_y, int col, int n_mean, int n_nodes,
                           const int32_t* __restrict__ node_ptr, const int32_t* __restrict__ lig_ptr,
                           const uint64_t* __restrict__ keep, int n_slots, int n_rec, int n_words, int rec_blocks,
                           float* __restrict__ lig_val, float* __restrict__ slot_rec_val) {
    const int lane = threadIdx.x % PVS_WAVE;
    if ((int)blockIdx.x < rec_blocks) {
        const long long wid = (long long)blockIdx.x * kWavesPerBlock + threadIdx.x / PVS_WAVE;
        if (wid >= (long long)n_slots * n_words) return;       // (the whole wavefront)
        const int p = (int)(wid / n_words), w = (int)(wid - (long long)p * n_words);
        const uint64_t* keep_row = keep + (size_t)p * n_words;
        const KeepCensus c = keep_census(keep_row, n_words, n_rec, w, lane);
        const PvsContactSlot s = pvs_cropped_slot(node_ptr, lig_ptr, p, n_nodes, c.kept, c.stray);
        const uint64_t word = s.n > 0 ? keep_row[w] : 0;
        const int rank = __popcll(word & ((1ull << lane) - 1));
        const long long j = (long long)w * PVS_WAVE + lane;
        if (j < n_rec)
            slot_rec_val[(size_t)p * n_rec + j] =
                (word >> lane) & 1 ? node_value(y, ld_y, col, n_mean, s.node0 + s.n + c.below + rank) : NAN;
        return;
    }
    const int p = (int)blockIdx.x - rec_blocks;
    const KeepCensus c = keep_census(keep + (size_t)p * n_words, n_words, n_rec, 0, lane);
    const PvsContactSlot s = pvs_cropped_slot(node_ptr, lig_ptr, p, n_nodes, c.kept, c.stray);
    for (int i = threadIdx.x; i < s.n; i += kRowThreads)      // (no slot: n < 0)
        lig_val[s.a0 + i] = node_value(y, ld_y, col, n_mean, s.node0 + i);
}
}  // namespace

// The accumulation kernel by itself, over rows that came from elsewhere (masking scores, ranks: hit_ranks.hip).
extern "C" int pvs_hit_rows_accumulate(const float* rows, int32_t n_hits, int32_t n_rec, double* rec_sum,
                                       int32_t* rec_count, float* rec_max, pvs_stream_t stream) {
    PVS_REQUIRE(n_hits >= 0 && n_rec >= 0, "hit_rows_accumulate: %d hits, %d receptor atoms", n_hits, n_rec);
    if (n_hits == 0 || n_rec == 0) return 0;
    PVS_REQUIRE(rows && rec_sum && rec_count && rec_max, "hit_rows_accumulate: NULL argument");
    k_contact_accumulate<<<(n_rec + kRowThreads - 1) / kRowThreads, kRowThreads, 0, (hipStream_t)stream>>>(
        rows, n_hits, n_rec, rec_sum, rec_count, rec_max);
    PVS_CHECK_LAUNCH();
    return 0;
}

extern "C" int pvs_slot_node_values_cropped(const float* y, int32_t ld_y, int32_t col, int32_t n_mean, int32_t n_nodes,
                                            const int32_t* node_ptr, const int32_t* lig_ptr, const uint64_t* keep,
                                            int32_t n_slots, int32_t n_rec, float* lig_val, float* slot_rec_val,
                                            double* rec_sum, int32_t* rec_count, float* rec_max, pvs_stream_t stream) {
    PVS_REQUIRE(n_mean == 1 || n_mean == 3, "slot_node_values_cropped: a node's value is one column or the mean of "
                "three (n_mean %d)", n_mean);
    PVS_REQUIRE(col >= 0 && ld_y >= 1 && col <= ld_y - n_mean, "slot_node_values_cropped: columns [%d, %d + %d) outside "
                "the %d of y", col, col, n_mean, ld_y);
    PVS_REQUIRE(n_slots >= 0 && n_rec >= 0 && n_nodes >= 0, "slot_node_values_cropped: %d slots, %d receptor atoms, %d "
                "rows", n_slots, n_rec, n_nodes);
    if (n_slots == 0 || n_rec == 0) return 0;
    PVS_REQUIRE(y && node_ptr && lig_ptr && keep && lig_val && slot_rec_val && rec_sum && rec_count && rec_max,
                "slot_node_values_cropped: NULL argument");
    const int n_words = (int)(((long long)n_rec + PVS_WAVE - 1) / PVS_WAVE);
    const long long rec_blocks = ((long long)n_slots * n_words + kWavesPerBlock - 1) / kWavesPerBlock;
    const long long blocks = rec_blocks + n_slots;
    PVS_REQUIRE(blocks < INT32_MAX, "slot_node_values_cropped: %d slots of %d receptor atoms are too many for one launch",
                n_slots, n_rec);
    hipStream_t s = (hipStream_t)stream;
    k_cropped_node_values<<<(unsigned)blocks, kRowThreads, 0, s>>>(y, ld_y, col, n_mean, n_nodes, node_ptr, lig_ptr,
                                                                        keep, n_slots, n_rec, n_words, (int)rec_blocks,
                                                                        lig_val, slot_rec_val);
    PVS_CHECK_LAUNCH();
    k_contact_accumulate<<<(n_rec + kRowThreads - 1) / kRowThreads, kRowThreads, 0, s>>>(slot_rec_val, n_slots, n_rec,
                                                                                         rec_sum, rec_count, rec_max);
    PVS_CHECK_LAUNCH();
    return 0;
}

extern "C" int pvs_contact_attention_cropped(const int32_t* rowptr, const uint8_t* etype, const float* att,
                                             int32_t n_nodes, int32_t n_edges, const int32_t* node_ptr,
                                             const int32_t* lig_ptr, const uint64_t* keep, int32_t n_slots,
                                             int32_t n_rec, float* lig_att, float* slot_rec_att, double* rec_sum,
                                             int32_t* rec_count, float* rec_max, pvs_stream_t stream) {
    PVS_REQUIRE(n_slots >= 0 && n_rec >= 0 && n_edges >= 0 && n_nodes >= 0, "contact_attention_cropped: %d slots, %d "
                "receptor atoms, %d edges, %d rows", n_slots, n_rec, n_edges, n_nodes);
    if (n_slots == 0 || n_rec == 0) return 0;
    PVS_REQUIRE(rowptr && etype && att && node_ptr && lig_ptr && keep && lig_att && slot_rec_att && rec_sum &&
                rec_count && rec_max, "contact_attention_cropped: NULL argument");
    const int n_words = (int)(((long long)n_rec + PVS_WAVE - 1) / PVS_WAVE);
    const long long rec_blocks = (long long)n_slots * n_words;
    const long long blocks = rec_blocks + (long long)n_slots * kLigBlocksPerSlot;
    PVS_REQUIRE(blocks < INT32_MAX, "contact_attention_cropped: %d slots of %d receptor atoms are too many for one "
                "launch", n_slots, n_rec);
    hipStream_t s = (hipStream_t)stream;
    k_cropped_contact_rows<<<(unsigned)blocks, kRowThreads, 0, s>>>(rowptr, etype, att, n_nodes, n_edges, node_ptr,
                                                                    lig_ptr, keep, n_slots, n_rec, n_words,
                                                                    (int)rec_blocks, lig_att, slot_rec_att);
    PVS_CHECK_LAUNCH();
    k_contact_accumulate<<<(n_rec + kRowThreads - 1) / kRowThreads, kRowThreads, 0, s>>>(slot_rec_att, n_slots, n_rec,
                                                                                         rec_sum, rec_count, rec_max);
    PVS_CHECK_LAUNCH();
    return 0;
}

extern "C" int pvs_slot_node_values(const float* y, int32_t ld_y, int32_t col, int32_t n_mean, int32_t n_nodes,
                                    const int32_t* node_ptr, const int32_t* lig_ptr, int32_t n_slots, int32_t n_rec,
                                    float* lig_val, float* slot_rec_val, double* rec_sum, int32_t* rec_count,
                                    float* rec_max, pvs_stream_t stream) {
    PVS_REQUIRE(n_mean == 1 || n_mean == 3, "slot_node_values: a node's value is one column or the mean of three (n_mean "
                "%d)", n_mean);
    PVS_REQUIRE(col >= 0 && ld_y >= 1 && col <= ld_y - n_mean, "slot_node_values: columns [%d, %d + %d) outside the %d "
                "of y", col, col, n_mean, ld_y);
    PVS_REQUIRE(n_slots >= 0 && n_rec >= 0 && n_nodes >= 0, "slot_node_values: %d slots, %d receptor atoms, %d rows",
                n_slots, n_rec, n_nodes);
    if (n_slots == 0 || n_rec == 0) return 0;
    PVS_REQUIRE((long long)n_slots * n_rec <= (long long)n_nodes, "slot_node_values: %d rows cannot hold %d slots of "
                "%d receptor atoms", n_nodes, n_slots, n_rec);
    PVS_REQUIRE(y && node_ptr && lig_ptr && lig_val && slot_rec_val && rec_sum && rec_count && rec_max,
                "slot_node_values: NULL argument");
    const long long rec_blocks = ((long long)n_slots * n_rec + kRowThreads - 1) / kRowThreads;
    const long long blocks = rec_blocks + n_slots;
    PVS_REQUIRE(blocks < INT32_MAX, "slot_node_values: %d slots of %d receptor atoms are too many for one launch",
                n_slots, n_rec);
    hipStream_t s = (hipStream_t)stream;
    k_slot_node_values<<<(unsigned)blocks, kRowThreads, 0, s>>>(y, ld_y, col, n_mean, n_nodes, node_ptr, lig_ptr,
                                                                n_slots, n_rec, (int)rec_blocks, lig_val, slot_rec_val);
    PVS_CHECK_LAUNCH();
    k_contact_accumulate<<<(n_rec + kRowThreads - 1) / kRowThreads, kRowThreads, 0, s>>>(slot_rec_val, n_slots, n_rec,
                                                                                         rec_sum, rec_count, rec_max);
    PVS_CHECK_LAUNCH();
    return 0;
}

extern "C" int pvs_contact_attention(const int32_t* rowptr, const uint8_t* etype, const float* att, int32_t n_nodes,
                                     int32_t n_edges, const int32_t* node_ptr, const int32_t* lig_ptr, int32_t n_slots,
                                     int32_t n_rec, float* lig_att, float* slot_rec_att, double* rec_sum,
                                     int32_t* rec_count, float* rec_max, pvs_stream_t stream) {
    PVS_REQUIRE(n_slots >= 0 && n_rec >= 0 && n_edges >= 0, "contact_attention: %d slots, %d receptor atoms, %d edges",
                n_slots, n_rec, n_edges);
    if (n_slots == 0 || n_rec == 0) return 0;
    PVS_REQUIRE((long long)n_slots * n_rec <= (long long)n_nodes, "contact_attention: %d rows cannot hold %d slots of "
                "%d receptor atoms", n_nodes, n_slots, n_rec);
    PVS_REQUIRE(rowptr && etype && att && node_ptr && lig_ptr && lig_att && slot_rec_att && rec_sum && rec_count &&
                rec_max, "contact_attention: NULL argument");
    const long long rec_blocks = ((long long)n_slots * n_rec * kRecLanes + kRowThreads - 1) / kRowThreads;
    const long long blocks = rec_blocks + (long long)n_slots * kLigBlocksPerSlot;
    PVS_REQUIRE(blocks < INT32_MAX, "contact_attention: %d slots of %d receptor atoms are too many for one launch",
                n_slots, n_rec);
    hipStream_t s = (hipStream_t)stream;
    k_contact_rows<<<(unsigned)blocks, kRowThreads, 0, s>>>(rowptr, etype, att, n_nodes, n_edges, node_ptr, lig_ptr,
                                                            n_slots, n_rec, (int)rec_blocks, lig_att, slot_rec_att);
    PVS_CHECK_LAUNCH();
    k_contact_accumulate<<<(n_rec + kRowThreads - 1) / kRowThreads, kRowThreads, 0, s>>>(slot_rec_att, n_slots, n_rec,
                                                                                         rec_sum, rec_count, rec_max);
    PVS_CHECK_LAUNCH();
    return 0;
}
