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
template <int LANES>
__device__ __forceinline__ float row_contact_max(const int32_t* __restrict__ rowptr, const uint8_t* __restrict__ etype,
                                                 const float* __restrict__ att, int n_edges, int row, int lane) {
    const int e0 = max(rowptr[row], 0), e1 = min(rowptr[row + 1], n_edges);
    float cur = NAN;
    for (int k = lane; k < e1 - e0; k += LANES)
        if (etype[e0 + k] == 1) cur = pvs_contact_max(cur, att[e0 + k]);
#pragma unroll
    for (int o = 1; o < LANES; o <<= 1) cur = pvs_contact_max(cur, __shfl_xor(cur, o, PVS_WAVE));
    return cur;
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
}  // namespace

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
