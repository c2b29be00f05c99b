// Leave-one-atom-out copies of a set of ligands as the slots of a pose batch (pvs_leave_out_ligand_pack): what turns the
// hits of a sweep into LibraryScreen batches without a host loop per atom.
#include "common.h"
#include "leave_out.h"
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
}  // namespace

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
