// Best pose per ligand (pvs_segment_argmax): the one reduction every user of a sweep does next, on the device.
#include "common.h"
#include "pose_select.h"

namespace {
constexpr int kSelectWaves = 4;     // segments per workgroup, one wavefront each

// One wavefront per segment: lane l looks at the rows l, l + 64, ... of the segment and keeps the better candidate
// (pose_select.h), six butterfly steps leave the segment's winner in every lane, then the lanes copy the winning row.
// Nothing is shared between wavefronts: no LDS, no barrier, no atomics.
__global__ void __launch_bounds__(kSelectWaves * PVS_WAVE)
k_segment_argmax(const float* __restrict__ scores, int C, int column, const int32_t* __restrict__ seg_ptr, int L,
                 int32_t* __restrict__ best, float* __restrict__ best_rows) {
    const int lane = threadIdx.x % PVS_WAVE;
    const int seg = blockIdx.x * kSelectWaves + threadIdx.x / PVS_WAVE;
    if (seg >= L) return;       // (the whole wavefront)
    const int r0 = seg_ptr[seg], r1 = seg_ptr[seg + 1];
    PvsPosePick cur = pvs_pose_none();
    for (int r = r0 + lane; r < r1; r += PVS_WAVE) {
        const PvsPosePick cand{scores[(size_t)r * C + column], r - r0};
        if (pvs_pose_better(cand, cur)) cur = cand;
    }
#pragma unroll
    for (int o = 1; o < PVS_WAVE; o <<= 1) {
        const PvsPosePick other{__shfl_xor(cur.value, o, PVS_WAVE), __shfl_xor(cur.index, o, PVS_WAVE)};
        cur = pvs_pose_merge(cur, other);
    }
    if (lane == 0) best[seg] = cur.index;
    const float* src = scores + (size_t)(r0 + (cur.index < 0 ? 0 : cur.index)) * C;
    for (int c = lane; c < C; c += PVS_WAVE) best_rows[(size_t)seg * C + c] = cur.index < 0 ? NAN : src[c];
}
}  // namespace

extern "C" int pvs_segment_argmax(const float* scores, int32_t n_cols, int32_t column, const int32_t* seg_ptr,
                                  int32_t n_segments, int32_t* best, float* best_rows, pvs_stream_t stream) {
    PVS_REQUIRE(n_cols >= 1 && column >= 0 && column < n_cols, "segment_argmax: column %d of %d", column, n_cols);
    PVS_REQUIRE(n_segments >= 0, "segment_argmax: %d segments", n_segments);
    if (n_segments == 0) return 0;
    PVS_REQUIRE(scores && seg_ptr && best && best_rows, "segment_argmax: NULL argument");
    const int blocks = (n_segments + kSelectWaves - 1) / kSelectWaves;
    k_segment_argmax<<<blocks, kSelectWaves * PVS_WAVE, 0, (hipStream_t)stream>>>(scores, n_cols, column, seg_ptr,
                                                                                  n_segments, best, best_rows);
    PVS_CHECK_LAUNCH();
    return 0;
}
