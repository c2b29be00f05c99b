// Per-hit ranks of receptor (and ligand) values (pvs_hit_value_ranks): the reference's hotspot.py with use_rank, where
// every atom's value in a binding event is replaced by its position in that event's descending sort before the mean
// over events (screening.py: ScreeningSweep.receptor_hotspots(use_rank=True)). A rank is a COUNT - how many candidates
// of the same hit stand before this one (hit_ranks.h) - so it needs no sort, no workspace and no order of evaluation:
// a workgroup per (hit, 256 candidates), the hit's candidates staged through LDS a tile at a time, every thread
// counting for its own candidate. O(M^2) compares per hit of M candidates; see DESIGN §5 for where that stops paying.
#include <math.h>
#include "common.h"
#include "hit_ranks.h"

namespace {
constexpr int kRankThreads = 256;

// Workgroup b of hit h owns the candidates q = 256 b + thread: q < n_rec is receptor atom q (position n_lig + q),
// the others are ligand atom q - n_rec (position q - n_rec) as far as the hit has them. Every output element has one
// writer. A hit's ligand range is checked by pvs_rank_hit; its values lie in the caller's lig_val / lig_rank.
__global__ void __launch_bounds__(kRankThreads)
k_hit_value_ranks(const float* __restrict__ rows, int n_rec, const float* __restrict__ lig_val,
                  const int32_t* __restrict__ lig_ptr, int blocks_per_hit, float* __restrict__ row_rank,
                  float* __restrict__ lig_rank) {
    __shared__ float tile[kPvsRankTile];
    const int h = (int)(blockIdx.x / (unsigned)blocks_per_hit), b = (int)(blockIdx.x % (unsigned)blocks_per_hit);
    const int q = b * kRankThreads + (int)threadIdx.x;
    const PvsRankHit hit = pvs_rank_hit(lig_ptr, h);       // (the same in every thread of the workgroup)
    const float* __restrict__ row = rows + (size_t)h * n_rec;
    float* __restrict__ out_row = row_rank + (size_t)h * n_rec;
    if (hit.n < 0) {                                        // no hit: a row of NaN, no ligand write
        if (q < n_rec) out_row[q] = NAN;
        return;
    }
    const int i = q - n_rec;                                // (the ligand atom, where q is one)
    float v = NAN;
    int pos = 0;
    if (q < n_rec) {
        v = row[q];
        pos = hit.n + q;
    } else if (i < hit.n) {
        v = lig_val[hit.a0 + i];
        pos = i;
    }
    const bool mine = v == v;
    int before = 0;
    if (__syncthreads_or(mine)) {                           // (a workgroup without a candidate counts nothing)
        const int m = hit.n + n_rec;
        for (int t0 = 0; t0 < m; t0 += kPvsRankTile) {
            for (int k = threadIdx.x; k < kPvsRankTile; k += kRankThreads) {
                const int p = t0 + k;
                tile[k] = p >= m ? NAN : p < hit.n ? lig_val[hit.a0 + p] : row[p - hit.n];
            }
            __syncthreads();
            const int len = min(kPvsRankTile, m - t0);
            if (mine) {
#pragma unroll 8
                for (int k = 0; k < len; ++k) before += pvs_rank_before(tile[k], t0 + k, v, pos) ? 1 : 0;
            }
            __syncthreads();
        }
    }
    const float rank = mine ? (float)before : NAN;
    if (q < n_rec) out_row[q] = rank;
    else if (i < hit.n) lig_rank[hit.a0 + i] = rank;
}
}  // namespace

extern "C" int pvs_hit_value_ranks(const float* rows, int32_t n_hits, int32_t n_rec, const float* lig_val,
                                   const int32_t* lig_ptr, float* row_rank, float* lig_rank, double* rank_sum,
                                   int32_t* rank_count, float* rank_max, pvs_stream_t stream) {
    PVS_REQUIRE(n_hits >= 0 && n_rec >= 0, "hit_value_ranks: %d hits, %d receptor atoms", n_hits, n_rec);
    const bool with_lig = lig_val || lig_ptr || lig_rank;
    PVS_REQUIRE(!with_lig || (lig_val && lig_ptr && lig_rank), "hit_value_ranks: lig_val, lig_ptr and lig_rank are all "
                "given or all NULL");
    PVS_REQUIRE((long long)n_rec + kPvsContactMaxLigand < (1ll << 24), "hit_value_ranks: %d receptor atoms: a rank is "
                "stored as a float and must be exact (n_rec + %d < 2^24)", n_rec, (int)kPvsContactMaxLigand);
    if (n_hits == 0 || n_rec == 0) return 0;
    PVS_REQUIRE(rows && row_rank && rank_sum && rank_count && rank_max, "hit_value_ranks: NULL argument");
    const long long room = (long long)n_rec + (with_lig ? (long long)kPvsContactMaxLigand : 0);
    const long long blocks_per_hit = (room + kRankThreads - 1) / kRankThreads;
    PVS_REQUIRE(blocks_per_hit * n_hits < INT32_MAX, "hit_value_ranks: %d hits of %d receptor atoms are too many for "
                "one launch", n_hits, n_rec);
    k_hit_value_ranks<<<(unsigned)(blocks_per_hit * n_hits), kRankThreads, 0, (hipStream_t)stream>>>(
        rows, n_rec, lig_val, lig_ptr, (int)blocks_per_hit, row_rank, lig_rank);
    PVS_CHECK_LAUNCH();
    return pvs_hit_rows_accumulate(row_rank, n_hits, n_rec, rank_sum, rank_count, rank_max, stream);
}
