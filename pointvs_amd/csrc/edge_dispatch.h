// Host-side choices of the edge kernels, in one place: which kernel family runs a layer, on what grid, and as which
// edge-residual kind. Plain C++ (no HIP types): tests/test_edge_dispatch.py compiles it alone with the host compiler.
#pragma once
#include <stdint.h>
#include <stdlib.h>
#include <type_traits>

#include "../../include/pvs_egnn.h"

// ---- kernel family ---------------------------------------------------------------------------------------------------
enum PvsEdgeFamily {
    PVS_EDGE_GENERIC,   // VALU / LDS kernels (edge_v0.hip): H = 16, more than 3 edge classes backward, PVS_EGNN_KERNELS=generic
    PVS_EDGE_SPLIT,     // H = 32 / 64 on split products: f16x2 forward and H = 32 backward, bf16x3 H = 64 backward
    PVS_EDGE_EXACT,     // exact fp32 MFMAs (edge_mfma.hip, the forward's F16X2 = false): the cross-check family of the tests
    PVS_EDGE_WIDE,      // H = 128 (hidden sizes 65..128 padded by the caller) on f16x2 products
};
enum PvsEdgeDirection { PVS_EDGE_FWD, PVS_EDGE_BWD };

// The ONLY place that reads the family switches:
//   PVS_EGNN_KERNELS=generic   the generic kernels everywhere (H = 128 has none: the layer calls refuse it)
//   PVS_EGNN_BF16X3=0          exact fp32 MFMAs instead of the split products (the H = 128 forward has no exact form)
//   PVS_EGNN_BF16X3_H64=0      the same for H = 64 only
// Read at every call: the tests flip them inside one process (layer_plan.h, pvs_layer_switches). No family depends on the
// layer's flags today; they are part of the question all the same.
inline PvsEdgeFamily pvs_edge_family(int H, uint32_t flags, int n_attr, PvsEdgeDirection dir) {
    (void)flags;
    const char* kernels = getenv("PVS_EGNN_KERNELS");
    if (kernels && kernels[0] == 'g') return PVS_EDGE_GENERIC;
    if (H != 32 && H != 64 && H != 128) return PVS_EDGE_GENERIC;
    if (dir == PVS_EDGE_BWD && n_attr > 3) return PVS_EDGE_GENERIC;      // (the MFMA backward holds 3 edge classes)
    const char* bf = getenv("PVS_EGNN_BF16X3");
    const char* bf64 = getenv("PVS_EGNN_BF16X3_H64");
    const bool exact_all = bf && bf[0] == '0', exact_h64 = bf64 && bf64[0] == '0';
    if (H == 128) return dir == PVS_EDGE_BWD && exact_all ? PVS_EDGE_EXACT : PVS_EDGE_WIDE;
    return exact_all || (H == 64 && exact_h64) ? PVS_EDGE_EXACT : PVS_EDGE_SPLIT;
}

// ---- grid and chunk plan ---------------------------------------------------------------------------------------------
// Edges a wave gets before the grid grows by another workgroup. 512 until round 5 (sixteen tiles amortise a workgroup's
// weight staging): right for BASELINE-size batches, whose grids are capped by the CU count anyway, and wrong for small ones
// - at the reference's default shape (32 graphs of 500 atoms, r = 4 A: 176k edges) the backward ran on 43 of 256 CUs.
// Two tiles per wave: edge forward 0.62 -> 0.20 ms, edge backward 0.81 -> 0.28 ms per 6-layer step there (32: 0.19 / 0.28;
// profiles/r05_ab_small_batch_grid.txt). PVS_EDGES_PER_WAVE overrides it (A/B, and the tests' way to other work partitions:
// read at every call, like the family switches; 0 or below counts as unset). The team kernels (H = 128 backward, exact
// H = 64 backward) keep 512 per team whatever it says.
inline int pvs_edges_per_wave() {
    const char* e = getenv("PVS_EDGES_PER_WAVE");
    const int x = e ? atoi(e) : 0;
    return x > 0 ? x : 64;
}

// Edges per chunk above which a wave's share is cut into several chunks (PVS_CHUNK_EDGES overrides it: A/B and tests; read
// at every call; 0 or below counts as unset; it reaches every MFMA edge launcher, each with its own default).
// Chunk ends are row-aligned, so a wave's share is uneven by up to a row per chunk end (157 edges at cfg2) and the launch
// waits for the largest share: FEWER, larger chunks per wave balance better (round 6, H = 32 backward at cfg2: two chunks
// of 2.5 k edges per wave -> one of 5 k: -2.5 % per launch; perfectly equal shares - a timing-only build - would give
// -3.3 %: profiles/r06_ab_chunk_balance.txt).
inline long long pvs_chunk_edges(long long dflt = 4096) {
    const char* e = getenv("PVS_CHUNK_EDGES");
    const long long v = e ? atoll(e) : 0ll;
    return v > 0 ? v : dflt;
}

// Fill the chip first: a wave (a team, for the team kernels: waves_per_block = teams per block) gets at least
// min_edges_per_wave edges where the range allows, on at most max_blocks workgroups; then every wave gets the same number
// of chunks, of at most ~chunk_edges edges each.
struct PvsEdgeGrid {
    int blocks, n_chunks;
};
// (also device code: a forward launch over a graph whose edge count lives on the device plans its chunks there, from the
// count itself - pvs_edge_replan below - so that its sums do not depend on the room the caller gave the edge arrays)
#ifdef __HIPCC__
#define PVS_DISPATCH_FN __host__ __device__ inline
#else
#define PVS_DISPATCH_FN inline
#endif
PVS_DISPATCH_FN PvsEdgeGrid pvs_edge_grid(long long E, int waves_per_block, int max_blocks, long long min_edges_per_wave,
                                          long long chunk_edges) {
    const long long per_block = waves_per_block * min_edges_per_wave;
    long long b = (E + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    const long long waves = b * waves_per_block;
    long long per_wave = (E + waves * chunk_edges - 1) / (waves * chunk_edges);
    if (per_wave < 1) per_wave = 1;
    return PvsEdgeGrid{(int)b, (int)(waves * per_wave)};
}

// What a launch planned on the host with a CAPACITY keeps, so that the kernel can plan again with the device-side count:
// the chunk count of pvs_edge_grid for that count. The grid stays the capacity's (at least as many workgroups: the block
// count grows with E), and the chunk loop strides over whatever number of chunks there is.
struct PvsEdgePlan {
    int waves_per_block, max_blocks, min_edges_per_wave, chunk_edges;
};
inline PvsEdgePlan pvs_edge_plan(int waves_per_block, int max_blocks, long long min_edges_per_wave, long long chunk_edges) {
    const long long top = 0x7fffffffll;
    return PvsEdgePlan{waves_per_block, max_blocks, (int)(min_edges_per_wave < top ? min_edges_per_wave : top),
                       (int)(chunk_edges < top ? chunk_edges : top)};
}
PVS_DISPATCH_FN int pvs_edge_replan(const PvsEdgePlan& p, long long E) {
    return pvs_edge_grid(E, p.waves_per_block, p.max_blocks, p.min_edges_per_wave, p.chunk_edges).n_chunks;
}

// Block caps (256 CUs). A backward workgroup leaves one weight-gradient slab, so the layer's workspace holds
// kPvsEdgeSlabCapacity of them and every backward launcher checks its grid against that before it reports *n_slabs.
constexpr int kPvsFwdMaxBlocks = 1024;            // forward, 256-thread workgroups: four per CU
constexpr int kPvsFwdLargeMaxBlocks = 256;        // forward, 512 / 768 threads (H = 64) or 138 KB of LDS (H = 128): one per CU
constexpr int kPvsBwdF16MaxBlocks = 256;          // H = 32 split: one workgroup per CU (LDS)
constexpr int kPvsBwdH64MaxBlocks = 256;          // H = 64 split: one workgroup per CU (registers: one wave per SIMD)
constexpr int kPvsBwdWideMaxBlocks = 256;         // H = 128: one team per CU (LDS; edge_bwd_wide.hip asserts it)
constexpr int kPvsBwdExactMaxBlocks = 512;        // exact H = 32: 2 x 256 threads per CU; H = 64: two 128-thread teams per CU
constexpr int kPvsBwdExactWideMaxBlocks = 256;    // exact H = 128: one team per CU
constexpr int kPvsBwdGenericMaxBlocks = 512;
constexpr int pvs_max_int(int a, int b) { return a > b ? a : b; }
constexpr int kPvsEdgeSlabCapacity =
    pvs_max_int(pvs_max_int(pvs_max_int(kPvsBwdF16MaxBlocks, kPvsBwdH64MaxBlocks),
                            pvs_max_int(kPvsBwdWideMaxBlocks, kPvsBwdExactMaxBlocks)),
                pvs_max_int(kPvsBwdExactWideMaxBlocks, kPvsBwdGenericMaxBlocks));

// ---- edge residual ---------------------------------------------------------------------------------------------------
// m = m_new + m_prev (sum), g m_new + m_prev (rezero), relu(g) m_new + (1 - relu(g)) m_prev (gated); rezero wins over gated
// as the reference orders them (egnn_satorras.py:194-202). Each launcher maps the kind to its own template kinds.
enum PvsEdgeResidual { PVS_ERES_NONE = 0, PVS_ERES_SUM = 1, PVS_ERES_REZERO = 2, PVS_ERES_GATED = 3 };
inline PvsEdgeResidual pvs_edge_residual_kind(uint32_t flags, bool has_m_prev) {
    if (!(flags & PVS_EDGE_RESIDUAL) || !has_m_prev) return PVS_ERES_NONE;
    if (flags & PVS_REZERO) return PVS_ERES_REZERO;
    return (flags & PVS_GATED_RESIDUAL) ? PVS_ERES_GATED : PVS_ERES_SUM;
}

// ---- first-layer backward --------------------------------------------------------------------------------------------
// A backward call whose caller asks no gradient of the layer's INPUT coordinates (g_x == NULL: the first layer of a model
// whose positions need no gradient - training, scoring, the benchmark) takes the first-layer pair: an edge backward that
// forms no per-edge coordinate gradient and leaves one word per edge (rho | type) instead of the 16-byte record
// (edge_bwd_f16.hip: k_edge_bwd_f16_nogx), and a column gather that reads that word alone (edge_v0.hip:
// k_node_gather_rho). The pair exists for the BASELINE instantiation of the H = 32 split family only: no edge residual, no
// edge attention, coordinates updated with a live g_x_out. Every other call runs the general pair.
//   PVS_EGNN_FIRST_LAYER_BWD=0   the general pair everywhere (A/B, and the tests' reference run; read at every call)
// n_attr <= 3 is what the split family's backward holds (pvs_edge_family); it is restated because the gather variant sums
// three classes.
inline bool pvs_first_layer_bwd(int H, uint32_t flags, int n_attr, bool has_m_prev, bool has_g_x_out, bool wants_g_x) {
    const char* sw = getenv("PVS_EGNN_FIRST_LAYER_BWD");
    if (sw && sw[0] == '0') return false;
    if (wants_g_x || !has_g_x_out || !(flags & PVS_UPDATE_COORDS)) return false;
    if (H != 32 || n_attr > 3 || pvs_edge_family(H, flags, n_attr, PVS_EDGE_BWD) != PVS_EDGE_SPLIT) return false;
    return !(flags & PVS_EDGE_ATTENTION) && pvs_edge_residual_kind(flags, has_m_prev) == PVS_ERES_NONE;
}

// ---- run-time (kind, switch) -> template arguments -------------------------------------------------------------------
// Calls f(std::integral_constant<int, K>{}, std::bool_constant<B>{}) for kind == K in [0, NK) and b == B and returns its
// result: exactly NK x 2 instantiations of what f launches.
template <int NK, class F>
int pvs_dispatch(int kind, bool b, F&& f) {
    if constexpr (NK > 1) {
        if (kind != NK - 1) return pvs_dispatch<NK - 1>(kind, b, f);
    }
    return b ? f(std::integral_constant<int, NK - 1>{}, std::true_type{})
             : f(std::integral_constant<int, NK - 1>{}, std::false_type{});
}
