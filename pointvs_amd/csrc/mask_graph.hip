// pvs_mask_graph_build: the leave-out graph batch of masking attribution (the reference's atom_masking /
// bond_masking, /root/reference/point_vs/attribution/attribution_fns.py:39-115, 356-456). Input: the prepared CSR of ONE
// complex and a table drop[B][2] of node ids (drop[b][1] = -1: one atom). Output: the CSR of the disjoint union of B
// copies of the complex, copy b without its dropped node(s) and every edge that touches them, node ids renumbered
// densely (the reference's `-= 1` shifts), plus src_node (which parent node each output node is: the caller gathers
// features and coordinates with it, so nothing here depends on their dtype).
//
// No sort: the parent's edges are ordered by row and, inside a row, in input order (pvs_graph_prepare's stable sort).
// Dropping nodes keeps the relative order of the surviving rows (the renumbering is monotone) and of the surviving
// edges inside a row, and a stable sort of a filtered list is the filtered stable sort - so the filtered parent CSR IS
// what pvs_graph_prepare makes of the masked COO list. Three passes over (copy, parent row) pairs: count the surviving
// edges, scan, fill. Every output word is written by exactly one lane at a position that depends on the inputs only:
// no atomics on the outputs, bitwise reproducible. Forward-only (no CSC, no perm).
#include "common.h"
#include "profile.h"
#include <hipcub/hipcub.hpp>

namespace {

typedef unsigned long long u64;

enum { kBadId = 1, kOverflow = 4, kNodeCount = 8, kEdgeCount = 16 };

// thread per copy: validate the pair, order it (lo < hi, hi = -1 for one atom), count its dropped nodes
__global__ void k_mask_pairs(const int32_t* __restrict__ drop, int B, int N, int2* __restrict__ pairs,
                             int32_t* __restrict__ n_drop, int32_t* __restrict__ status) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b > B) return;
    if (b == B) { n_drop[b] = 0; return; }
    int d0 = drop[2 * b], d1 = drop[2 * b + 1];
    if (d0 < 0 || d0 >= N || d1 < -1 || d1 >= N) {
        atomicOr(status, kBadId);       // (a flag: the later passes write nothing once it is set)
        d0 = 0; d1 = -1;
    }
    if (d1 == d0) d1 = -1;
    const int lo = d1 < 0 ? d0 : min(d0, d1), hi = d1 < 0 ? -1 : max(d0, d1);
    pairs[b] = make_int2(lo, hi);
    n_drop[b] = hi < 0 ? 1 : 2;
}

struct MaskArgs {
    const int32_t *rowptr, *col;
    const uint8_t* etype;
    const int2* pairs;
    const int32_t* drop_ptr;     // [B + 1] exclusive scan of the dropped-node counts
    int B, N, total_nodes, capacity;
    bool exact;                  // the caller states the edge count: anything else than `capacity` edges is an error
};

// new id of parent node i in a copy without lo (and hi)
__device__ __forceinline__ int mask_shift(int i, int lo, int hi) { return i - (i > lo) - (hi >= 0 && i > hi); }

// a group of G lanes per (copy, parent row). FILL = false: the row's surviving degree, src_node, graph_ptr;
// FILL = true: the row's segment of row / col / etype, inv_deg, graph_eptr.
template <int G, bool FILL>
__global__ void __launch_bounds__(256)
k_mask_rows(MaskArgs a, int32_t* __restrict__ deg, int32_t* __restrict__ src_node, int32_t* __restrict__ graph_ptr,
            const int32_t* __restrict__ out_rowptr, int32_t* __restrict__ row, int32_t* __restrict__ col,
            uint8_t* __restrict__ etype, float* __restrict__ inv_deg, int32_t* __restrict__ graph_eptr,
            int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63, sub = lane & (G - 1), gbase = lane & ~(G - 1);
    const long long item = ((long long)blockIdx.x * 256 + threadIdx.x) / G;
    if (item >= (long long)a.B * a.N) return;
    if (*status & (kBadId | kNodeCount)) return;
    if ((long long)a.B * a.N - a.drop_ptr[a.B] != a.total_nodes) {        // the caller's node count is not this table's
        if (item == 0 && sub == 0) atomicOr(status, kNodeCount);
        return;
    }
    if (FILL && out_rowptr[a.total_nodes] > a.capacity) {
        if (item == 0 && sub == 0) atomicOr(status, kOverflow);
        return;
    }
    if (FILL && a.exact && out_rowptr[a.total_nodes] != a.capacity) {
        if (item == 0 && sub == 0) atomicOr(status, kEdgeCount);
        return;
    }
    const int b = (int)(item / a.N), i = (int)(item - (long long)b * a.N);
    const int2 p = a.pairs[b];
    const int node0 = b * a.N - a.drop_ptr[b];                             // first output node of copy b
    if (i == 0 && sub == 0) {
        if (!FILL) {
            graph_ptr[b] = node0;
            if (b == a.B - 1) { graph_ptr[a.B] = a.total_nodes; deg[a.total_nodes] = 0; }
        } else {
            graph_eptr[b] = out_rowptr[node0];
            if (b == a.B - 1) graph_eptr[a.B] = out_rowptr[a.total_nodes];
        }
    }
    if (i == p.x || i == p.y) return;                                      // (group-uniform)
    const int r = node0 + mask_shift(i, p.x, p.y);
    const int e0 = a.rowptr[i], e1 = a.rowptr[i + 1];
    const u64 gmask = (G == 64 ? ~0ull : ((1ull << G) - 1ull) << gbase);
    const u64 below = gmask & ((1ull << lane) - 1ull);
    int kept = 0;
    int out = FILL ? out_rowptr[r] : 0;
    for (int e = e0; e < e1; e += G) {                                     // (trip count is group-uniform)
        const int k = e + sub;
        int c = -1;
        if (k < e1) c = a.col[k];
        const bool keep = k < e1 && c != p.x && c != p.y;
        const u64 m = __ballot(keep) & gmask;
        if (FILL && keep) {
            const int at = out + kept + __popcll(m & below);
            row[at] = r;
            col[at] = node0 + mask_shift(c, p.x, p.y);
            if (etype) etype[at] = a.etype[k];
        }
        kept += __popcll(m);
    }
    if (sub == 0) {
        if (!FILL) {
            deg[r] = kept;
            src_node[r] = i;
        } else {
            inv_deg[r] = 1.0f / (float)(kept > 1 ? kept : 1);
        }
    }
}

struct MaskWs {
    int2* pairs;
    int32_t *n_drop, *drop_ptr, *deg;
    void* scan_tmp;
    size_t scan_bytes;
};

size_t carve_mask(PvsArena& a, long long total_nodes_cap, int B, MaskWs* out) {
    MaskWs t;
    t.pairs = a.take<int2>((size_t)B);
    t.n_drop = a.take<int32_t>((size_t)B + 1);
    t.drop_ptr = a.take<int32_t>((size_t)B + 1);
    t.deg = a.take<int32_t>((size_t)total_nodes_cap + 1);
    size_t s1 = 0, s2 = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, s1, (const int32_t*)nullptr, (int32_t*)nullptr, B + 1);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, s2, (const int32_t*)nullptr, (int32_t*)nullptr,
                                           (int)(total_nodes_cap + 1));
    t.scan_bytes = s1 > s2 ? s1 : s2;
    t.scan_tmp = a.take<char>(t.scan_bytes);
    if (out) *out = t;
    return a.off;
}

template <int G>
int launch_mask(const MaskArgs& a, const MaskWs& w, int32_t* rowptr, int32_t* row, int32_t* col, uint8_t* etype,
                float* inv_deg, int32_t* src_node, int32_t* graph_ptr, int32_t* graph_eptr, int32_t* status,
                hipStream_t s) {
    const long long lanes = (long long)a.B * a.N * G;
    const unsigned blocks = (unsigned)((lanes + 255) / 256);
    k_mask_rows<G, false><<<blocks, 256, 0, s>>>(a, w.deg, src_node, graph_ptr, nullptr, nullptr, nullptr, nullptr,
                                                  nullptr, nullptr, status);
    PVS_CHECK_LAUNCH();
    size_t sb = w.scan_bytes;
    PVS_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(w.scan_tmp, sb, w.deg, rowptr, a.total_nodes + 1, s));
    k_mask_rows<G, true><<<blocks, 256, 0, s>>>(a, nullptr, nullptr, nullptr, rowptr, row, col, etype, inv_deg,
                                                 graph_eptr, status);
    PVS_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" size_t pvs_mask_graph_workspace_bytes(int32_t n_nodes, int32_t n_masks) {
    if (n_nodes <= 0 || n_masks <= 0) return 256;
    PvsArena a(nullptr, 0);
    return carve_mask(a, (long long)n_nodes * n_masks, n_masks, nullptr) + 256;
}

extern "C" int pvs_mask_graph_build(const PvsGraph* parent, const int32_t* drop, int32_t n_masks, int32_t total_nodes,
                                    int32_t capacity, int32_t exact_edges, int32_t* rowptr, int32_t* row, int32_t* col, uint8_t* etype,
                                    float* inv_deg, int32_t* src_node, int32_t* graph_ptr, int32_t* graph_eptr,
                                    int32_t* status, void* workspace, size_t workspace_bytes, pvs_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    PVS_REQUIRE(parent && drop && rowptr && row && col && inv_deg && src_node && graph_ptr && graph_eptr && status &&
                workspace, "pvs_mask_graph_build: NULL");
    const int N = parent->n_nodes, E = parent->n_edges, B = n_masks;
    PVS_REQUIRE(N > 0 && E >= 0 && B > 0, "pvs_mask_graph_build: needs a graph and at least one mask (N=%d E=%d B=%d)",
                N, E, B);
    PVS_REQUIRE(!parent->n_edges_dev, "pvs_mask_graph_build: needs a parent with a host-side edge count");
    PVS_REQUIRE(parent->rowptr && (E == 0 || parent->col), "pvs_mask_graph_build: parent without CSR arrays");
    PVS_REQUIRE((etype != nullptr) == (parent->etype != nullptr), "pvs_mask_graph_build: etype output must be given "
                "exactly when the parent has edge classes");
    PVS_REQUIRE((long long)N * B < (1ll << 31) - 1 && (long long)E * B < (1ll << 31),
                "pvs_mask_graph_build: %d copies of N=%d E=%d do not fit int32", B, N, E);
    PVS_REQUIRE(total_nodes >= (long long)B * N - 2ll * B && total_nodes <= (long long)B * (N - 1) && total_nodes >= 0,
                "pvs_mask_graph_build: total_nodes=%d is not %d copies of %d nodes less one or two each", total_nodes,
                B, N);
    PVS_REQUIRE(capacity >= 0 && (long long)capacity <= (long long)B * E, "pvs_mask_graph_build: capacity %d outside "
                "[0, n_masks * E = %lld]", capacity, (long long)B * E);
    PvsArena arena(workspace, workspace_bytes);
    MaskWs w;
    carve_mask(arena, (long long)N * B, B, &w);
    PVS_REQUIRE(arena.ok(), "pvs_mask_graph_build: workspace too small (%zu < %zu)", workspace_bytes, arena.off);
    PvsProfScope prof(s, PVS_PROF_MASK_GRAPH);
    PVS_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    k_mask_pairs<<<(B + 1 + 255) / 256, 256, 0, s>>>(drop, B, N, w.pairs, w.n_drop, status);
    PVS_CHECK_LAUNCH();
    size_t sb = w.scan_bytes;
    PVS_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(w.scan_tmp, sb, w.n_drop, w.drop_ptr, B + 1, s));
    MaskArgs a{parent->rowptr, parent->col, parent->etype, w.pairs, w.drop_ptr, B, N, total_nodes, capacity, exact_edges != 0};
    // lanes per row: a whole wave for the long rows of a 10 A graph (~150 edges), 16 lanes for the short rows of the
    // reference's default 4 A graphs (~15 edges), where a wave per row would idle three lanes in four
    if ((long long)E >= 48ll * N)
        return launch_mask<64>(a, w, rowptr, row, col, etype, inv_deg, src_node, graph_ptr, graph_eptr, status, s);
    return launch_mask<16>(a, w, rowptr, row, col, etype, inv_deg, src_node, graph_ptr, graph_eptr, status, s);
}
