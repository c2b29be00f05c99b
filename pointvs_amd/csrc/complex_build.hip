// pvs_complex_batch_*: the node tables of a batch of protein-ligand complexes, built from a device-resident pool of
// structure files. Restates, per sample, parquets_to_inputs / __getitem__ of the reference loader
// (/root/reference/point_vs/preprocessing/data_loaders.py:259-309, 349-391) up to the edge list:
//   concat_structs      ligand atoms (optionally turned: augmented actives), then the receptor's
//   make_box            a receptor atom stays iff some ligand atom is closer than `radius`
//                       (cdist(ligand, receptor) < radius: fp64, sqrt(sum_k d_k^2), no FMA contraction)
//   hydrogen filter     atomic_number > 1, AFTER the crop (a contact through a hydrogen still keeps the receptor atom)
//   make_bit_vector     one-hot features from the smina type or the atomic-number class, receptor classes offset by
//                       n_features; compact: class % n_features plus the class / n_features column
//   pos                 fp32 of the fp64 coordinates; with `rot` a per-sample rotation on pos only - the edge list is
//                       built from the unrotated coordinates (pos_graph), as the reference builds it from `struct`
// One workgroup per sample: the ligand's (turned) coordinates sit in LDS as fp64, the receptor's atoms are strided over
// the lanes; survivors are compacted stably (ballot + prefix over the waves), so the node order is the reference's:
// all ligand atoms in file order, then the surviving receptor atoms in file order.
// _count writes one flag per input atom and the two counts of every sample; the host reads the counts (one copy per
// batch), sizes the tables and hands the node offsets to _fill. pvs_complex_edges turns the radius graph of the batch
// (pvs_radius_graph_*, run on pos_graph) into the loader's per-graph edge lists.
#include "common.h"
#include "profile.h"
#include "radius_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxLig = 1024;      // ligand atoms held in LDS (24 KB as fp64)
constexpr int kLutSize = 128;      // atomic numbers the class table covers; others fall into the overflow class

enum : int { kBadPair = 1, kLigTooLarge = 2, kBadType = 4, kBadCounts = 8, kBadEdges = 16,
              kNodeOverflow = PVS_CAP_NODE_OVERFLOW, kNoAtomLeft = PVS_CAP_EMPTY_SAMPLE };

// row vector times matrix, x' = x @ M, products and sums rounded one by one in this order (no contraction), so that a
// host evaluation with element-wise fp64 operations gives the same bits
__device__ __forceinline__ void xform(const double* __restrict__ m, double x, double y, double z, double* out) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        double t = __dmul_rn(x, m[j]);
        t = __dadd_rn(t, __dmul_rn(y, m[3 + j]));
        t = __dadd_rn(t, __dmul_rn(z, m[6 + j]));
        out[j] = t;
    }
}

struct Sample {
    int rec0, n_rec, lig0, n_lig, flag0;
    bool ok;
};

// pairs [B,3]: receptor id, ligand id, offset of the sample's flags (ligand atoms first) in the flag array
__device__ __forceinline__ Sample load_sample(const PvsComplexPool& pool, const int32_t* __restrict__ pairs, int s,
                                              int32_t* __restrict__ status) {
    Sample q;
    const int r = pairs[3 * s], l = pairs[3 * s + 1];
    q.flag0 = pairs[3 * s + 2];
    q.ok = r >= 0 && r < pool.n_rec && l >= 0 && l < pool.n_lig && q.flag0 >= 0;
    if (!q.ok) {
        if (threadIdx.x == 0) atomicOr(status, kBadPair);
        return q;
    }
    q.rec0 = pool.rec_ptr[r];
    q.n_rec = pool.rec_ptr[r + 1] - q.rec0;
    q.lig0 = pool.lig_ptr[l];
    q.n_lig = pool.lig_ptr[l + 1] - q.lig0;
    if (q.n_lig > kMaxLig || q.n_lig < 0 || q.n_rec < 0) {
        q.ok = false;
        if (threadIdx.x == 0) atomicOr(status, kLigTooLarge);
    }
    return q;
}

__global__ void __launch_bounds__(kThreads)
k_complex_count(PvsComplexPool pool, const int32_t* __restrict__ pairs, const double* __restrict__ lig_xform,
                Radius radius, int keep_hydrogens, int flag_cap, uint8_t* __restrict__ flags,
                int32_t* __restrict__ counts, int32_t* __restrict__ status) {
    __shared__ double lx[kMaxLig], ly[kMaxLig], lz[kMaxLig];
    __shared__ int n_kept[2];
    const int s = blockIdx.x;
    const Sample q = load_sample(pool, pairs, s, status);
    const bool fits = q.ok && q.flag0 + q.n_lig + q.n_rec <= flag_cap;
    if (!fits) {                                      // (block-uniform)
        if (q.ok && threadIdx.x == 0) atomicOr(status, kBadPair);
        if (threadIdx.x < 2) counts[2 * s + threadIdx.x] = 0;
        return;
    }
    if (threadIdx.x < 2) n_kept[threadIdx.x] = 0;
    const double* m = lig_xform ? lig_xform + 9 * (size_t)s : nullptr;
    int mine = 0;
    for (int a = threadIdx.x; a < q.n_lig; a += kThreads) {
        const double* p = pool.lig_xyz + 3 * (size_t)(q.lig0 + a);
        double c[3] = {p[0], p[1], p[2]};
        if (m) xform(m, p[0], p[1], p[2], c);
        lx[a] = c[0]; ly[a] = c[1]; lz[a] = c[2];
        const bool keep = keep_hydrogens || pool.lig_z[q.lig0 + a] > 1;
        flags[q.flag0 + a] = keep;
        mine += keep;
    }
    __syncthreads();
    if (mine) atomicAdd(&n_kept[0], mine);
    mine = 0;
    for (int a = threadIdx.x; a < q.n_rec; a += kThreads) {
        const double* p = pool.rec_xyz + 3 * (size_t)(q.rec0 + a);
        const double x = p[0], y = p[1], z = p[2];
        bool near = false;
        for (int j = 0; j < q.n_lig && !near; ++j) near = below(pvs_sqdist(lx[j], ly[j], lz[j], x, y, z), radius);
        const bool keep = near && (keep_hydrogens || pool.rec_z[q.rec0 + a] > 1);
        flags[q.flag0 + q.n_lig + a] = keep;
        mine += keep;
    }
    if (mine) atomicAdd(&n_kept[1], mine);
    __syncthreads();
    if (threadIdx.x < 2) counts[2 * s + threadIdx.x] = n_kept[threadIdx.x];
}

struct Encoding {
    int use_atomic_numbers, n_features, compact, feature_dim;
};

// BatchT: the graph id of a node as the loader's int64 batch vector, or as the int32 node_graph of the capacity builder.
// kCap (pvs_complex_batch_build_cap): total_nodes is a capacity; a sample whose rows end behind it is left out whole
// (the offset scan has set the overflow bit already), everything else is as without it.
template <class BatchT, bool kCap>
__global__ void __launch_bounds__(kThreads)
k_complex_fill(PvsComplexPool pool, const int32_t* __restrict__ pairs, const double* __restrict__ lig_xform,
               const double* __restrict__ rot, Encoding enc, const int32_t* __restrict__ class_of_z, int flag_cap,
               const uint8_t* __restrict__ flags, const int32_t* __restrict__ counts,
               const int32_t* __restrict__ graph_ptr, int total_nodes, float* __restrict__ x,
               float* __restrict__ pos, float* __restrict__ pos_graph, uint8_t* __restrict__ bp,
               BatchT* __restrict__ batch, int32_t* __restrict__ status) {
    __shared__ int wave_n[kWaves];
    const int s = blockIdx.x;
    const Sample q = load_sample(pool, pairs, s, status);
    if (!q.ok || q.flag0 + q.n_lig + q.n_rec > flag_cap) return;
    const int n0 = graph_ptr[s], n1 = graph_ptr[s + 1];
    if (kCap && n0 >= 0 && n1 >= n0 && n1 > total_nodes) return;
    if (n0 < 0 || n1 < n0 || n1 > total_nodes || n1 - n0 != counts[2 * s] + counts[2 * s + 1]) {
        if (threadIdx.x == 0) atomicOr(status, kBadCounts);
        return;
    }
    const double* m = lig_xform ? lig_xform + 9 * (size_t)s : nullptr;
    const double* r = rot ? rot + 9 * (size_t)s : nullptr;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int n_in = q.n_lig + q.n_rec;
    int done = 0;                                     // nodes written by the passes before this one
    for (int a0 = 0; a0 < n_in; a0 += kThreads) {
        const int a = a0 + threadIdx.x;
        const bool keep = a < n_in && flags[q.flag0 + a];
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) wave_n[wv] = __popcll(mask);
        __syncthreads();
        int before = 0, pass_total = 0;
        for (int w = 0; w < kWaves; ++w) {
            if (w < wv) before += wave_n[w];
            pass_total += wave_n[w];
        }
        const int node = n0 + done + before + __popcll(mask & ((1ull << lane) - 1ull));
        done += pass_total;
        __syncthreads();                              // wave_n is rewritten by the next pass
        if (!keep) continue;
        if (node >= n1) {                             // flags and counts disagree: never write past the sample's rows
            atomicOr(status, kBadCounts);
            continue;
        }
        const bool is_rec = a >= q.n_lig;
        const int src = is_rec ? q.rec0 + (a - q.n_lig) : q.lig0 + a;
        const double* p = (is_rec ? pool.rec_xyz : pool.lig_xyz) + 3 * (size_t)src;
        double c[3] = {p[0], p[1], p[2]};
        if (!is_rec && m) xform(m, p[0], p[1], p[2], c);
        if (pos_graph) {
            pos_graph[3 * (size_t)node] = (float)c[0];
            pos_graph[3 * (size_t)node + 1] = (float)c[1];
            pos_graph[3 * (size_t)node + 2] = (float)c[2];
        }
        double o[3] = {c[0], c[1], c[2]};
        if (r) xform(r, c[0], c[1], c[2], o);
        pos[3 * (size_t)node] = (float)o[0];
        pos[3 * (size_t)node + 1] = (float)o[1];
        pos[3 * (size_t)node + 2] = (float)o[2];
        bp[node] = is_rec;
        batch[node] = (BatchT)s;
        // class of the atom (data_loaders.py:288-291, preprocessing.py:275): receptor classes sit n_features higher
        int cls;
        if (enc.use_atomic_numbers) {
            const int z = (is_rec ? pool.rec_z : pool.lig_z)[src];
            cls = (z >= 0 && z < kLutSize) ? class_of_z[z] : enc.n_features;
        } else {
            cls = (is_rec ? pool.rec_types : pool.lig_types)[src];
        }
        cls += is_rec ? enc.n_features : 0;
        // make_bit_vector (preprocessing.py:214-239)
        int hot, last = 0;
        if (enc.compact) {
            hot = cls % enc.n_features;
            last = cls / enc.n_features;
        } else {
            hot = cls;
        }
        const int n_hot = enc.compact ? enc.n_features : enc.feature_dim;
        if (cls < 0 || hot < 0 || hot >= n_hot) {     // F.one_hot raises on these
            atomicOr(status, kBadType);
            hot = -1;
        }
        float* row = x + (size_t)node * enc.feature_dim;
        for (int k = 0; k < enc.feature_dim; ++k) row[k] = k == hot ? 1.0f : 0.0f;
        if (enc.compact) row[enc.n_features] = (float)last;
    }
}

// sorted position p of the batch's radius graph -> its place in the loader's list: graph by graph, the graph's inter
// block then its intra block, each row-major. perm (pvs_radius_graph_fill) counts the inter edges of ALL graphs first.
__global__ void k_complex_edges(int n_nodes, int n_edges, int n_graphs, const int32_t* __restrict__ graph_ptr,
                                const int32_t* __restrict__ rowptr, const int32_t* __restrict__ inter_ptr,
                                const int32_t* __restrict__ intra_ptr, const int32_t* __restrict__ row,
                                const int32_t* __restrict__ col, const uint8_t* __restrict__ etype,
                                const int32_t* __restrict__ perm, int64_t* __restrict__ edge_index,
                                int64_t* __restrict__ edge_attr, int32_t* __restrict__ status) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n_edges) return;
    const int i = row[p];
    const int lo = pvs_last_le(graph_ptr, n_graphs, i);      // (a row outside every graph fails the range check below)
    const int n0 = graph_ptr[lo], n1 = graph_ptr[lo + 1];
    bool ok = i >= 0 && i < n_nodes && n0 >= 0 && n0 <= i && i < n1 && n1 <= n_nodes;
    int dst = -1;
    if (ok) {
        const int n_inter_all = inter_ptr[n_nodes];
        const int q = perm[p];
        dst = rowptr[n0] + (q < n_inter_all ? q - inter_ptr[n0]
                                            : inter_ptr[n1] - inter_ptr[n0] + (q - n_inter_all - intra_ptr[n0]));
        ok = dst >= 0 && dst < n_edges;
    }
    if (!ok) {
        atomicOr(status, kBadEdges);
        return;
    }
    edge_index[dst] = i;
    edge_index[(size_t)n_edges + dst] = col[p];
    const int ty = etype[p];
    for (int k = 0; k < 3; ++k) edge_attr[3 * (size_t)dst + k] = k == ty;
}

// counts [B,2] -> node_ptr [B+1], their running sum, on the device (one wave; B is a few hundred at most). The sum is
// carried in 64 bits and saturates at INT32_MAX, so an offset never wraps. Sets the two bits a capacity batch adds on
// the node side: a sample without any atom left, more nodes than node_cap.
__global__ void k_node_offsets(const int32_t* __restrict__ counts, int B, int node_cap, int32_t* __restrict__ node_ptr,
                               int32_t* __restrict__ status) {
    const int lane = threadIdx.x;
    long long base = 0;
    int bits = 0;
    for (int g0 = 0; g0 < B; g0 += 64) {
        const int g = g0 + lane;
        const int n = g < B ? counts[2 * g] + counts[2 * g + 1] : 0;
        if (g < B && n <= 0) bits |= kNoAtomLeft;
        long long scan = n > 0 ? n : 0;
        for (int o = 1; o < 64; o <<= 1) {
            const long long t = __shfl_up(scan, o, 64);
            if (lane >= o) scan += t;
        }
        const long long end = base + scan;
        if (g < B) node_ptr[g + 1] = end > 0x7fffffffll ? 0x7fffffff : (int32_t)end;
        base += __shfl(scan, 63, 64);
    }
    if (lane == 0) node_ptr[0] = 0;
    if (base > node_cap) bits |= kNodeOverflow;
    if (bits) atomicOr(status, bits);
}

// Every row of the node tables that no sample owns - behind node_ptr[B], or inside a sample that does not fit node_cap
// and was therefore left out whole - is padding: zero features and coordinates, bp 0, node_graph -1. Together with
// k_complex_fill this rewrites every row at every call.
__global__ void k_pad_rows(const int32_t* __restrict__ node_ptr, int B, int node_cap, int feature_dim,
                           float* __restrict__ x, float* __restrict__ pos, float* __restrict__ pos_graph,
                           uint8_t* __restrict__ bp, int32_t* __restrict__ node_graph) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= node_cap) return;
    if (i < node_ptr[B]) {
        const int g = pvs_last_le(node_ptr, B, i);
        if (node_ptr[g + 1] <= node_cap) return;      // a row k_complex_fill writes
    }
    float* row = x + (size_t)i * feature_dim;
    for (int k = 0; k < feature_dim; ++k) row[k] = 0.0f;
    for (int k = 0; k < 3; ++k) {
        pos[3 * (size_t)i + k] = 0.0f;
        if (pos_graph) pos_graph[3 * (size_t)i + k] = 0.0f;
    }
    bp[i] = 0;
    node_graph[i] = -1;
}

bool pool_ok(const PvsComplexPool* pool) {
    return pool && pool->rec_xyz && pool->lig_xyz && pool->rec_types && pool->lig_types && pool->rec_z && pool->lig_z &&
           pool->rec_ptr && pool->lig_ptr && pool->n_rec > 0 && pool->n_lig > 0;
}

}  // namespace

// workspace = one flag byte per input atom of the batch (n_atoms_in = sum over the samples of ligand + receptor atoms)
extern "C" size_t pvs_complex_batch_workspace_bytes(int32_t n_samples, int32_t n_atoms_in) {
    (void)n_samples;
    return pvs_align_up((size_t)(n_atoms_in > 0 ? n_atoms_in : 0), 256) + 256;
}

extern "C" int pvs_complex_batch_count(const PvsComplexPool* pool, const int32_t* pairs, const double* lig_xform,
                                       int32_t n_samples, int32_t n_atoms_in, double radius, int32_t keep_hydrogens,
                                       int32_t* counts, int32_t* status, void* workspace, size_t workspace_bytes,
                                       pvs_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    const char* who = "pvs_complex_batch_count";
    PVS_REQUIRE(pool_ok(pool) && pairs && counts && status && workspace, "%s: NULL argument or empty pool", who);
    PVS_REQUIRE(n_samples > 0 && n_atoms_in >= 0, "%s: bad sizes B=%d atoms=%d", who, n_samples, n_atoms_in);
    PVS_REQUIRE(workspace_bytes >= pvs_complex_batch_workspace_bytes(n_samples, n_atoms_in),
                "%s: workspace too small (%zu)", who, workspace_bytes);
    PvsProfScope prof(s, PVS_PROF_PREPARE);
    PVS_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    k_complex_count<<<n_samples, kThreads, 0, s>>>(*pool, pairs, lig_xform, make_radius(radius), keep_hydrogens,
                                                   n_atoms_in, (uint8_t*)workspace, counts, status);
    PVS_CHECK_LAUNCH();
    return 0;
}

extern "C" int pvs_complex_batch_fill(const PvsComplexPool* pool, const int32_t* pairs, const double* lig_xform,
                                      const double* rot, int32_t n_samples, int32_t n_atoms_in, int32_t total_nodes,
                                      int32_t use_atomic_numbers, int32_t n_features, int32_t compact,
                                      const int32_t* class_of_z, const int32_t* counts, const int32_t* graph_ptr,
                                      float* x, float* pos, float* pos_graph, uint8_t* bp, int64_t* batch,
                                      int32_t* status, const void* workspace, size_t workspace_bytes,
                                      pvs_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    const char* who = "pvs_complex_batch_fill";
    PVS_REQUIRE(pool_ok(pool) && pairs && counts && graph_ptr && status && workspace, "%s: NULL argument or empty pool",
                who);
    PVS_REQUIRE(n_samples > 0 && n_atoms_in >= 0 && total_nodes >= 0, "%s: bad sizes", who);
    PVS_REQUIRE(n_features > 0 && (!use_atomic_numbers || class_of_z), "%s: bad feature encoding", who);
    PVS_REQUIRE(total_nodes == 0 || (x && pos && bp && batch), "%s: NULL output", who);
    PVS_REQUIRE(workspace_bytes >= pvs_complex_batch_workspace_bytes(n_samples, n_atoms_in),
                "%s: workspace too small (%zu)", who, workspace_bytes);
    PvsProfScope prof(s, PVS_PROF_PREPARE);
    Encoding enc;
    enc.use_atomic_numbers = use_atomic_numbers;
    enc.n_features = n_features;
    enc.compact = compact;
    enc.feature_dim = compact ? n_features + 1 : 2 * n_features;
    k_complex_fill<int64_t, false><<<n_samples, kThreads, 0, s>>>(
        *pool, pairs, lig_xform, rot, enc, class_of_z, n_atoms_in, (const uint8_t*)workspace, counts, graph_ptr,
        total_nodes, x, pos, pos_graph, bp, batch, status);
    PVS_CHECK_LAUNCH();
    return 0;
}

// _count, the offsets and _fill in one call at host-chosen capacities: nothing about the batch's content reaches the
// host, and the launch geometry depends on (n_samples, node_cap) alone, so the call can be captured.
extern "C" int pvs_complex_batch_build_cap(const PvsComplexPool* pool, const int32_t* pairs, const double* lig_xform,
                                           const double* rot, int32_t n_samples, int32_t atoms_in_cap, int32_t node_cap,
                                           double radius, int32_t keep_hydrogens, int32_t use_atomic_numbers,
                                           int32_t n_features, int32_t compact, const int32_t* class_of_z,
                                           int32_t* counts, int32_t* node_ptr, float* x, float* pos, float* pos_graph,
                                           uint8_t* bp, int32_t* node_graph, int32_t* status, void* workspace,
                                           size_t workspace_bytes, pvs_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    const char* who = "pvs_complex_batch_build_cap";
    PVS_REQUIRE(pool_ok(pool) && pairs && counts && node_ptr && status && workspace, "%s: NULL argument or empty pool",
                who);
    PVS_REQUIRE(n_samples > 0 && atoms_in_cap >= 0 && node_cap > 0, "%s: bad sizes B=%d atoms=%d nodes=%d", who,
                n_samples, atoms_in_cap, node_cap);
    PVS_REQUIRE(n_features > 0 && (!use_atomic_numbers || class_of_z), "%s: bad feature encoding", who);
    PVS_REQUIRE(x && pos && bp && node_graph, "%s: NULL output", who);
    PVS_REQUIRE(workspace_bytes >= pvs_complex_batch_workspace_bytes(n_samples, atoms_in_cap),
                "%s: workspace too small (%zu)", who, workspace_bytes);
    PvsProfScope prof(s, PVS_PROF_PREPARE);
    Encoding enc;
    enc.use_atomic_numbers = use_atomic_numbers;
    enc.n_features = n_features;
    enc.compact = compact;
    enc.feature_dim = compact ? n_features + 1 : 2 * n_features;
    PVS_CHECK_HIP(hipMemsetAsync(status, 0, sizeof(int32_t), s));
    k_complex_count<<<n_samples, kThreads, 0, s>>>(*pool, pairs, lig_xform, make_radius(radius), keep_hydrogens,
                                                   atoms_in_cap, (uint8_t*)workspace, counts, status);
    PVS_CHECK_LAUNCH();
    k_node_offsets<<<1, 64, 0, s>>>(counts, n_samples, node_cap, node_ptr, status);
    PVS_CHECK_LAUNCH();
    k_complex_fill<int32_t, true><<<n_samples, kThreads, 0, s>>>(
        *pool, pairs, lig_xform, rot, enc, class_of_z, atoms_in_cap, (const uint8_t*)workspace, counts, node_ptr,
        node_cap, x, pos, pos_graph, bp, node_graph, status);
    PVS_CHECK_LAUNCH();
    k_pad_rows<<<(node_cap + 255) / 256, 256, 0, s>>>(node_ptr, n_samples, node_cap, enc.feature_dim, x, pos, pos_graph,
                                                      bp, node_graph);
    PVS_CHECK_LAUNCH();
    return 0;
}

extern "C" int pvs_complex_edges(int32_t n_nodes, int32_t n_edges, int32_t n_graphs, const int32_t* graph_ptr,
                                 const int32_t* rowptr, const int32_t* inter_ptr, const int32_t* intra_ptr,
                                 const int32_t* row, const int32_t* col, const uint8_t* etype, const int32_t* perm,
                                 int64_t* edge_index, int64_t* edge_attr, int32_t* status, pvs_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    const char* who = "pvs_complex_edges";
    PVS_REQUIRE(n_nodes > 0 && n_graphs > 0 && n_edges >= 0, "%s: bad sizes", who);
    if (n_edges == 0) return 0;
    PVS_REQUIRE(graph_ptr && rowptr && inter_ptr && intra_ptr && row && col && etype && perm && edge_index &&
                edge_attr && status, "%s: NULL argument", who);
    PvsProfScope prof(s, PVS_PROF_PREPARE);
    k_complex_edges<<<(n_edges + 255) / 256, 256, 0, s>>>(n_nodes, n_edges, n_graphs, graph_ptr, rowptr, inter_ptr,
                                                          intra_ptr, row, col, etype, perm, edge_index, edge_attr,
                                                          status);
    PVS_CHECK_LAUNCH();
    return 0;
}
