// pvs_screen_graph_build: the radius graphs of B rigid poses of ONE ligand against ONE receptor
// (virtual screening) without testing the receptor-receptor pairs again: they
// are the same for every pose and come in as a template CSR (built once with pvs_radius_graph_*).
// Node layout per pose: the n_lig ligand atoms first, then the n_rec receptor atoms (so that inside
// a row "ligand columns then receptor columns" IS ascending column order). Same edges, classes and
// in-row order as generate_edges (/root/reference/point_vs/preprocessing/preprocessing.py:68-155):
//   inter block (class 1): ligand<->receptor pairs with 1e-7 < d < inter_radius
//   intra block: all pairs with 1e-7 < d < intra_radius: ligand-ligand and ligand-receptor (class 0),
//                receptor-receptor (class 2, from the template)
// Only the B * n_lig * n_rec ligand-receptor and B * n_lig^2 ligand-ligand distances are evaluated
// (fp64, cdist operation order). A ligand has 1..1024 atoms: its ligand-ligand contacts are W = ceil(n_lig / 64) mask
// words per atom, and every lane-per-ligand-atom step runs as W trips of the wave (one trip up to 64 atoms, the same
// instructions as when one word was all there was). Two CSRs come out, both with the edge count left on the device
// (their rowptr[N]; PvsGraph.n_edges_dev): the full graph, and its ligand-touching edges only (what
// the first layer runs over when the receptor-receptor sums are cached, pvs_egnn_layer_fwd_partial).
#include "common.h"
#include "profile.h"
#include "radius_common.h"
#include "screen_copies.h"
#include "screen_job.h"
#include "screen_slots.h"
#include <hipcub/hipcub.hpp>
#include <type_traits>

namespace {

typedef unsigned long long u64;

// Struck slots (PvsStruckSlots: a slot's receptor may lack one atom) run through the same kernels; what they do
// differently is compiled only for that layout.
template <class Slots> constexpr bool kStruck = std::is_same<Slots, PvsStruckSlots>::value;
// Cropped slots (PvsCroppedSlots: a slot's receptor is the subset its keep mask names) likewise. Their builder writes
// the full CSR only: what concerns the ligand-touching CSR is compiled out for that layout.
template <class Slots> constexpr bool kCropped = std::is_same<Slots, PvsCroppedSlots>::value;

// wave per packed ligand atom q: contact masks against the receptor (64 atoms per word) and the atom's own ligand
// (W words per atom; trip w, lane l: the slot's atom 64 w + l)
template <class Slots>
__global__ void __launch_bounds__(256)
k_contacts(const float* __restrict__ lig_pos, const float* __restrict__ rec_pos, Slots L, Radius r_inter,
           Radius r_intra, Radius r_zero, u64* __restrict__ m_inter, u64* __restrict__ m_intra,
           u64* __restrict__ m_ll, int32_t* __restrict__ clear_status) {
    const int lane = threadIdx.x & 63;
    const int q = (blockIdx.x * 256 + threadIdx.x) >> 6;
    // (the status word of this build is cleared here, by a plain store of the call's first kernel, and not by a 4-byte
    // memset ahead of it: in a replayed hipGraph that memset node has left the word filled with one arbitrary byte,
    // 0x14141414 or 0x2c2c2c2c, which check() then read as an overflow or a bad table)
    if (clear_status && blockIdx.x == 0 && threadIdx.x == 0) *clear_status = 0;
    if (q >= L.atoms()) return;
    const PvsSlotAtom slot = L.atom(q);
    if (!slot.valid) return;
    const int n_rec = L.n_rec, n_chunks = (n_rec + 63) / 64;
    int drop = -1;                                       // the receptor atom this atom's slot lacks: no contact with it
    if constexpr (kStruck<Slots>) drop = L.drop_of_atom(q);
    const float* la = lig_pos + (size_t)q * 3;
    const double xa = la[0], ya = la[1], za = la[2];
    for (int c = 0; c < n_chunks; ++c) {
        const int i = 64 * c + lane;
        bool ei = false, ea = false;
        if (i < n_rec && (!kStruck<Slots> || i != drop)) {
            const double s = pvs_sqdist(xa, ya, za, (double)rec_pos[3 * i], (double)rec_pos[3 * i + 1],
                                        (double)rec_pos[3 * i + 2]);
            if (above(s, r_zero)) {
                ei = below(s, r_inter);
                ea = below(s, r_intra);
            }
        }
        u64 bi = __ballot(ei), ba = __ballot(ea);
        if constexpr (kCropped<Slots>) {                  // contacts with the slot's kept atoms only
            const u64 kw = L.keep_word_of_atom(q, c);
            bi &= kw;
            ba &= kw;
        }
        if (lane == 0) {
            m_inter[(size_t)q * n_chunks + c] = bi;
            m_intra[(size_t)q * n_chunks + c] = ba;
        }
    }
    const int W = L.words();
    for (int w = 0; w < W; ++w) {
        const int b = 64 * w + lane;
        bool ell = false;
        if (b < slot.n_lig) {
            const float* lb = lig_pos + (size_t)(slot.a0 + b) * 3;
            const double s = pvs_sqdist(xa, ya, za, (double)lb[0], (double)lb[1], (double)lb[2]);
            ell = above(s, r_zero) && below(s, r_intra);
        }
        const u64 bl = __ballot(ell);
        if (lane == 0) m_ll[(size_t)q * W + w] = bl;
    }
}

__device__ __forceinline__ int row_popc(const u64* __restrict__ m, int n_chunks) {
    int c = 0;
    for (int k = 0; k < n_chunks; ++k) c += __popcll(m[k]);
    return c;
}

// thread per row (and one past the end): degree in the full graph and in the ligand-touching subgraph (a receptor
// row walks the slot's ligand atoms one by one: linear in n_lig)
template <class Slots>
__global__ void k_degrees(const u64* __restrict__ m_inter, const u64* __restrict__ m_intra,
                          const u64* __restrict__ m_ll, const int32_t* __restrict__ rr_rowptr,
                          const int32_t* __restrict__ rr_col, Slots L, int32_t* __restrict__ deg,
                          int32_t* __restrict__ deg_l) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > L.rows()) return;
    PvsSlotRow r = {};
    if (g < L.rows()) r = L.row(g);
    if (!r.valid) {
        deg[g] = 0;
        if constexpr (!kCropped<Slots>) deg_l[g] = 0;
        return;
    }
    const int n_chunks = (L.n_rec + 63) / 64;
    if (r.local < r.n_lig) {
        const size_t w = (size_t)r.a0 + r.local;
        const int W = L.words();
        const int d = row_popc(m_inter + w * n_chunks, n_chunks) + row_popc(m_ll + w * W, W) +
                      row_popc(m_intra + w * n_chunks, n_chunks);
        deg[g] = d;
        if constexpr (!kCropped<Slots>) deg_l[g] = d;
    } else {
        int i = r.local - r.n_lig;
        if constexpr (kStruck<Slots>) i = pvs_struck_receptor(i, r.drop);
        if constexpr (kCropped<Slots>) i = L.receptor(r.slot, i);
        const int c = i >> 6;
        const u64 bit = 1ull << (i & 63);
        int nl = 0;
        for (int a = 0; a < r.n_lig; ++a) {
            const size_t w = (size_t)r.a0 + a;
            nl += (m_inter[w * n_chunks + c] & bit) ? 1 : 0;
            nl += (m_intra[w * n_chunks + c] & bit) ? 1 : 0;
        }
        int rr = rr_rowptr[i + 1] - rr_rowptr[i];
        bool touched = false;           // a struck slot's row that had the struck atom as a neighbour: the whole row
        if constexpr (kStruck<Slots>) {  // goes through the ligand-touching CSR too
            touched = r.drop >= 0 && pvs_find_ascending(rr_col + rr_rowptr[i], rr, r.drop) >= 0;
            rr -= touched ? 1 : 0;
        }
        if constexpr (kCropped<Slots>) {                  // the template neighbours that the slot keeps
            const int r0 = rr_rowptr[i], n = rr;
            rr = 0;
            for (int k = 0; k < n; ++k) rr += L.kept(r.slot, rr_col[r0 + k]) ? 1 : 0;
        } else {
            deg_l[g] = touched ? nl + rr : nl;
        }
        deg[g] = nl + rr;
    }
}

struct OutCsr {
    const int32_t* rowptr;
    int32_t *row, *col;
    uint8_t* etype;
    int capacity;
};

// wave per row: writes the row's segment of the full CSR and of the ligand-touching CSR
template <class Slots>
__global__ void __launch_bounds__(256)
k_fill(const u64* __restrict__ m_inter, const u64* __restrict__ m_intra, const u64* __restrict__ m_ll,
       const int32_t* __restrict__ rr_rowptr, const int32_t* __restrict__ rr_col, Slots L, OutCsr full, OutCsr lig,
       float* __restrict__ inv_deg, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int g = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const int N = L.rows();
    if (g >= N) return;
    if constexpr (kCropped<Slots>) {
        if (full.rowptr[N] > full.capacity) {
            if (g == 0 && lane == 0) *status |= 4;        // (the word's one writer in this launch)
            return;
        }
    } else if (full.rowptr[N] > full.capacity || lig.rowptr[N] > lig.capacity) {
        if (g == 0 && lane == 0) atomicOr(status, 4);
        return;
    }
    const PvsSlotRow r = L.row(g);
    if (!r.valid) {                                       // padding row (or no valid table: an empty graph)
        if (lane == 0) inv_deg[g] = 1.0f;
        return;
    }
    const int n_lig = r.n_lig, node0 = r.node0;
    const int n_chunks = (L.n_rec + 63) / 64, W = L.words();
    const int trips = pvs_slot_words(n_lig);               // the words that this slot's atoms reach (<= W)
    const u64 lower = (1ull << lane) - 1ull;
    int pf = full.rowptr[g], pl = 0;
    if constexpr (!kCropped<Slots>) pl = lig.rowptr[g];
    if (lane == 0) {
        const int d = full.rowptr[g + 1] - pf;
        inv_deg[g] = 1.0f / (float)(d > 1 ? d : 1);
    }
    auto emit = [&](int off, int column, int cls, bool also_lig) {
        full.row[pf + off] = g; full.col[pf + off] = column; full.etype[pf + off] = (uint8_t)cls;
        if constexpr (!kCropped<Slots>) {
            if (also_lig) { lig.row[pl + off] = g; lig.col[pl + off] = column; lig.etype[pl + off] = (uint8_t)cls; }
        }
    };
    auto expand_words = [&](const u64* __restrict__ m, int col0, int cls) {
        const int done = pvs_expand_mask_row(m, n_chunks, lane, [&](int k, int b) {
            if constexpr (kStruck<Slots>) b = pvs_struck_row(b, r.drop);
            if constexpr (kCropped<Slots>) b = L.receptor_row(r.slot, b);     // (the masks hold kept atoms only)
            emit(k, col0 + b, cls, true);
        });
        pf += done;
        pl += done;
    };
    if (r.local < n_lig) {
        const size_t w = (size_t)r.a0 + r.local;
        expand_words(m_inter + w * n_chunks, node0 + n_lig, 1);             // inter block: receptor atoms
        {                                                                     // intra block: ligand atoms ...
            const u64* mll = m_ll + w * W;
            for (int t = 0; t < trips; ++t) {
                if ((mll[t] >> lane) & 1ull) emit(pvs_mask_rank(mll, t, lane), node0 + 64 * t + lane, 0, true);
            }
            const int c = row_popc(mll, W);
            pf += c; pl += c;
        }
        expand_words(m_intra + w * n_chunks, node0 + n_lig, 0);              // ... then receptor atoms
    } else {
        int i = r.local - n_lig;
        if constexpr (kStruck<Slots>) i = pvs_struck_receptor(i, r.drop);
        if constexpr (kCropped<Slots>) i = L.receptor(r.slot, i);
        const int c = i >> 6;
        const u64 bit = 1ull << (i & 63);
        for (int kind = 0; kind < 2; ++kind) {                                // inter block, then intra: ligand atoms
            const u64* m = kind == 0 ? m_inter : m_intra;
            int cnt = 0;
            for (int t = 0; t < trips; ++t) {                                 // (trip t: the slot's atoms 64 t ..)
                const int a = 64 * t + lane;
                const bool on = a < n_lig && (m[((size_t)r.a0 + a) * n_chunks + c] & bit);
                const u64 b = __ballot(on);
                if (on) emit(cnt + __popcll(b & lower), node0 + a, kind == 0 ? 1 : 0, true);
                cnt += __popcll(b);
            }
            pf += cnt; pl += cnt;
        }
        const int r0 = rr_rowptr[i], r1 = rr_rowptr[i + 1];                   // intra block: receptor atoms
        if constexpr (kCropped<Slots>) {   // the template neighbours that the slot keeps, renumbered by their rank
            int cnt = 0;
            for (int k0 = 0; k0 < r1 - r0; k0 += 64) {
                const int k = k0 + lane;
                const int j = k < r1 - r0 ? rr_col[r0 + k] : -1;
                const bool on = j >= 0 && L.kept(r.slot, j);
                const u64 b = __ballot(on);
                if (on) emit(cnt + __popcll(b & lower), node0 + n_lig + L.receptor_row(r.slot, j), 2, false);
                cnt += __popcll(b);
            }
        } else if (!kStruck<Slots> || r.drop < 0) {
            for (int k = lane; k < r1 - r0; k += 64) emit(k, node0 + n_lig + rr_col[r0 + k], 2, false);
        } else {                        // without the struck atom; a row that had it is written to both CSRs
            const int at = pvs_find_ascending(rr_col + r0, r1 - r0, r.drop);
            for (int k = lane; k < r1 - r0; k += 64) {
                if (k == at) continue;
                emit(k - ((at >= 0 && k > at) ? 1 : 0), node0 + n_lig + pvs_struck_row(rr_col[r0 + k], r.drop), 2,
                     at >= 0);
            }
        }
    }
}

// the builder's scratch: contact masks per packed atom (n_chunks receptor words each, `words` ligand words), degrees
// per row; slot_of (atom -> slot) for the ragged layout; keep_rank (crop_slots slots of n_chunks + 1 entries) for the
// cropped layout, which has no second degree table
struct ScreenState {
    u64 *m_inter, *m_intra, *m_ll;
    int32_t *deg, *deg_l, *slot_of, *keep_rank;
    void* scan_tmp;
    size_t scan_bytes;
};

size_t carve_screen(PvsArena& a, size_t atoms, int rows, int n_rec, int words, bool ragged, ScreenState* out,
                    int crop_slots = 0) {
    ScreenState t;
    const size_t n_chunks = (size_t)(n_rec + 63) / 64;
    t.m_inter = a.take<u64>(atoms * n_chunks);
    t.m_intra = a.take<u64>(atoms * n_chunks);
    t.m_ll = a.take<u64>(atoms * (size_t)words);
    t.slot_of = ragged ? a.take<int32_t>(atoms) : nullptr;
    t.deg = a.take<int32_t>((size_t)rows + 1);
    t.deg_l = crop_slots ? nullptr : a.take<int32_t>((size_t)rows + 1);
    t.keep_rank = crop_slots ? a.take<int32_t>((size_t)crop_slots * (n_chunks + 1)) : nullptr;
    size_t sb = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, sb, (const int32_t*)nullptr, (int32_t*)nullptr, rows + 1);
    t.scan_bytes = sb;
    t.scan_tmp = a.take<char>(sb);
    if (out) *out = t;
    return a.off;
}

// contacts -> degrees -> the two row pointers (rowptr, rowptr_lig: what full.rowptr / lig.rowptr read) -> fill, for
// either layout
template <class Slots>
int build_csrs(const Slots& L, const float* lig_pos, const float* rec_pos, const int32_t* rr_rowptr,
               const int32_t* rr_col, double inter_radius, double intra_radius, int32_t* rowptr, int32_t* rowptr_lig,
               OutCsr full, OutCsr lig, float* inv_deg, int32_t* status, bool clear_status, const ScreenState& w,
               hipStream_t s) {
    const int N = L.rows();
    k_contacts<<<(L.atoms() + 3) / 4, 256, 0, s>>>(lig_pos, rec_pos, L, make_radius(inter_radius),
                                                   make_radius(intra_radius), make_radius(1e-7), w.m_inter,
                                                   w.m_intra, w.m_ll, clear_status ? status : nullptr);
    PVS_CHECK_LAUNCH();
    k_degrees<<<(N + 1 + 255) / 256, 256, 0, s>>>(w.m_inter, w.m_intra, w.m_ll, rr_rowptr, rr_col, L, w.deg, w.deg_l);
    PVS_CHECK_LAUNCH();
    size_t sb = w.scan_bytes;
    PVS_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(w.scan_tmp, sb, w.deg, rowptr, N + 1, s));
    if constexpr (!kCropped<Slots>) {
        sb = w.scan_bytes;
        PVS_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(w.scan_tmp, sb, w.deg_l, rowptr_lig, N + 1, s));
    }
    k_fill<<<(N + 3) / 4, 256, 0, s>>>(w.m_inter, w.m_intra, w.m_ll, rr_rowptr, rr_col, L, full, lig, inv_deg, status);
    PVS_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" size_t pvs_screen_graph_state_bytes(int32_t B, int32_t n_lig, int32_t n_rec) {
    PvsArena a(nullptr, 0);
    const PvsUniformSlots L{B, n_lig, n_rec};
    return carve_screen(a, (size_t)L.atoms(), L.rows(), n_rec, L.words(), false, nullptr) + 256;
}

extern "C" int pvs_screen_graph_build(const float* lig_pos, const float* rec_pos, const int32_t* rr_rowptr,
                                      const int32_t* rr_col, int32_t B, int32_t n_lig, int32_t n_rec,
                                      double inter_radius, double intra_radius, int32_t capacity,
                                      int32_t capacity_lig, int32_t* rowptr, int32_t* row, int32_t* col,
                                      uint8_t* etype, float* inv_deg, int32_t* rowptr_lig, int32_t* row_lig,
                                      int32_t* col_lig, uint8_t* etype_lig, int32_t* status, void* state,
                                      size_t state_bytes, pvs_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    PVS_REQUIRE(lig_pos && rec_pos && rr_rowptr && rr_col && rowptr && row && col && etype && inv_deg &&
                rowptr_lig && row_lig && col_lig && etype_lig && status && state, "pvs_screen_graph_build: NULL");
    PVS_REQUIRE(B > 0 && n_lig > 0 && n_lig <= kPvsMaxSlotCap && n_rec > 0, "pvs_screen_graph_build: needs 1..%d "
                "ligand atoms (n_lig: got %d) and a receptor", kPvsMaxSlotCap, n_lig);
    const PvsUniformSlots L{B, n_lig, n_rec};
    PvsArena arena(state, state_bytes);
    ScreenState w;
    carve_screen(arena, (size_t)L.atoms(), L.rows(), n_rec, L.words(), false, &w);
    PVS_REQUIRE(arena.ok(), "pvs_screen_graph_build: state too small (%zu < %zu)", state_bytes, arena.off);
    PvsProfScope prof(s, PVS_PROF_PREPARE);
    return build_csrs(L, lig_pos, rec_pos, rr_rowptr, rr_col, inter_radius, intra_radius, rowptr, rowptr_lig,
                      OutCsr{rowptr, row, col, etype, capacity},
                      OutCsr{rowptr_lig, row_lig, col_lig, etype_lig, capacity_lig}, inv_deg, status, true, w, s);
}

// ---- library batches: every slot of the batch holds one pose of ANY ligand of 0..slot_cap atoms ----
// pvs_screen_slots_build (PvsScreenSlotsJob, layout PVS_SLOTS_RAGGED): the same graphs for a batch whose B slots hold
// poses of different ligands (a docking library: thousands of ligands of 8-60 atoms with ~10 poses each). The ligand atoms
// come packed, lig_pos [L_cap,3] with the device table lig_ptr [B+1]; slot p has lig_ptr[p+1]-lig_ptr[p]
// atoms (0 = receptor only). Compact node layout: slot p owns nodes node_ptr[p] .. node_ptr[p+1],
// node_ptr[p] = lig_ptr[p] + p * n_rec, ligand atoms first, then the receptor; the nodes from node_ptr[B]
// up to N_cap = L_cap + B * n_rec are padding (degree 0, inv_deg 1, graph id -1). No host argument depends
// on the batch's composition, so one captured step serves every batch of a library. The masks are indexed by
// the packed atom (same words as above), node -> slot by bisection of node_ptr, atom -> slot by a table that
// the first kernel fills; the node tables of the layer stack (graph id, pos, features, first-layer receptor
// sums) are expanded by a sibling kernel of the same call. The kernels above run on either layout (screen_slots.h:
// PvsUniformSlots, PvsRaggedSlots); only k_slots and k_node_tables_ragged are the ragged builder's own.
namespace {

// thread per slot: validates the slot, node_ptr, atom -> slot table. The thread behind the last slot walks the whole
// table once more and STORES the build's status word (0 or kPvsBadTable): the word's one writer in this kernel, so no
// clearing launch or memset has to come before it (k_contacts: why not a memset).
__global__ void k_slots(const int32_t* __restrict__ lig_ptr, int B, int L_cap, int n_rec, int slot_cap,
                        int32_t* __restrict__ node_ptr, int32_t* __restrict__ slot_of,
                        int32_t* __restrict__ status) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > B) return;
    if (p == B) {
        const int t = lig_ptr[B];
        node_ptr[B] = (t >= 0 && t <= L_cap) ? t + B * n_rec : B * n_rec;
        bool bad = lig_ptr[0] != 0;
        for (int k = 0; k < B; ++k) {
            const int a0 = lig_ptr[k], a1 = lig_ptr[k + 1];
            bad = bad || a0 < 0 || a1 < a0 || a1 - a0 > slot_cap || a1 > L_cap;
        }
        *status = bad ? kPvsBadTable : 0;
        return;
    }
    const int a0 = lig_ptr[p], a1 = lig_ptr[p + 1];
    if (a0 < 0 || a1 < a0 || a1 - a0 > slot_cap || a1 > L_cap) {
        node_ptr[p] = p * n_rec;
        return;
    }
    node_ptr[p] = a0 + p * n_rec;
    for (int q = a0; q < a1; ++q) slot_of[q] = p;
}

// k_slots for struck slots (PVS_SLOTS_STRUCK; screen_slots.h: PvsStruckSlots): the same with rec_drop [B], -1 or the
// receptor atom that the slot's receptor lacks. A struck slot has one row less, so node_ptr[p] also counts the
// struck slots before p (a walk over the table per thread: B is a batch size); an entry of rec_drop outside
// -1..n_rec-1 makes the whole table bad: *status bit 3 and an edgeless batch, as for a bad lig_ptr. The slot's graph is
// what the reference's masking leaves of the unstruck slot's graph: the atom and every edge that touches it are gone,
// the ids above it move down by one, classes and in-row order stay. A receptor row that had the atom as a template
// neighbour can no longer start from the receptor's cached first-layer sums: its base is zero and its WHOLE row (ligand
// entries, then the class-2 entries that remain) is in the ligand-touching CSR, which is all
// pvs_egnn_layer_fwd_partial needs.
__global__ void k_slots_struck(const int32_t* __restrict__ lig_ptr, const int32_t* __restrict__ rec_drop, int B,
                               int L_cap, int n_rec, int slot_cap, int32_t* __restrict__ node_ptr,
                               int32_t* __restrict__ slot_of, int32_t* __restrict__ status) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p > B) return;
    int struck = 0;
    for (int k = 0; k < p; ++k) struck += rec_drop[k] >= 0 ? 1 : 0;
    if (p == B) {
        const int t = lig_ptr[B];
        bool bad = lig_ptr[0] != 0;
        for (int k = 0; k < B; ++k) {
            const int a0 = lig_ptr[k], a1 = lig_ptr[k + 1];
            bad = bad || a0 < 0 || a1 < a0 || a1 - a0 > slot_cap || a1 > L_cap || !pvs_rec_drop_ok(rec_drop[k], n_rec);
        }
        node_ptr[B] = bad ? B * n_rec : t + B * n_rec - struck;
        *status = bad ? kPvsBadTable : 0;
        return;
    }
    const int a0 = lig_ptr[p], a1 = lig_ptr[p + 1];
    if (a0 < 0 || a1 < a0 || a1 - a0 > slot_cap || a1 > L_cap) {
        node_ptr[p] = p * n_rec;
        return;
    }
    node_ptr[p] = a0 + p * n_rec - struck;
    for (int q = a0; q < a1; ++q) slot_of[q] = p;
}

// wave per node: graph id, coordinates and (with tables) the feature row and the first-layer receptor sums (zero for
// a struck slot's row that had the struck atom as a neighbour: its whole row is in the ligand-touching CSR)
template <class Slots>
__global__ void __launch_bounds__(256)
k_node_tables_ragged(const float* __restrict__ lig_pos, const float* __restrict__ rec_pos, Slots L,
                     const int32_t* __restrict__ rr_rowptr, const int32_t* __restrict__ rr_col,
                     int32_t* __restrict__ node_graph, float* __restrict__ pos, PvsRaggedNodeTables t) {
    const int lane = threadIdx.x & 63;
    const int g = (blockIdx.x * 256 + threadIdx.x) >> 6;
    if (g >= L.rows()) return;
    const int F = t.n_feats, H = t.hidden;
    const PvsSlotRow r = L.row(g);
    int lig_row = -1, rec_row = -1;                        // padding: every table zero
    if (r.valid) {
        if (r.local < r.n_lig) lig_row = r.a0 + r.local; else rec_row = r.local - r.n_lig;
    }
    if constexpr (kCropped<Slots>) {                      // (the k-th kept atom; the cropped builder has no base tables)
        if (rec_row >= 0) rec_row = L.receptor(r.slot, rec_row);
    }
    bool based = rec_row >= 0;                            // the row starts from the receptor's cached sums
    if constexpr (kStruck<Slots>) {
        if (rec_row >= 0) rec_row = pvs_struck_receptor(rec_row, r.drop);
        if (rec_row >= 0 && r.drop >= 0 && t.base_magg) {
            const int r0 = rr_rowptr[rec_row];
            based = pvs_find_ascending(rr_col + r0, rr_rowptr[rec_row + 1] - r0, r.drop) < 0;
        }
    }
    if (lane == 0) node_graph[g] = r.slot;
    if (lane < 3) {
        pos[(size_t)g * 3 + lane] = lig_row >= 0 ? lig_pos[(size_t)lig_row * 3 + lane]
                                  : rec_row >= 0 ? rec_pos[(size_t)rec_row * 3 + lane] : 0.0f;
    }
    if (t.feats) {
        const float* src = lig_row >= 0 ? t.lig_feats + (size_t)lig_row * F
                         : rec_row >= 0 ? t.rec_feats + (size_t)rec_row * F : nullptr;
        for (int c = lane; c < F; c += 64) t.feats[(size_t)g * F + c] = src ? src[c] : 0.0f;
    }
    if (t.base_magg) {
        for (int c = lane; c < H; c += 64)
            t.base_magg[(size_t)g * H + c] = based ? t.rec_magg[(size_t)rec_row * H + c] : 0.0f;
        if (lane < 3) t.base_xsum[(size_t)g * 3 + lane] = based ? t.rec_xsum[(size_t)rec_row * 3 + lane] : 0.0f;
        if (lane == 0) t.base_deg[g] = based ? t.rec_deg[rec_row] : 0.0f;
    }
}

}  // namespace

// ---- cropped slots (PVS_SLOTS_CROPPED): the ragged builder where every slot keeps only the receptor atoms closer than
// crop_radius to one of its ligand atoms (screen_slots.h: PvsCroppedSlots), as the training loader crops a complex
// around its ligand. k_crop_keep decides the masks, k_crop_slots turns them into ranks and node offsets; the kernels
// above then run on the layout: a ligand atom's contact masks are cut down to the kept atoms, a receptor row is the
// k-th kept atom (select), a receptor column the rank of its atom, and the template's receptor-receptor edges go in
// where both ends are kept - no distance is evaluated for them. Only the full CSR is written. No atomics anywhere:
// every word has one writer, so a build gives the same bits on every run. ----
namespace {

// The atoms a0 .. a1 of a packed table of `cap` rows, or none where the pair is no set of at most set_cap atoms of a
// valid table.
__device__ __forceinline__ bool crop_slot_ok(int a0, int a1, int cap, int set_cap) {
    return a0 >= 0 && a1 >= a0 && a1 - a0 <= set_cap && a1 <= cap;
}

// Which atoms the slots are cropped AROUND: the rows ptr[p] .. ptr[p + 1] of pos [cap, 3], at most set_cap (<=
// kPvsMaxSlotCap) per slot, and, with `drop`, the receptor atom drop[p] that slot p lacks whatever the crop says (-1:
// none). pvs_screen_slots_build: the slot's own ligand atoms and no drop; pvs_screen_copies_build: the job's crop table
// (a leave-out copy's parent) and its rec_drop; pvs_crop_keep: packed hits.
struct CropSets {
    const float* pos;
    const int32_t *ptr, *drop;
    int cap, set_cap;
};

// THE keep decision, its one copy. block (p, y): the slot's crop set staged in LDS; wave w of the block takes the mask
// word 4 y + w: lane l decides receptor atom 64 (4 y + w) + l against every staged atom (fp64 on the fp32 coordinates,
// strict, no lower bound: a coincident atom is kept), then the dropped bit, one ballot per word. An empty or invalid
// set keeps nothing.
__global__ void __launch_bounds__(256)
k_crop_keep(CropSets from, const float* __restrict__ rec_pos, int n_rec, Radius r_crop, u64* __restrict__ keep) {
    __shared__ float lig[3 * kPvsMaxSlotCap];
    const int p = blockIdx.x, lane = threadIdx.x & 63;
    const int W = pvs_rec_words(n_rec), c = 4 * blockIdx.y + (threadIdx.x >> 6);
    const int a0 = from.ptr[p], a1 = from.ptr[p + 1];
    const int n = crop_slot_ok(a0, a1, from.cap, from.set_cap) ? a1 - a0 : 0;       // (<= set_cap <= kPvsMaxSlotCap)
    for (int t = threadIdx.x; t < 3 * n; t += 256) lig[t] = from.pos[(size_t)a0 * 3 + t];
    __syncthreads();
    if (c >= W) return;
    const int i = 64 * c + lane;
    bool in = false;
    if (i < n_rec) {
        const double xr = rec_pos[3 * i], yr = rec_pos[3 * i + 1], zr = rec_pos[3 * i + 2];
        for (int a = 0; a < n && !in; ++a)
            in = below(pvs_sqdist((double)lig[3 * a], (double)lig[3 * a + 1], (double)lig[3 * a + 2], xr, yr, zr), r_crop);
        if (from.drop) in = in && i != from.drop[p];
    }
    const u64 b = __ballot(in);
    if (lane == 0) keep[(size_t)p * W + c] = b;
}

// ONE block. First every slot's ranks (thread per slot: keep_rank[p, w] = the kept atoms before word w, entry W the
// slot's count) and its verdict on lig_ptr - and, for copies (crop.ptr set), on the crop table and rec_drop; behind the
// barrier the node offsets (thread p adds the counts of the slots before it: B is a batch size), the atom -> slot table
// and the status word, STORED as in k_slots: this kernel stays the word's one writer for copies too. A table that is
// not one: every offset 0 and kPvsBadTable, an edgeless batch of padding rows.
__global__ void __launch_bounds__(256)
k_crop_slots(const int32_t* __restrict__ lig_ptr, CropSets crop, const u64* __restrict__ keep, int B, int L_cap,
             int n_rec, int slot_cap, int32_t* __restrict__ keep_rank, int32_t* __restrict__ node_ptr,
             int32_t* __restrict__ slot_of, int32_t* __restrict__ status) {
    __shared__ int bad;
    const int W = pvs_rec_words(n_rec);
    if (threadIdx.x == 0) bad = (lig_ptr[0] != 0 || (crop.ptr && crop.ptr[0] != 0)) ? 1 : 0;
    __syncthreads();
    for (int p = threadIdx.x; p < B; p += 256) {
        if (!crop_slot_ok(lig_ptr[p], lig_ptr[p + 1], L_cap, slot_cap)) bad = 1;     // (every writer stores the same 1)
        if (crop.ptr && !crop_slot_ok(crop.ptr[p], crop.ptr[p + 1], crop.cap, crop.set_cap)) bad = 1;
        if (crop.drop && !pvs_rec_drop_ok(crop.drop[p], n_rec)) bad = 1;
        int32_t* rank = keep_rank + (size_t)p * (W + 1);
        int before = 0;
        for (int w = 0; w < W; ++w) {
            rank[w] = before;
            before += __popcll(keep[(size_t)p * W + w]);
        }
        rank[W] = before;
    }
    __syncthreads();
    const bool ok = !bad;
    for (int p = threadIdx.x; p <= B; p += 256) {
        int rows = 0;
        if (ok) {
            rows = lig_ptr[p];
            for (int k = 0; k < p; ++k) rows += keep_rank[(size_t)k * (W + 1) + W];
        }
        node_ptr[p] = rows;
        if (p == B) *status = ok ? 0 : kPvsBadTable;
        else if (ok) for (int q = lig_ptr[p]; q < lig_ptr[p + 1]; ++q) slot_of[q] = p;
    }
}

// pvs_crop_keep's second launch, ONE block: kept_ptr [S + 1] <- the exclusive scan of the hits' kept counts (thread t
// owns a contiguous run of hits, as k_contact_scan of leave_out.hip). A lig_ptr that is no table of hits of at most
// kPvsMaxSlotCap atoms inside n_rows: keep and kept_ptr zero, kept_ptr[S] = -1.
__global__ void __launch_bounds__(256)
k_crop_keep_scan(const int32_t* __restrict__ lig_ptr, int S, int n_rows, int W, u64* __restrict__ keep,
                 int32_t* __restrict__ kept_ptr) {
    __shared__ long long part[256];
    const int tid = threadIdx.x, per = (S + 255) / 256;
    const int lo = min(S, tid * per), hi = min(S, lo + per);
    int bad = tid == 0 && lig_ptr[0] != 0;
    long long sum = 0;
    for (int s = lo; s < hi; ++s) {
        bad |= !crop_slot_ok(lig_ptr[s], lig_ptr[s + 1], n_rows, kPvsMaxSlotCap);
        for (int w = 0; w < W; ++w) sum += __popcll(keep[(size_t)s * W + w]);
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
        kept_ptr[s] = bad ? 0 : (int32_t)at;
        for (int w = 0; w < W; ++w) {
            at += __popcll(keep[(size_t)s * W + w]);
            if (bad) keep[(size_t)s * W + w] = 0;
        }
    }
    if (tid == 0) kept_ptr[S] = bad ? -1 : (int32_t)total;
}

// ---- the host path of all three layouts: check (screen_job.h), carve, then the layout's own first launch(es) and the
// shared sequence behind them ----
size_t carve_job(PvsArena& a, const PvsScreenSlotsJob& j, ScreenState* out) {
    return carve_screen(a, (size_t)j.lig_cap, j.lig_cap + j.n_slots * j.n_rec, j.n_rec, pvs_slot_words(j.slot_cap),
                        true, out, j.layout == PVS_SLOTS_CROPPED ? j.n_slots : 0);
}

// The layout's first launch(es): they validate the slot table and write node_ptr, the atom -> slot table and the status
// word, and leave in *L the layout that the kernels behind them read.
int start_slots(const PvsScreenSlotsJob& j, const ScreenState& w, hipStream_t s, PvsRaggedSlots* L) {
    *L = PvsRaggedSlots{j.lig_ptr, j.node_ptr, w.slot_of, j.status, j.n_slots, j.lig_cap, j.n_rec, j.slot_cap};
    k_slots<<<(j.n_slots + 1 + 255) / 256, 256, 0, s>>>(j.lig_ptr, j.n_slots, j.lig_cap, j.n_rec, j.slot_cap,
                                                         j.node_ptr, w.slot_of, j.status);
    PVS_CHECK_LAUNCH();
    return 0;
}

int start_slots(const PvsScreenSlotsJob& j, const ScreenState& w, hipStream_t s, PvsStruckSlots* L) {
    *L = PvsStruckSlots{j.lig_ptr, j.node_ptr, w.slot_of, j.status, j.rec_drop, j.n_slots, j.lig_cap, j.n_rec,
                        j.slot_cap};
    k_slots_struck<<<(j.n_slots + 1 + 255) / 256, 256, 0, s>>>(j.lig_ptr, j.rec_drop, j.n_slots, j.lig_cap, j.n_rec,
                                                                j.slot_cap, j.node_ptr, w.slot_of, j.status);
    PVS_CHECK_LAUNCH();
    return 0;
}

// Cropped slots. crop: nullptr for slots cropped around their own ligand atoms (pvs_screen_slots_build), else the
// crop table and rec_drop of pvs_screen_copies_build - the same two launches either way.
int start_slots(const PvsScreenSlotsJob& j, const ScreenState& w, hipStream_t s, PvsCroppedSlots* L,
                const CropSets* crop = nullptr) {
    const int W = pvs_rec_words(j.n_rec);
    u64* keep = (u64*)j.keep;
    *L = PvsCroppedSlots{j.lig_ptr, j.node_ptr, w.slot_of, j.status, keep, w.keep_rank, j.n_slots, j.lig_cap, j.n_rec,
                         j.slot_cap};
    const CropSets own{j.lig_pos, j.lig_ptr, nullptr, j.lig_cap, j.slot_cap};
    k_crop_keep<<<dim3(j.n_slots, (W + 3) / 4), 256, 0, s>>>(crop ? *crop : own, j.rec_pos, j.n_rec,
                                                              make_radius(j.crop_radius), keep);
    PVS_CHECK_LAUNCH();
    k_crop_slots<<<1, 256, 0, s>>>(j.lig_ptr, crop ? *crop : CropSets{}, keep, j.n_slots, j.lig_cap, j.n_rec, j.slot_cap,
                                   w.keep_rank, j.node_ptr, w.slot_of, j.status);
    PVS_CHECK_LAUNCH();
    return 0;
}

OutCsr out_csr(const PvsCsrOut& c) { return OutCsr{c.rowptr, c.row, c.col, c.etype, c.capacity}; }

template <class Slots, class... Start>
int build_slots(const PvsScreenSlotsJob& j, const ScreenState& w, hipStream_t s, Start... start) {
    Slots L;
    PVS_TRY(start_slots(j, w, s, &L, start...));
    const PvsCsrOut lig = kCropped<Slots> ? PvsCsrOut{} : j.lig;       // (cropped slots: no ligand-touching CSR)
    PVS_TRY(build_csrs(L, j.lig_pos, j.rec_pos, j.rr_rowptr, j.rr_col, j.inter_radius, j.intra_radius, j.full.rowptr,
                       lig.rowptr, out_csr(j.full), out_csr(lig), j.inv_deg, j.status, false, w, s));
    const int n_rows = j.lig_cap + j.n_slots * j.n_rec;
    k_node_tables_ragged<<<(n_rows + 3) / 4, 256, 0, s>>>(j.lig_pos, j.rec_pos, L, j.rr_rowptr, j.rr_col, j.node_graph,
                                                          j.pos, pvs_screen_job_tables(j));
    PVS_CHECK_LAUNCH();
    return 0;
}

}  // namespace

extern "C" size_t pvs_screen_slots_state_bytes(const PvsScreenSlotsJob* job) {
    char why[256];
    if (!job || pvs_screen_job_refusal(*job, true, why, sizeof(why))) return 0;
    PvsArena a(nullptr, 0);
    return carve_job(a, *job, nullptr) + 256;
}

extern "C" int pvs_screen_slots_build(const PvsScreenSlotsJob* job, void* state, size_t state_bytes,
                                      pvs_stream_t stream_) {
    const char* who = kPvsScreenJobWho;
    hipStream_t s = (hipStream_t)stream_;
    char why[256];
    PVS_REQUIRE(job && state, "%s: NULL %s", who, job ? "state" : "job");
    PVS_REQUIRE(!pvs_screen_job_refusal(*job, false, why, sizeof(why)), "%s", why);
    PvsArena arena(state, state_bytes);
    ScreenState w;
    carve_job(arena, *job, &w);
    PVS_REQUIRE(arena.ok(), "%s: state too small (%zu < %zu)", who, state_bytes, arena.off);
    PvsProfScope prof(s, PVS_PROF_PREPARE);
    switch (job->layout) {          // (one of the three: the refusal above)
        case PVS_SLOTS_STRUCK: return build_slots<PvsStruckSlots>(*job, w, s);
        case PVS_SLOTS_RAGGED: return build_slots<PvsRaggedSlots>(*job, w, s);
        default: return build_slots<PvsCroppedSlots>(*job, w, s);
    }
}

// ---- cropped copies (PvsScreenCopiesJob): cropped slots whose masks come from the job's crop table and rec_drop; the
// checks are screen_copies.h, the state and every launch behind the first two those of the embedded job ----
extern "C" size_t pvs_screen_copies_state_bytes(const PvsScreenCopiesJob* job) {
    char why[256];
    if (!job || pvs_screen_copies_refusal(*job, true, why, sizeof(why))) return 0;
    PvsArena a(nullptr, 0);
    return carve_job(a, job->slots, nullptr) + 256;
}

extern "C" int pvs_screen_copies_build(const PvsScreenCopiesJob* job, void* state, size_t state_bytes,
                                       pvs_stream_t stream_) {
    const char* who = kPvsScreenCopiesWho;
    hipStream_t s = (hipStream_t)stream_;
    char why[256];
    PVS_REQUIRE(job && state, "%s: NULL %s", who, job ? "state" : "job");
    PVS_REQUIRE(!pvs_screen_copies_refusal(*job, false, why, sizeof(why)), "%s", why);
    PvsArena arena(state, state_bytes);
    ScreenState w;
    carve_job(arena, job->slots, &w);
    PVS_REQUIRE(arena.ok(), "%s: state too small (%zu < %zu)", who, state_bytes, arena.off);
    PvsProfScope prof(s, PVS_PROF_PREPARE);
    const CropSets crop{job->crop_pos, job->crop_ptr, job->rec_drop, job->crop_cap, kPvsMaxSlotCap};
    return build_slots<PvsCroppedSlots>(job->slots, w, s, &crop);
}

extern "C" int pvs_crop_keep(const float* lig_pos, const int32_t* lig_ptr, int32_t n_hits, int32_t n_rows,
                             const float* rec_pos, int32_t n_rec, double crop_radius, uint64_t* keep,
                             int32_t* kept_ptr, pvs_stream_t stream_) {
    hipStream_t s = (hipStream_t)stream_;
    PVS_REQUIRE(n_hits >= 0 && n_rows >= 0 && n_rec >= 1, "pvs_crop_keep: %d hits, %d rows, %d receptor atoms", n_hits,
                n_rows, n_rec);
    PVS_REQUIRE(crop_radius > 0.0, "pvs_crop_keep: crop_radius must be positive (got %g)", crop_radius);
    PVS_REQUIRE(lig_ptr && rec_pos && kept_ptr && (n_rows == 0 || lig_pos) && (n_hits == 0 || keep),
                "pvs_crop_keep: NULL argument");
    const int W = pvs_rec_words(n_rec);
    PVS_REQUIRE((W + 3) / 4 <= 65535, "pvs_crop_keep: %d receptor atoms are more than one launch takes", n_rec);
    if (n_hits > 0) {
        const CropSets hits{lig_pos, lig_ptr, nullptr, n_rows, kPvsMaxSlotCap};
        k_crop_keep<<<dim3(n_hits, (W + 3) / 4), 256, 0, s>>>(hits, rec_pos, n_rec, make_radius(crop_radius),
                                                               (u64*)keep);
        PVS_CHECK_LAUNCH();
    }
    k_crop_keep_scan<<<1, 256, 0, s>>>(lig_ptr, n_hits, n_rows, W, (u64*)keep, kept_ptr);
    PVS_CHECK_LAUNCH();
    return 0;
}
