"""Cases and numpy references for the pose-batch builders, the leave-out packers and the hit listers at 65-513 slots
or hits (tests/test_gpu_many_slots.py; pinned on the host by tests/test_many_slots_cases_host.py). Pure numpy, importable
without a GPU; no GPU result is a yardstick here.

The case: ONE receptor of 70 atoms (two mask words, six bits in the second) and, for a count B, B slots whose ligands
have mostly 1-5 atoms. Slot p's atoms and features depend on p alone and its size on p and on whether p is the last slot
(the prefix property: the slots of a smaller count are those of a larger one, but for the last), so a slot's reference
edge list is computed once and shared by every count.

The references, as plain loops over the slots: the slot's complex through oracle.generate_edges_oracle.generate_edges
(rows gathered stably, as tests/test_gpu_library_screen.py does for a few slots), concatenated with node offsets into
what pvs_screen_slots_build writes for the ragged and the struck layout (`slot_batch`: the masking of
tests/_attribution_ref.masked_coo per struck slot) and for cropped slots and cropped copies (`cropped_batch`:
tests/_crop_ref.py, tests/_crop_copies_ref.py). Beside them the constructions the packer and lister tests share: the
copies of a hit table and a batch of them (`ligand_copies`, `pair_copies`, `packed_batch`), a brute-force fp64 contact
list (`contact_list`)."""
import numpy as np

from tests import _crop_copies_ref as cref
from tests import _crop_ref as ref
from tests._attribution_ref import masked_coo

N_REC, F = 70, 12
COUNTS = (65, 255, 256, 257, 513)
EMPTY_AT = (0, 63, 64, 255, 256)             # slots of 0 atoms, beside the last one
WIDE_AT = {1: 64, 65: 65, 257: 130}          # the sizes of a full ligand word, one past it, and two words and two bits
SLOT_CAP = 130
FAR_EVERY, FAR_AT = 41, 7                    # slot p with p % 41 == 7 is 100 A away: atoms, and no contact
RADII = (4.0, 6.0, 7.0)                      # the edge radii and the crop radius of the GPU tests
BAND = 1e-6
BOX = 10.0


# ---------------------------------------------------------------- the case

def receptor():
    """(rec_pos [70, 3], rec_feats [70, 12]) fp32: atoms drawn uniformly in a 10 A box, the last feature 1."""
    rng = np.random.default_rng(7001)
    pos = (rng.random((N_REC, 3)) * BOX).astype(np.float32)
    feats = rng.random((N_REC, F)).astype(np.float32)
    feats[:, -1] = 1
    return pos, feats


def slot_sizes(b):
    """The ligand sizes of a batch of b slots: 1-5 atoms, 0 at slots 0, 63, 64, 255, 256 and b - 1, and 64, 65 and 130
    atoms at slots 1, 65 and 257 (where they exist; the last slot is empty whatever else it would be)."""
    sizes = [1 + (7 * p + p // 3) % 5 for p in range(b)]
    for p, n in WIDE_AT.items():
        if p < b:
            sizes[p] = n
    for p in EMPTY_AT + (b - 1,):
        if p < b:
            sizes[p] = 0
    return sizes


def _slot_atoms(p):
    """(feats [130, 12], pos [130, 3]) of slot p, of which the slot holds the first `size` rows: small ligands are a
    3 A cloud around a centre inside the receptor's box, the wide ones spread over the box and 1 A beyond it."""
    rng = np.random.default_rng([7002, p])
    centre = 1.0 + rng.random(3) * (BOX - 2.0)
    cloud = centre + (rng.random((SLOT_CAP, 3)) - 0.5) * 3.0
    spread = rng.random((SLOT_CAP, 3)) * (BOX + 2.0) - 1.0
    pos = spread if p in WIDE_AT else cloud
    if p % FAR_EVERY == FAR_AT:
        pos = pos + np.array([100.0, 0.0, 0.0])
    feats = rng.random((SLOT_CAP, F)).astype(np.float32)
    feats[:, -1] = 0
    return feats, pos.astype(np.float32)


_SLOTS = {}


def slots(b):
    """[(feats [n, 12], pose [n, 3])] fp32 for the b slots."""
    out = []
    for p, n in enumerate(slot_sizes(b)):
        if p not in _SLOTS:
            _SLOTS[p] = _slot_atoms(p)
        feats, pos = _SLOTS[p]
        out.append((feats[:n], pos[:n]))
    return out


def distances(a, b):
    """[len(a), len(b)] fp64: the squares summed in index order and the root taken, as scipy's euclidean cdist."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 3), np.asarray(b, dtype=np.float64).reshape(-1, 3)
    d = a[:, None, :] - b[None, :, :]
    s = d[..., 0] * d[..., 0]
    s = s + d[..., 1] * d[..., 1]
    s = s + d[..., 2] * d[..., 2]
    return np.sqrt(s)


def contact_list(lig_pos, lig_ptr, rec_pos, radius):
    """(pairs [K, 2] int32, pair_ptr [S + 1] int32): every (ligand atom counted inside its hit, receptor atom) with
    1e-7 < d < radius in fp64, sorted by (hit, ligand atom, receptor atom) - brute force over all pairs."""
    lig_pos = np.asarray(lig_pos).reshape(-1, 3)
    pairs, ptr = [], [0]
    for s in range(len(lig_ptr) - 1):
        d = distances(lig_pos[int(lig_ptr[s]):int(lig_ptr[s + 1])], rec_pos)
        a, r = np.nonzero((d < float(radius)) & (d > 1e-7))          # (row-major: by a, then r)
        pairs.append(np.stack([a, r], 1))
        ptr.append(ptr[-1] + len(a))
    pairs = np.concatenate(pairs) if pairs else np.zeros((0, 2))
    return pairs.astype(np.int32).reshape(-1, 2), np.array(ptr, dtype=np.int32)


# ---------------------------------------------------------------- slot graphs

_EDGES = {}


def complex_edges(pos, is_rec, r_inter, r_intra=None):
    """(edge_index [2, E] int64, etype [E]) of one complex in CSR order: the oracle's generate_edges, rows gathered
    stably (the inter block before the intra block inside a row). A complex without atoms has no edges."""
    from oracle.generate_edges_oracle import generate_edges
    if len(pos) == 0:
        return np.zeros((2, 0), dtype=np.int64), np.zeros(0, dtype=np.int64)
    _, (rows, cols), attrs = generate_edges(np.asarray(pos), np.asarray(is_rec), r_inter,
                                            r_inter if r_intra is None else r_intra, prune=False)
    order = np.argsort(rows, kind='stable')
    return np.stack([rows[order], cols[order]]).astype(np.int64), np.asarray(attrs)[order].astype(np.int64)


def slot_edges(b, radius):
    """Per slot of the batch of b slots the edges of (its ligand, the whole receptor) at edge radius `radius`; cached by
    (slot, size, radius)."""
    rec, _ = receptor()
    out = []
    for p, (_, pose) in enumerate(slots(b)):
        key = (p, len(pose), float(radius))
        if key not in _EDGES:
            _EDGES[key] = complex_edges(np.concatenate([pose, rec]), np.concatenate([np.zeros(len(pose)), np.ones(N_REC)]),
                                        radius)
        out.append(_EDGES[key])
    return out


def _csr(want, rows, cols, ets, n_cap, lig_keep=None):
    """The CSR arrays of the concatenated slots into `want`: the full one and its inv_deg, and with lig_keep the
    ligand-touching one."""
    row = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    col = np.concatenate(cols) if cols else np.zeros(0, dtype=np.int64)
    et = np.concatenate(ets) if ets else np.zeros(0, dtype=np.int64)
    masks = [('', np.ones(len(row), dtype=bool))]
    if lig_keep is not None:
        masks.append(('_l', np.concatenate(lig_keep) if lig_keep else np.zeros(0, dtype=bool)))
    for tag, m in masks:
        d = np.bincount(row[m], minlength=n_cap)
        want['rowptr' + tag] = np.concatenate([[0], np.cumsum(d)]).astype(np.int32)
        want['row' + tag], want['col' + tag] = row[m].astype(np.int32), col[m].astype(np.int32)
        want['etype' + tag] = et[m].astype(np.uint8)
        if not tag:
            want['inv_deg'] = np.float32(1) / np.maximum(d, 1).astype(np.float32)
    return want


def slot_batch(edges, slots, rec_drop, rec, rec_feats, sums, n_cap):
    """What the ragged (rec_drop all -1) or the struck slot builder must write for a batch. edges: per slot (edge_index
    in slot-local ids, etype) of the UNSTRUCK slot in CSR order; slots: per slot (feats, pose) as numpy; sums: the
    screen's (rec_magg, rec_xsum, rec_deg), which the builder gathers. A struck slot is the reference's masking of the
    unstruck one (masked_coo: the atom and its edges go, the ids above it move down); a receptor row that had the atom as
    a template neighbour has a zero base and its whole row in the ligand-touching CSR. Padding rows: graph id -1, zeros,
    degree 0, inv_deg 1."""
    magg, xsum, deg = sums
    n_rec = rec.shape[0]
    rows, cols, ets, lig_keep = [], [], [], []
    node_ptr, node_graph = [0], np.full(n_cap, -1, dtype=np.int32)
    pos, x = np.zeros((n_cap, 3), np.float32), np.zeros((n_cap, rec_feats.shape[1]), np.float32)
    base = [np.zeros((n_cap, magg.shape[1]), np.float32), np.zeros((n_cap, 3), np.float32), np.zeros(n_cap, np.float32)]
    for p, ((ei, et), (feats, pose), r) in enumerate(zip(edges, slots, rec_drop)):
        n = len(pose)
        touched = np.zeros(n_rec, dtype=bool)
        if r >= 0:
            touched[ei[0][(ei[1] == n + r) & (et == 2)] - n] = True       # the rows that had r in their template row
            ei, et, _ = masked_coo(ei, et, [n + r])
        keep = np.array([i for i in range(n_rec) if i != r])
        n0 = node_ptr[-1]
        rows.append(ei[0] + n0)
        cols.append(ei[1] + n0)
        ets.append(et)
        row_touched = np.concatenate([np.zeros(n, dtype=bool), touched[keep]])
        lig_keep.append((ei[0] < n) | (ei[1] < n) | row_touched[ei[0]])
        size = n + len(keep)
        node_graph[n0:n0 + size] = p
        pos[n0:n0 + n], pos[n0 + n:n0 + size] = pose, rec[keep]
        x[n0:n0 + n], x[n0 + n:n0 + size] = feats, rec_feats[keep]
        based = keep[~touched[keep]]
        at = n0 + n + np.flatnonzero(~touched[keep])
        base[0][at], base[1][at], base[2][at] = magg[based], xsum[based], deg[based]
        node_ptr.append(n0 + size)
    want = dict(node_ptr=np.array(node_ptr, np.int32), node_graph=node_graph, pos=pos, x=x, base_magg=base[0],
                base_xsum=base[1], base_deg=base[2])
    return _csr(want, rows, cols, ets, n_cap, lig_keep)


_CROPPED = {}


def cropped_batch(slots, rec, rec_feats, crop, radius, n_cap, parents=None, rec_drop=None, cache=None):
    """What the cropped slot builder (parents None: every slot cropped around its own atoms) or the cropped copies
    builder (parents: per slot the atoms it is cropped AROUND; rec_drop: per slot -1 or the receptor atom it lacks) must
    write: keep [B, W] uint64, keep_rank [B, W + 1] int32, the node tables and the full CSR of the cropped complexes.
    cache: per slot a hashable name of the slot's inputs (or None), under which its complex and edges are kept."""
    b = len(slots)
    n_words = (rec.shape[0] + 63) // 64
    keep = np.zeros((b, n_words), dtype=np.uint64)
    rank = np.zeros((b, n_words + 1), dtype=np.int32)
    rows, cols, ets = [], [], []
    node_ptr, node_graph = [0], np.full(n_cap, -1, dtype=np.int32)
    pos, x = np.zeros((n_cap, 3), np.float32), np.zeros((n_cap, rec_feats.shape[1]), np.float32)
    for p, (feats, pose) in enumerate(slots):
        key = None if cache is None or cache[p] is None else (cache[p], float(crop), float(radius))
        if key is None or key not in _CROPPED:
            cx, cpos, kept = cref.copy_complex(feats, pose, rec_feats, rec, crop,
                                               rec_drop=-1 if rec_drop is None else int(rec_drop[p]),
                                               parent_pos=None if parents is None else parents[p])
            done = (cx, cpos.reshape(-1, 3), kept, complex_edges(cpos.reshape(-1, 3), cx[:, -1], radius))
            if key is not None:
                _CROPPED[key] = done
        cx, cpos, kept, (ei, et) = _CROPPED[key] if key is not None else done
        mask = np.zeros(rec.shape[0], dtype=bool)
        mask[kept] = True
        keep[p], rank[p] = ref.mask_words(mask), ref.rank_table(mask)
        n0, size = node_ptr[-1], len(cx)
        assert size == len(pose) + len(kept)
        rows.append(ei[0] + n0)
        cols.append(ei[1] + n0)
        ets.append(et)
        node_graph[n0:n0 + size] = p
        pos[n0:n0 + size], x[n0:n0 + size] = cpos, cx
        node_ptr.append(n0 + size)
    want = dict(keep=keep, keep_rank=rank, node_ptr=np.array(node_ptr, np.int32), node_graph=node_graph, pos=pos, x=x)
    return _csr(want, rows, cols, ets, n_cap)


# ---------------------------------------------------------------- hit tables, copies, packed batches

def ligands(sizes, n_feats=F):
    """(pos [L, 3], feats [L, n_feats], lig_ptr) of hits whose rows are distinct small integers as floats: every row of
    pos and feats names its source row."""
    total = int(sum(sizes))
    pos = np.arange(total * 3, dtype=np.float32).reshape(total, 3)
    feats = 1000.0 + np.arange(total * n_feats, dtype=np.float32).reshape(total, n_feats)
    return pos, feats, np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def pair_table(pairs):
    """(table [K, 2] int32, pair_ptr [S + 1] int32) of per-hit lists of (a, r)."""
    flat = [p for hit in pairs for p in hit]
    table = np.array(flat, dtype=np.int32).reshape(len(flat), 2)
    return table, np.concatenate([[0], np.cumsum([len(hit) for hit in pairs])]).astype(np.int32)


def ligand_copies(pos, feats, ptr):
    """Every leave-one-atom-out copy in order, (pos rows, feats rows, -1): the whole hit, then the hit without atom 0,
    without atom 1, ..."""
    out = []
    for s in range(len(ptr) - 1):
        rows = np.arange(ptr[s], ptr[s + 1])
        out.append((pos[rows], feats[rows], -1))
        for a in range(len(rows)):
            keep = np.delete(rows, a)
            out.append((pos[keep], feats[keep], -1))
    return out


def pair_copies(pos, feats, ptr, pairs):
    """Every leave-one-pair-out copy in order, (pos rows, feats rows, rec_drop): the whole hit, then one per pair (a, r)
    of the hit - without ligand atom a (-1: all of them), rec_drop r."""
    out = []
    for s, hit in enumerate(pairs):
        rows = np.arange(ptr[s], ptr[s + 1])
        out.append((pos[rows], feats[rows], -1))
        for a, r in hit:
            keep = np.delete(rows, a) if a >= 0 else rows
            out.append((pos[keep], feats[keep], int(r)))
    return out


def packed_batch(copies, first, n_slots, slot_cap, n_feats=F, sentinel=-7.0):
    """(pos, feats, out_ptr, rec_drop) of the batch whose slot k holds copy first + k (nothing for a number that is no
    copy): the rows packed from 0, sentinels behind out_ptr[n_slots]."""
    pos = np.full((n_slots * slot_cap, 3), sentinel, dtype=np.float32)
    feats = np.full((n_slots * slot_cap, n_feats), sentinel, dtype=np.float32)
    ptr, drop = np.zeros(n_slots + 1, dtype=np.int32), np.full(n_slots, -1, dtype=np.int32)
    for k in range(n_slots):
        at = ptr[k]
        if 0 <= first + k < len(copies):
            p, f, drop[k] = copies[first + k]
            pos[at:at + len(p)], feats[at:at + len(p)] = p, f
            at += len(p)
        ptr[k + 1] = at
    return pos, feats, ptr, drop


def hit_sizes(s):
    """The sizes of a table of s hits for the packers and listers: 1-4 atoms, none at hits 0, 255, 256 and s - 1 and
    every 50th, 9 atoms at hit 3."""
    sizes = [1 + (5 * h + h // 7) % 4 for h in range(s)]
    sizes[3 % s] = 9
    for h in (0, 255, 256, s - 1):
        if h < s:
            sizes[h] = 0
    for h in range(50, s, 50):
        sizes[h] = 0
    return sizes


def hit_pairs(sizes, n_rec):
    """Per hit a list of (a, r) pairs for the pair packer: 0-3 pairs per hit, none for a hit without atoms (and for
    every 9th), a of -1 and r of -1 among them, the receptor's last atom too."""
    out = []
    for h, n in enumerate(sizes):
        count = 0 if n == 0 or h % 9 == 4 else (h * 3 + 1) % 4
        hit = []
        for j in range(count):
            a = -1 if (h + j) % 5 == 0 else (h + 2 * j) % n
            r = -1 if (h + j) % 7 == 3 and a >= 0 else (n_rec - 1 if (h + j) % 11 == 0 else (13 * h + 5 * j) % n_rec)
            hit.append((a, r))
        out.append(hit)
    return out


def lister_hits(s, swap=False):
    """(lig_pos [L, 3] fp32, lig_ptr [S + 1] int32) for the listers: the atoms of slots(s + 1)[:s] (so a 64-atom hit
    at 1 and far hits among them) with hits 0, 255, 256 and s - 1 alternately empty (0 atoms) and far (atoms, no
    contact); swap: far where the other table has empty and the other way round."""
    poses = [pose for _, pose in slots(s + 1)[:s]]
    for k, h in enumerate(sorted({0, 255, 256, s - 1})):
        if h < s:
            poses[h] = poses[h][:0] if k % 2 == int(swap) else (_slot_atoms(2)[1][:3] + np.float32(200.0))
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in poses])]).astype(np.int32)
    return np.concatenate(poses).astype(np.float32).reshape(-1, 3), ptr
