"""Hand-made inputs for the radius-graph builders (pvs_radius_graph_*, pvs_screen_graph_build[_ragged]) at the
places where random coordinates never go: squared distances inside the +-2^-48 band around a radius (where
radius_common.h leaves the `s` vs `r*r` shortcut and takes the correctly rounded square root), around the 1e-7 lower
bound, and graph sizes at the edges of the builders' tables. Pure numpy, deterministic, no GPU: the host test
(tests/test_radius_cases_host.py) proves that the cases discriminate, the GPU test (tests/test_gpu_radius_decisions.py)
runs them.

The arbiter is oracle.generate_edges_oracle (pinned by tests/golden/edges_*.npz); `reference_edges` restates its
prune=False result without n^2 temporaries."""
import numpy as np

ZERO = 1e-7                 # the reference's lower bound on a distance (preprocessing.py:110)
BAND = 2.0 ** -48           # relative half width of the band in which radius_common.h evaluates the square root
KS = tuple(range(-8, 9))    # radius = ulps(d, k) of a probe pair's distance d


def sqdist(a, b):
    """s[i, j] = sum_k (a[i, k] - b[j, k])^2 in fp64, accumulated in index order from 0 exactly as
    oracle.generate_edges_oracle.cdist_euclidean (scipy's euclidean_distance_double) does; sqrt(s) is the distance."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    s = np.zeros((len(a), len(b)), dtype=np.float64)
    for k in range(a.shape[1]):
        d = a[:, None, k] - b[None, :, k]
        s += d * d
    return s


def ulps(x, k):
    """x moved by k double ulps (k < 0: towards zero for positive x)."""
    x = np.float64(x)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, np.float64(np.inf if k > 0 else -np.inf))
    return float(x)


def reference_edges(pos, bp, inter, intra, block=256):
    """(rows, cols, attrs) of the oracle's generate_edges(pos, bp, inter, intra, prune=False) for ONE graph, in its
    order (inter block row-major, then intra block row-major), from row blocks of `block` x n distances."""
    pos = np.asarray(pos, dtype=np.float64)
    bp = np.asarray(bp).astype(np.int64)
    parts = {'ri': [], 'ci': [], 'ra': [], 'ca': []}
    for r0 in range(0, len(pos), block):
        d = np.sqrt(sqdist(pos[r0:r0 + block], pos))
        near = d > ZERO
        r, c = np.where((d < inter) & near)
        keep = bp[r + r0] != bp[c]
        parts['ri'].append(r[keep] + r0)
        parts['ci'].append(c[keep])
        r, c = np.where((d < intra) & near)
        parts['ra'].append(r + r0)
        parts['ca'].append(c)
    ri, ci, ra, ca = (np.concatenate(parts[k]) if parts[k] else np.zeros(0, dtype=np.int64)
                      for k in ('ri', 'ci', 'ra', 'ca'))
    attrs = np.concatenate([np.ones(len(ri), dtype=np.int32),
                            np.where((bp[ra] == 1) & (bp[ca] == 1), 2, 0).astype(np.int32)])
    return np.concatenate([ri, ra]).astype(np.int64), np.concatenate([ci, ca]).astype(np.int64), attrs


def batch_reference(pos, bp, ptr, inter, intra, ligand_pairs_only=False):
    """The edge list radius_graph() stands for on a batch: every graph's inter block (global node ids, graphs in
    order), then every graph's intra block. ligand_pairs_only: the pairs that touch a ligand atom (bp == 0)."""
    pos, bp = np.asarray(pos), np.asarray(bp).astype(np.int64)
    inter_part, intra_part = [], []
    for g in range(len(ptr) - 1):
        n0, n1 = int(ptr[g]), int(ptr[g + 1])
        rows, cols, attrs = reference_edges(pos[n0:n1], bp[n0:n1], inter, intra)
        if ligand_pairs_only:
            keep = (bp[n0:n1][rows] == 0) | (bp[n0:n1][cols] == 0)
            rows, cols, attrs = rows[keep], cols[keep], attrs[keep]
        n_inter = int((attrs == 1).sum())          # class 1 = the inter block; intra edges are class 0 or 2
        assert (attrs[:n_inter] == 1).all()
        inter_part.append((rows[:n_inter] + n0, cols[:n_inter] + n0, attrs[:n_inter]))
        intra_part.append((rows[n_inter:] + n0, cols[n_inter:] + n0, attrs[n_inter:]))
    parts = inter_part + intra_part
    return tuple(np.concatenate([p[k] for p in parts]) for k in range(3))


# ---- the 1e-7 band ----
def zero_band_pairs(keep_differing=3, keep_each_side=10):
    """fp32 triples (a, b, c) whose squared distance from the origin, as cdist accumulates it, lies inside
    [1e-14 (1 - 2^-48), 1e-14 (1 + 2^-48)], each with the oracle's decision sqrt(s) > 1e-7.

    Search over a fixed grid (no random draw): a = fp32(7.0e-8) + 0..399 ulps, b = fp32(sqrt(1e-14 - a^2)) - 0..799
    ulps, c = fp32(sqrt(1e-14 - a^2 - b^2)) - 3..+3 ulps: 1817 triples in the band, on 47 different doubles s.

    "Differs" is measured against the shortcut a kernel would take, s > r*r with r = 1e-7: fl(1e-7 * 1e-7) is the
    double BELOW 1e-14, sqrt(1e-14) rounds to exactly 1e-7, so at s == 1e-14 the shortcut says "edge" and the
    reference says "no edge". That is the only double where they differ (48 of the 1817 triples land on it). The
    literal `s > 1e-14` is NOT a wrong rule: it agrees with sqrt(s) > 1e-7 at every double (test_radius_cases_host).

    Kept: the first `keep_differing` triples (grid order) with s == 1e-14 - they all pin the same double - and on each
    side of the decision one triple for each of `keep_each_side` different doubles: the half nearest to 1e-14 and the
    half nearest to the band's edge.
    Returns (triples [K, 3] float32, decision [K] bool, s [K] float64, n_in_band, n_differing_in_band)."""
    a = np.float32(7.0e-8)
    a = (a + np.arange(400, dtype=np.float64) * np.spacing(a)).astype(np.float32)
    assert (np.diff(a) > 0).all()
    a64 = a.astype(np.float64)[:, None]
    b0 = np.sqrt(1e-14 - a64 * a64).astype(np.float32)
    b = (b0.astype(np.float64) - np.arange(800, dtype=np.float64)[None, :] * np.spacing(b0)).astype(np.float32)
    b64 = b.astype(np.float64)
    ab = a64 * a64 + b64 * b64                                          # [400, 800]
    c0 = np.sqrt(np.maximum(1e-14 - ab, 0.0)).astype(np.float32)
    found = []
    for k in range(-3, 4):
        c = (c0.astype(np.float64) + k * np.spacing(c0)).astype(np.float32)
        c64 = c.astype(np.float64)
        s = ab + c64 * c64
        hit = (s >= 1e-14 * (1.0 - BAND)) & (s <= 1e-14 * (1.0 + BAND)) & (c > 0)
        for ii, jj in zip(*np.where(hit)):
            found.append((int(ii), int(jj), k, a[ii], b[ii, jj], c[ii, jj], s[ii, jj]))
    found.sort(key=lambda t: t[:3])
    triples = np.array([t[3:6] for t in found], dtype=np.float32).reshape(-1, 3)
    s = np.array([t[6] for t in found], dtype=np.float64)
    decision = np.sqrt(s) > ZERO
    differs = decision != (s > ZERO * ZERO)
    keep = np.zeros(len(s), dtype=bool)
    keep[np.flatnonzero(differs)[:keep_differing]] = True
    for side in (True, False):
        same = np.flatnonzero((decision == side) & ~differs)
        values, first = np.unique(s[same], return_index=True)          # one triple (the first on the grid) per double
        by_gap = same[first[np.argsort(np.abs(values - 1e-14), kind='stable')]]
        half = keep_each_side // 2
        keep[by_gap[:half]] = True
        keep[by_gap[len(by_gap) - (keep_each_side - half):]] = True
    return triples[keep], decision[keep], s[keep], len(found), int(differs.sum())


# ---- wrong decision rules a builder could take instead of radius_common.h's (host test only) ----
def oracle_rule(s, r):
    """1e-7 < d < r as the reference decides it."""
    d = np.sqrt(s)
    return (d < r) & (d > ZERO)


naive_rules = {
    's < r*r': lambda s, r: (s < r * r) & (np.sqrt(s) > ZERO),
    's <= r*r': lambda s, r: (s <= r * r) & (np.sqrt(s) > ZERO),
    'sqrt in fp32': lambda s, r: (np.sqrt(np.asarray(s, dtype=np.float32)) < np.float32(r)) & (np.sqrt(s) > ZERO),
    # the lower bound by squares, as a kernel that is handed the bound 1e-7 computes it (see zero_band_pairs)
    's > 1e-7*1e-7': lambda s, r: (np.sqrt(s) < r) & (s > ZERO * ZERO),
}


# ---- the upper band: one 130-atom graph, three probe pairs across 64-column chunk boundaries ----
N_UPPER = 130
UPPER_PROBES = (('inter', 63, 64), ('intra_rr', 62, 65), ('intra_ll', 1, 129))     # every pair: i // 64 != j // 64


def upper_band_graph(seed=10):
    """pos [130, 3] fp32 in a 6 A box, bp [130]: two full 64-column chunks and a tail of 2, three row blocks. Ligand
    atoms: 0..3, 63, 128, 129, so that the probes 63-64 (ligand-receptor), 62-65 (receptor-receptor) and 1-129
    (ligand-ligand) each have their two atoms in different 64-column chunks and different row blocks. The seed is one
    at which the probes' d = sqrt(s) squares to more than s (63-64, 62-65) and to less (1-129): `s < d*d` and
    `s <= d*d` then decide radius = d wrongly (tests/test_radius_cases_host.py holds the sweeps to that)."""
    rng = np.random.RandomState(seed)
    pos = (rng.rand(N_UPPER, 3) * 6.0).astype(np.float32)
    bp = np.ones(N_UPPER, dtype=np.int64)
    bp[[0, 1, 2, 3, 63, 128, 129]] = 0
    return pos, bp


def upper_band_sweeps(pos, bp):
    """[(name, kind, s, inter_radius, intra_radius)]: for each probe pair (squared distance s, d = sqrt(s)) the probed
    radius (`kind`: 'inter' or 'intra') at ulps(d, k), k = -8..8, with the other radius once below and once above it,
    so that `far` in k_radius_masks is once the probed radius and once the other one (inter < intra, inter > intra)."""
    out = []
    for name, i, j in UPPER_PROBES:
        s = float(sqdist(pos[i:i + 1], pos[j:j + 1])[0, 0])
        d = float(np.sqrt(s))
        kind = 'inter' if name == 'inter' else 'intra'
        for other in (0.6 * d, 1.5 * d):
            for k in KS:
                r = ulps(d, k)
                out.append((f'{name} k={k} other={other / d:.1f}d', kind, s) +
                           ((r, other) if kind == 'inter' else (other, r)))
    return out


# ---- the 1e-7 band as a batch of two-atom graphs ----
ZERO_BATCH_RADIUS = 4.0      # inter = intra radius of that batch: every pair with d > 1e-7 is an edge of both blocks


def zero_band_batch(n_graphs=70):
    """(pos [N, 3] fp32, bp [N], ptr [B + 1], s [n_pairs]): `n_graphs` two-atom graphs (a ligand atom at the origin, a
    receptor atom beside it) with an empty graph first, in the middle and last. The pairs: zero_band_pairs(), an exact
    duplicate, a subnormal-scale separation, then the fp32 neighbours of 1e-7 along x (below and above, alternating)."""
    triples = zero_band_pairs()[0]
    second = [t for t in triples]
    second.append(np.zeros(3, dtype=np.float32))                                  # exact duplicate: d = 0
    second.append(np.array([1e-40, 0, 0], dtype=np.float32))                      # subnormal fp32, s = 1e-80
    assert len(second) < n_graphs
    x = np.float32(ZERO)
    step = 0
    while len(second) < n_graphs:
        k = ((step + 1) // 2) * (-1 if step % 2 else 1)            # 0, -1, 1, -2, 2, ...
        second.append(np.array([np.float64(x) + k * np.spacing(x), 0, 0], dtype=np.float32))
        step += 1
    sizes = []
    pos = []
    for g, p in enumerate(second):
        if g in (0, n_graphs // 2):
            sizes.append(0)
        sizes.append(2)
        pos += [np.zeros(3, dtype=np.float32), p]
    sizes.append(0)
    pos = np.array(pos, dtype=np.float32)
    bp = np.tile(np.array([0, 1], dtype=np.int64), n_graphs)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    s = np.array([sqdist(pos[2 * g:2 * g + 1], pos[2 * g + 1:2 * g + 2])[0, 0] for g in range(n_graphs)])
    return pos, bp, ptr, s


# ---- table edges ----
RAGGED_SIZES = (1, 0, 2, 63, 64, 65, 128, 129, 0)


def ragged_batch(seed=11):
    """Graphs of RAGGED_SIZES atoms (empty ones inside and last: equal graph_ptr entries), each in a 5 A box, every
    fourth atom a ligand atom."""
    rng = np.random.RandomState(seed)
    n = sum(RAGGED_SIZES)
    pos = (rng.rand(n, 3) * 5.0).astype(np.float32)
    bp = (np.arange(n) % 4 != 0).astype(np.int64)
    ptr = np.concatenate([[0], np.cumsum(RAGGED_SIZES)]).astype(np.int64)
    return pos, bp, ptr


N_LONG_ROW = 4160            # 65 mask words per row: the 64-words-at-a-time loops make their second trip


def long_row_graph(seed=13):
    """One graph of 4160 atoms in a 40 A box (about 45 neighbours within an intra radius of 5.5 A: E in the low hundred thousands); the
    first 8 atoms are the ligand; atoms 4100, 4130 and 4159 (65th mask word) sit within 1 A of atom 0."""
    rng = np.random.RandomState(seed)
    pos = (rng.rand(N_LONG_ROW, 3) * 40.0).astype(np.float32)
    for k, j in enumerate((4100, 4130, 4159)):
        pos[j] = pos[0] + np.array([0.3 * (k + 1), 0.2, -0.1 * k], dtype=np.float32)
    bp = np.ones(N_LONG_ROW, dtype=np.int64)
    bp[:8] = 0
    return pos, bp


def no_edge_batch():
    """40 atoms 50 A apart on a line, in 3 graphs (13, 14, 13): no edge at any sensible radius."""
    pos = np.zeros((40, 3), dtype=np.float32)
    pos[:, 0] = np.arange(40) * 50.0
    bp = (np.arange(40) % 2).astype(np.int64)
    return pos, bp, np.array([0, 13, 27, 40], dtype=np.int64)


# ---- pose builders ----
def pose_case(n_lig, n_rec, seed=17):
    """(lig [n_lig, 3], rec [n_rec, 3]) fp32 in a 6 A box. The last receptor atom (last bit of the last contact-mask
    word) sits 2.3 A from the first ligand atom: the ligand-receptor probe. With 64 ligand atoms the last one
    coincides exactly with the first (d = 0: no edge between them, the same contacts for both) and atom 62 sits
    1.5 A from atom 1: the ligand-ligand probe."""
    rng = np.random.RandomState(seed + 1000 * n_lig + n_rec)
    lig = (rng.rand(n_lig, 3) * 6.0).astype(np.float32)
    rec = (rng.rand(n_rec, 3) * 6.0).astype(np.float32)
    rec[-1] = lig[0] + np.array([1.7, 1.3, 0.9], dtype=np.float32)
    if n_lig > 2:
        lig[-1] = lig[0]
        lig[-2] = lig[1] + np.array([1.1, -0.8, 0.6], dtype=np.float32)
    return lig, rec


def pose_sweeps(lig, rec):
    """[(name, kind, s, inter_radius, intra_radius)] like upper_band_sweeps: the ligand-receptor probe (first ligand
    atom - last receptor atom: the last bit of the last mask word) with inter_radius = ulps(d, k) and, with three or
    more ligand atoms, the ligand-ligand probe (atoms 1 and n_lig - 2) with intra_radius = ulps(d, k)."""
    out = []
    s = float(sqdist(lig[:1], rec[-1:])[0, 0])
    d = float(np.sqrt(s))
    out += [(f'inter k={k}', 'inter', s, ulps(d, k), 0.5 * d) for k in KS]
    if len(lig) > 2:
        i, j = 1, len(lig) - 2
        s = float(sqdist(lig[i:i + 1], lig[j:j + 1])[0, 0])
        d = float(np.sqrt(s))
        out += [(f'intra k={k}', 'intra', s, 1.25 * d, ulps(d, k)) for k in KS]
    return out


POSE_SHAPES = tuple((n_lig, n_rec) for n_lig in (1, 64) for n_rec in (64, 65, 130))
RAGGED_SLOT_SIZES = (64, 0, 1, 64)


# ---- prune ----
def chain_structure():
    """A 300-atom receptor chain along x (1.5 A spacing: bonded at intra 2.0), one ligand atom 3 A beside its middle
    (inter 4.0 reaches a few chain atoms) and a second, disconnected 20-atom receptor chain 100 A away, placed in the
    MIDDLE of the node order (the kept set is not a prefix). The component's lowest label has to travel the whole
    chain: many min-label sweeps, several host round trips."""
    chain = np.zeros((300, 3), dtype=np.float32)
    chain[:, 0] = np.arange(300) * 1.5
    lig = np.array([[150 * 1.5, 3.0, 0.0]], dtype=np.float32)
    far = np.zeros((20, 3), dtype=np.float32)
    far[:, 0] = np.arange(20) * 1.5
    far[:, 1] = 100.0
    pos = np.concatenate([chain[:100], far, lig, chain[100:]], 0)
    bp = np.ones(len(pos), dtype=np.int64)
    bp[120] = 0
    return pos, bp
