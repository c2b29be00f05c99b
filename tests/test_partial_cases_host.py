"""Host-side pins of the partial-first-layer inputs and references (tests/_partial_cases.py): the rows the GPU tests
(tests/test_gpu_partial_layer.py) rely on are there, the two reference halves ARE the oracle layer, and the inputs tell
a wrong combination of base and partial sums from the right one by a wide margin - all from the oracle alone. No GPU."""
import numpy as np
import pytest
import torch

from tests import _edge_partition_cases as epc
from tests import _partial_cases as pc

FLAG_NAMES = tuple(pc.flag_sets())


def _csr(index, n):
    order = np.argsort(index[0], kind='stable')
    return np.searchsorted(index[0][order], np.arange(n + 1)), order


# (waves per block, block cap) of the forward launch sites the partial entries reach (tests/_edge_partition_cases.py SITES)
FWD_SITES = {name: epc.SITES[name][:2] for name in ('fwd_256', 'fwd_512', 'fwd_768', 'fwd_wide')}
# the environments of the GPU test's chunk cells -> (edges-per-wave floor, chunk size)
CHUNK_PLANS = {'PVS_CHUNK_EDGES=256': (64, 256), 'PVS_EDGES_PER_WAVE=4096 PVS_CHUNK_EDGES=256': (4096, 256)}


def _n_chunks(e, waves_per_block, cap, floor, chunk):
    """pvs_edge_grid (edge_dispatch.h; pinned against the C++ by tests/test_edge_dispatch.py)."""
    blocks = min(max(-(-e // (waves_per_block * floor)), 1), cap)
    waves = blocks * waves_per_block
    return waves * max(-(-e // (waves * chunk)), 1)


@pytest.mark.parametrize('ends', pc.ENDS)
@pytest.mark.parametrize('A', pc.CLASS_COUNTS)
def test_case_has_the_promised_rows(A, ends):
    c = pc.case(A, ends)
    n = c.n_nodes
    base, part = c.base_index.numpy(), c.part_index.numpy()
    nb, npart = base.shape[1], part.shape[1]
    assert n == 320 and 4000 <= nb + npart <= 6000 and c.pos.dtype == torch.float32 and c.pos.shape == (n, 3)
    for ei in (base, part):
        assert ei.min() >= 0 and ei.max() < n and not (ei[0] == ei[1]).any(), 'self loops make normalize=True ill-conditioned'
    assert (np.diff(part[0]) >= 0).all(), 'the partial list is CSR-sorted'
    assert (np.diff(base[0]) < 0).sum() > nb // 4, 'the base list is in arbitrary order'
    deg_b, deg_p = np.bincount(base[0], minlength=n), np.bincount(part[0], minlength=n)
    # the kinds on record are the kinds the edges give
    want = np.select([(deg_b == 0) & (deg_p == 0), deg_p == 0, deg_b == 0], [0, 1, 2], default=3)
    assert np.array_equal(c.kind, want) and pc.KINDS == ('none', 'base', 'partial', 'mixed')
    assert all(np.array_equal(c.rows[k], np.flatnonzero(want == i)) for i, k in enumerate(pc.KINDS))
    assert len(c.rows['none']) >= 8 and len(c.rows['base']) >= 40 and len(c.rows['partial']) >= 20
    assert (deg_b[pc.ONE_BASE], deg_p[pc.ONE_BASE]) == (1, 0) and (deg_b[pc.ONE_PARTIAL], deg_p[pc.ONE_PARTIAL]) == (0, 1)
    assert (deg_b[pc.ONE_ONE], deg_p[pc.ONE_ONE]) == (1, 1)
    assert (deg_b[pc.HUB], deg_p[pc.HUB]) == (pc.HUB_BASE, pc.HUB_PARTIAL) == (150, 200)
    # rows the partial launch never flushes, at both ends of the range and in the middle; rows it alone fills
    assert c.kind[0] == c.kind[n - 1] == pc.KINDS.index(ends)
    assert c.kind[n - 2] == c.kind[n - 3] == pc.KINDS.index('none')
    assert c.kind[5] == c.kind[6] == pc.KINDS.index('none'), 'two neighbouring rows without edges'
    # the split is the screens': the partial list = the ligand-touching edges of the union CSR, in its order
    bp = c.bp.numpy()
    assert np.array_equal(bp == 0, c.kind == pc.KINDS.index('partial'))
    ei, _ = pc.union(c)
    ei = ei.numpy()
    _, order = _csr(ei, n)
    keep = (bp[ei[0][order]] == 0) | (bp[ei[1][order]] == 0)
    assert np.array_equal(ei[:, order][:, keep], part)
    assert np.array_equal(order[keep] - nb, np.arange(npart))
    # the hub: several 32-edge tiles, and a nominal chunk cut inside it under every plan of the chunk cells
    rowptr, _ = _csr(part, n)
    lo, hi = int(rowptr[pc.HUB]), int(rowptr[pc.HUB + 1])
    assert hi - lo == 200 and (hi - 1) // 32 - lo // 32 >= 5
    for plan, (floor, chunk) in CHUNK_PLANS.items():
        for site, (nw, cap) in FWD_SITES.items():
            k = _n_chunks(npart, nw, cap, floor, chunk)
            cuts = np.arange(1, k, dtype=np.int64) * npart // k
            assert ((cuts > lo) & (cuts < hi)).any(), (plan, site, k, lo, hi)
            bounds = epc.chunk_bounds(rowptr, part[0], k)
            assert (bounds == lo).any() and not ((bounds > lo) & (bounds < hi)).any(), 'chunk ends are row-aligned'
    if A == 0:
        assert c.base_attr is None and c.part_attr is None and c.base_etype is None
        return
    for attr, et, index in ((c.base_attr, c.base_etype, base), (c.part_attr, c.part_etype, part)):
        assert attr.dtype == torch.int64 and tuple(attr.shape) == (index.shape[1], A)
        assert np.array_equal(attr.numpy().argmax(1), et.numpy()) and bool((attr.sum(1) == 1).all())
        assert (np.bincount(et.numpy(), minlength=A) > 0).all()
        assert set(et.numpy()[index[0] == pc.HUB]) == set(range(A)), 'the hub row holds every class in both sets'


def test_cases_share_their_rows_over_class_counts():
    a = pc.case(3, 'base')
    for A in pc.CLASS_COUNTS:
        b = pc.case(A, 'base')
        assert torch.equal(a.base_index, b.base_index) and torch.equal(a.part_index, b.part_index)
    other = pc.case(3, 'partial')
    assert other.kind[0] != a.kind[0] and int((other.kind != a.kind).sum()) == 2


def _sd64(p):
    return {k: v.double() for k, v in p.sd.items()}


# every flag set at A = 3, H = 32; three of them at the other class counts, widths and ends
THREE = ('plain', 'full-', 'gated-')
HALVES = [(f, 3, 32, 'base') for f in FLAG_NAMES] + [(f, A, hid, ends) for f in THREE for A, hid, ends in
                                                     ((3, 32, 'partial'), (0, 32, 'base'), (2, 32, 'base'), (5, 64, 'base'))]


@pytest.mark.parametrize('flags,A,hid,ends', HALVES)
def test_reference_halves_are_the_oracle_layer(flags, A, hid, ends):
    """finish(edge_sums(all edges)) is egnn_layer on the union graph (h', x', node attention), and the sums over the
    base set plus the sums over the partial set are the sums over the union: fp64, 1e-12."""
    from oracle import egnn_oracle as orc
    p = pc.problem(A, hid, flags, ends)
    c, f64 = p.case, torch.float64
    ei, ea = pc.union(c)
    h0, x0 = p.h0.double(), c.pos.double()
    with torch.no_grad():
        h, x, _, _, natt = orc.egnn_layer(_sd64(p), '', p.kw, h0, ei, x0, ea, None)
    whole = pc.edge_sums(p.sd, p.kw, p.h0, c.pos, ei, ea, f64)
    base = pc.edge_sums(p.sd, p.kw, p.h0, c.pos, c.base_index, c.base_attr, f64)
    part = pc.edge_sums(p.sd, p.kw, p.h0, c.pos, c.part_index, c.part_attr, f64)

    def same(a, b, what):
        scale = max(float(b.abs().max()), 1e-300)
        assert float((a - b).abs().max()) <= 1e-12 * scale, (what, float((a - b).abs().max()), scale)

    for a, b, w, what in zip(base, part, whole, ('magg', 'xsum', 'deg')):
        same(a + b, w, what)
    assert torch.equal(base[2] + part[2], whole[2])
    h2, x2, natt2 = pc.finish(p.sd, p.kw, p.h0, c.pos, *whole)
    same(h2, h, 'h_out')
    same(x2, x, 'x_out')
    assert (natt is None) == (natt2 is None) == (not p.kw['node_attention'])
    if natt is not None:
        same(natt2.reshape(-1), natt.reshape(-1), 'natt')
    if not p.kw['update_coords']:
        assert not whole[1].any() and torch.equal(x2, x0)
    # and the arbiter the GPU test holds is this one
    assert np.array_equal(p.ref64['h_out'], h.numpy()) and np.array_equal(p.ref64['base_magg'], base[0].numpy())
    assert np.array_equal(p.ref64['base_deg'], np.bincount(c.base_index[0].numpy(), minlength=c.n_nodes))


def _moved(p, key, got, kinds):
    """Smallest, over `kinds`, of (largest move of tensor `key` on the rows of the kind) / (the strict bound of those
    rows), and the same for the tensor as a whole."""
    ratios = []
    for k in kinds:
        rows = p.case.rows[k]
        ratios.append(float(np.abs(got[rows] - p.ref64[key][rows]).max()) / p.bound(key, rows))
    ratios.append(float(np.abs(got - p.ref64[key]).max()) / p.bound(key))
    return min(ratios)


@pytest.mark.parametrize('flags,hid', [(f, 32) for f in FLAG_NAMES] + [(f, 64) for f in THREE])
def test_wrong_combinations_of_the_sums_are_far_outside_the_bound(flags, hid):
    """Each defect moves the fp64 h' or x' on the rows of every kind it concerns by more than 100 x the strict bound the
    GPU test applies to those rows (and to the whole tensor):
      no base_magg      h' on base-only and mixed rows
      no base_xsum      x' on base-only and mixed rows
      partial degree    x' divided by the partial degree alone: base-only rows (clamped to 1) and mixed rows
      early clamp       max(base_deg, 1) + deg instead of max(base_deg + deg, 1): partial-only rows
    A layer whose node gate is shut hands h through (rezero0, gated0, gated-): there the node attention shows the first defect
    where the layer has one, and nothing can where it has none."""
    p = pc.problem(3, hid, flags)
    c, f64 = p.case, torch.float64
    mb, xb, db = pc.edge_sums(p.sd, p.kw, p.h0, c.pos, c.base_index, c.base_attr, f64)
    mp, xp, dp = pc.edge_sums(p.sd, p.kw, p.h0, c.pos, c.part_index, c.part_attr, f64)

    def run(magg, xsum, deg):
        h, x, natt = pc.finish(p.sd, p.kw, p.h0, c.pos, magg, xsum, deg)
        return h.numpy(), x.numpy(), (None if natt is None else natt.reshape(-1).numpy())

    right = run(mb + mp, xb + xp, db + dp)
    assert np.abs(right[0] - p.ref64['h_out']).max() <= 1e-12 * np.abs(p.ref64['h_out']).max()
    figures = {}
    no_magg = run(mp, xb + xp, db + dp)
    gate = p.flags.get('node_gate')      # (rezero: h + g out; gated: relu(g) out + (1 - relu(g)) h)
    gate_closed = gate is not None and (gate == 0.0 or (gate < 0 and not p.kw['rezero']))
    if not gate_closed:
        figures['no base_magg: h_out'] = _moved(p, 'h_out', no_magg[0], ('base', 'mixed'))
    elif p.kw['node_attention']:
        figures['no base_magg: natt'] = _moved(p, 'natt', no_magg[2], ('base', 'mixed'))
    else:
        assert np.array_equal(no_magg[0], right[0])
    if p.kw['update_coords']:
        figures['no base_xsum: x_out'] = _moved(p, 'x_out', run(mb + mp, xp, db + dp)[1], ('base', 'mixed'))
        figures['partial degree: x_out'] = _moved(p, 'x_out', run(mb + mp, xb + xp, dp)[1], ('base', 'mixed'))
        early = run(mb + mp, xb + xp, db.clamp(min=1) + dp)[1]
        figures['early clamp: x_out'] = _moved(p, 'x_out', early, ('partial',))
        for k in ('none', 'base', 'mixed'):        # (that defect is the partial-only rows' alone)
            assert np.array_equal(early[c.rows[k]], right[1][c.rows[k]])
    else:
        assert not xb.any() and not xp.any()
    print(flags, hid, {k: f'{v:.0f}x' for k, v in figures.items()})
    assert all(v > 100 for v in figures.values()), figures
