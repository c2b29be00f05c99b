"""The three radius-graph builders (pvs_radius_graph_count/_fill, pvs_screen_graph_build, pvs_screen_slots_build with PVS_SLOTS_RAGGED)
where random coordinates never take them (tests/_radius_cases.py): squared distances inside the +-2^-48 band around a
radius and around the 1e-7 lower bound (the square-root path of radius_common.h), and graph sizes at the edges of the
builders' tables (second trips of the 64-at-a-time loops, empty graphs, 1 / 63 / 64 / 65 nodes, no edge at all).
Integer work against the numpy oracle: every comparison is exact equality."""
import tempfile

import numpy as np
import pytest
import torch

from tests import _radius_cases as rc

pytestmark = pytest.mark.gpu

KW = dict(dim_input=12, k=32, dim_output=1, num_layers=2, residual=False, edge_residual=False,
          edge_attention=False, normalize=False, tanh=False, dropout=0.0, graphnorm=False, update_coords=True,
          permutation_invariance=False, node_attention=False, gated_residual=False, rezero=False,
          softmax_attention=False, model_task='classification')


def _csr(ref, n):
    """The CSR the builders make of a reference-order edge list: rows gathered stably (inside a row the inter block
    before the intra block, columns ascending in each), perm = the edge's position in the reference's order."""
    rows, cols, attrs = ref
    order = np.argsort(rows, kind='stable')
    deg = np.bincount(rows, minlength=n)
    return dict(rowptr=np.concatenate([[0], np.cumsum(deg)]).astype(np.int32), row=rows[order].astype(np.int32),
                col=cols[order].astype(np.int32), etype=attrs[order].astype(np.uint8), perm=order.astype(np.int32),
                inv_deg=(np.float32(1) / np.maximum(deg, 1).astype(np.float32)))


def _check_built(pos, bp, ptr, inter, intra, what='', only_modes=(False, True), backward_modes=(True, False)):
    """radius_graph(...) == the reference's edge list, array for array, full and ligand-touching, with and without
    the by-column lists. Returns the full graph's edge count."""
    from pointvs_amd.radius_graph import edges_in_reference_order, radius_graph
    n = len(pos)
    tpos, tbp = torch.from_numpy(pos).cuda(), torch.from_numpy(bp).cuda()
    tptr = None if ptr is None else torch.from_numpy(np.asarray(ptr))
    hptr = np.array([0, n]) if ptr is None else ptr
    n_edges = None
    for only in only_modes:
        ref = rc.batch_reference(pos, bp, hptr, inter, intra, ligand_pairs_only=only)
        want = _csr(ref, n)
        e = len(ref[0])
        for backward in backward_modes:
            tag = f'{what} ligand_pairs_only={only} need_backward={backward}'
            pg = radius_graph(tpos, tbp, tptr, inter, intra, need_backward=backward, ligand_pairs_only=only)
            assert pg.n_edges == e, tag
            ei, attrs = edges_in_reference_order(pg)
            assert np.array_equal(ei[0].cpu().numpy(), ref[0]) and np.array_equal(ei[1].cpu().numpy(), ref[1]), tag
            assert np.array_equal(attrs.cpu().numpy(), ref[2]), tag
            assert np.array_equal(pg.t['rowptr'].cpu().numpy(), want['rowptr']), tag
            for k in ('row', 'col', 'etype', 'perm'):
                assert np.array_equal(pg.t[k][:e].cpu().numpy(), want[k]), f'{tag} {k}'
            if not only:
                assert np.array_equal(pg.t['inv_deg'].cpu().numpy(), want['inv_deg']), tag
            assert int(pg.t['status'].item()) == 0, tag
            assert ('cedge' in pg.t) == backward and ('colptr' in pg.t) == backward
            if backward:
                by_col = np.argsort(want['col'], kind='stable')
                assert np.array_equal(pg.t['cedge'][:e].cpu().numpy(), by_col.astype(np.int32)), tag
                colptr = np.searchsorted(want['col'][by_col], np.arange(n + 1))
                assert np.array_equal(pg.t['colptr'].cpu().numpy(), colptr.astype(np.int32)), tag
        if not only:
            n_edges = e
    return n_edges


# ---- a. upper band, general builder ----
@pytest.mark.parametrize('probe', [p[0] for p in rc.UPPER_PROBES])
def test_radius_at_the_distance_of_a_pair_across_a_chunk_boundary(probe):
    """radius = the probe pair's distance moved by -8..8 ulps (the pair is an edge exactly for k > 0), the other
    radius below and above it; 130 atoms: three row blocks, two full mask words and a tail of 2."""
    pos, bp = rc.upper_band_graph()
    sweeps = [sw for sw in rc.upper_band_sweeps(pos, bp) if sw[0].startswith(probe + ' ')]
    assert len(sweeps) == 2 * len(rc.KS)
    counts = []
    for name, kind, s, inter, intra in sweeps:
        counts.append(_check_built(pos, bp, None, inter, intra, what=name))
    # the sweep does cross the decision: the pair's edges appear between k = 0 and k = 1 and nowhere else
    per_other = np.array(counts).reshape(2, len(rc.KS))
    step = np.diff(per_other, axis=1)
    k0 = rc.KS.index(0)
    assert (step[:, k0] > 0).all() and (np.delete(step, k0, axis=1) == 0).all(), per_other


# ---- b. the 1e-7 band ----
def test_lower_bound_band_on_a_batch_of_more_than_64_graphs():
    """73 graphs (70 two-atom ones, empty graphs first, in the middle and last: k_block_table's second trip and equal
    graph_ptr entries). Pairs with s in the band around 1e-14 (at s == 1e-14 the reference says no edge, s > r*r says
    edge), d = 0, a subnormal separation, the fp32 neighbours of 1e-7."""
    pos, bp, ptr, s = rc.zero_band_batch()
    assert len(ptr) - 1 == 73 and ptr[1] == 0 and ptr[-1] == ptr[-2]
    want_pairs = int((np.sqrt(s) > rc.ZERO).sum())
    assert 0 < want_pairs < len(s)
    e = _check_built(pos, bp, ptr, rc.ZERO_BATCH_RADIUS, rc.ZERO_BATCH_RADIUS, what='zero band')
    assert e == 4 * want_pairs          # both directions, inter block and intra block


# ---- c. table edges ----
def test_ragged_batch_with_empty_graphs_and_sizes_around_one_mask_word():
    pos, bp, ptr = rc.ragged_batch()
    assert tuple(np.diff(ptr)) == rc.RAGGED_SIZES
    assert _check_built(pos, bp, ptr, 3.0, 1.5, what='ragged') > 1000
    assert _check_built(pos, bp, ptr, 1.5, 3.0, what='ragged inter < intra') > 1000


def test_one_graph_of_4160_nodes_takes_the_second_trip_of_the_fill_loop():
    """65 mask words per row: lanes 0..63 expand the first 64, the second trip the last one (columns 4096..4159, three
    of them neighbours of node 0)."""
    pos, bp = rc.long_row_graph()
    near = np.flatnonzero(np.sqrt(rc.sqdist(pos[:1], pos))[0] < 1.0)
    assert {4100, 4130, 4159} <= set(near.tolist())
    e = _check_built(pos, bp, None, 3.0, 5.5, what='4160 nodes', backward_modes=(True,))
    assert 100_000 < e < 400_000, e


@pytest.mark.parametrize('need_backward', [True, False])
def test_a_batch_without_any_edge(need_backward):
    from pointvs_amd.radius_graph import edges_in_reference_order, radius_graph
    pos, bp, ptr = rc.no_edge_batch()
    for only in (False, True):
        pg = radius_graph(torch.from_numpy(pos).cuda(), torch.from_numpy(bp).cuda(), torch.from_numpy(ptr), 4.0, 2.0,
                          need_backward=need_backward, ligand_pairs_only=only)
        torch.cuda.synchronize()
        assert pg.n_edges == 0
        assert bool((pg.t['rowptr'] == 0).all()) and pg.t['rowptr'].numel() == 41
        assert bool((pg.t['inv_deg'] == 1).all()) and pg.t['inv_deg'].numel() == 40
        assert bool((pg.t['inter_ptr'] == 0).all()) and bool((pg.t['intra_ptr'] == 0).all())
        assert int(pg.t['status'].item()) == 0
        if need_backward:
            assert bool((pg.t['colptr'] == 0).all()) and pg.t['colptr'].numel() == 41
        ei, attrs = edges_in_reference_order(pg)
        assert ei.shape == (2, 0) and attrs.shape == (0,)
    _check_built(pos, bp, ptr, 4.0, 2.0, what='no edge')


# ---- d. pose builders ----
def _model():
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    torch.manual_seed(0)
    return SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **KW).eval()


def _feats(n_lig, n_rec, seed=3):
    """[n_lig + n_rec, 12] one-hot atom types, last column = bp (0 ligand, 1 receptor)."""
    rng = np.random.RandomState(seed)
    f = np.zeros((n_lig + n_rec, 12), dtype=np.float32)
    f[np.arange(n_lig + n_rec), rng.randint(0, 11, n_lig + n_rec)] = 1
    f[n_lig:, -1] = 1
    return torch.from_numpy(f)


def _assert_screen_csrs(f, n, n_alloc, pos, bp, ptr, inter, intra, what):
    """The builder's full and ligand-touching CSRs over the first n nodes == the reference per pose == radius_graph
    on the collated batch; rows from n on (padding) are empty."""
    from pointvs_amd.radius_graph import radius_graph
    tpos, tbp, tptr = torch.from_numpy(pos).cuda(), torch.from_numpy(bp).cuda(), torch.from_numpy(ptr)
    for tag, only in (('', False), ('_l', True)):
        ref = rc.batch_reference(pos, bp, ptr, inter, intra, ligand_pairs_only=only)
        want = _csr(ref, n)
        e = len(ref[0])
        rowptr = f['rowptr' + tag].cpu().numpy()
        assert rowptr.shape == (n_alloc + 1,) and np.array_equal(rowptr[:n + 1], want['rowptr']), what + tag
        assert (rowptr[n:] == e).all(), what + tag
        for k in ('row', 'col', 'etype'):
            assert np.array_equal(f[k + tag][:e].cpu().numpy(), want[k]), f'{what} {k}{tag}'
        if not only:
            assert np.array_equal(f['inv_deg'][:n].cpu().numpy(), want['inv_deg']), what
            assert bool((f['inv_deg'][n:] == 1).all()), what
        pg = radius_graph(tpos, tbp, tptr, inter, intra, need_backward=False, ligand_pairs_only=only)
        assert pg.n_edges == e and torch.equal(pg.t['rowptr'], f['rowptr' + tag][:n + 1]), what + tag
        for k in ('row', 'col', 'etype'):
            assert torch.equal(pg.t[k][:e], f[k + tag][:e]), f'{what} {k}{tag}'


POSE_SWEEPS = [(n_lig, n_rec, kind) for n_lig, n_rec in rc.POSE_SHAPES for kind in ('inter', 'intra')
               if n_lig > 2 or kind == 'inter']          # (one ligand atom: no ligand-ligand probe)


@pytest.mark.parametrize('n_lig,n_rec,kind', POSE_SWEEPS)
def test_pose_batch_builder_in_the_band(n_lig, n_rec, kind):
    """pvs_screen_graph_build for 1 and 64 ligand atoms against 64 / 65 / 130 receptor atoms (one full contact-mask
    word, one word and one bit, a partial third word), two poses; the probed radius at the probe pair's distance
    -8..8 ulps; two ligand atoms coincide (64-atom ligand)."""
    from pointvs_amd.screening import ReceptorScreen
    lig, rec = rc.pose_case(n_lig, n_rec)
    poses = np.stack([lig, lig + np.array([0.25, -0.5, 0.125], dtype=np.float32)])
    n = n_lig + n_rec
    pos = np.concatenate([np.concatenate([p, rec]) for p in poses]).astype(np.float32)
    feats = _feats(n_lig, n_rec)
    bp = np.tile(feats[:, -1].numpy().astype(np.int64), 2)
    ptr = np.array([0, n, 2 * n], dtype=np.int64)
    model = _model()
    sweeps = [sw for sw in rc.pose_sweeps(lig, rec) if sw[1] == kind]
    assert len(sweeps) == len(rc.KS)
    for name, _, s, inter, intra in sweeps:
        screen = ReceptorScreen(model, torch.from_numpy(rec).cuda(), feats, n_lig, 2, inter, intra)
        assert screen.fast_graph
        screen._build_fast(torch.from_numpy(poses).cuda())
        screen.check()
        torch.cuda.synchronize()
        _assert_screen_csrs(screen._fast, 2 * n, 2 * n, pos, bp, ptr, inter, intra, f'{n_lig}x{n_rec} {name}')


@pytest.mark.parametrize('n_rec,kind', [(n_rec, kind) for n_rec in (64, 65, 130) for kind in ('inter', 'intra')])
def test_ragged_pose_builder_in_the_band(n_rec, kind):
    """pvs_screen_slots_build (PVS_SLOTS_RAGGED) with slots of 64, 0, 1 and 64 ligand atoms: the same probes in slot 0."""
    from pointvs_amd.screening import LibraryScreen
    lig, rec = rc.pose_case(64, n_rec)
    feats = _feats(64, n_rec)
    lig_feats, rec_feats = feats[:64].contiguous(), feats[64:].contiguous()
    shifted = lig + np.array([0.25, -0.5, 0.125], dtype=np.float32)
    slot_pos = {0: lig, 2: shifted[5:6], 3: shifted}
    assert tuple(len(slot_pos.get(k, ())) for k in range(4)) == rc.RAGGED_SLOT_SIZES
    slots, parts, bps = [], [], []
    for k, size in enumerate(rc.RAGGED_SLOT_SIZES):
        p = slot_pos.get(k, lig[:0])
        slots.append((lig_feats[:size].contiguous(), torch.from_numpy(np.ascontiguousarray(p))))
        parts += [p, rec]
        bps += [np.zeros(size, dtype=np.int64), np.ones(n_rec, dtype=np.int64)]
    pos, bp = np.concatenate(parts).astype(np.float32), np.concatenate(bps)
    lig_ptr = np.concatenate([[0], np.cumsum(rc.RAGGED_SLOT_SIZES)])
    ptr = (lig_ptr + np.arange(5) * n_rec).astype(np.int64)
    n = int(ptr[-1])
    model = _model()
    sweeps = [sw for sw in rc.pose_sweeps(lig, rec) if sw[1] == kind]
    assert len(sweeps) == len(rc.KS)
    for name, _, s, inter, intra in sweeps:
        screen = LibraryScreen(model, torch.from_numpy(rec).cuda(), rec_feats, 4, 64, inter, intra).load(slots)
        f = screen._build()
        screen.check()
        torch.cuda.synchronize()
        assert f['node_ptr'].cpu().tolist() == ptr.tolist()
        _assert_screen_csrs(f, n, screen.n_cap, pos, bp, ptr, inter, intra, f'ragged x{n_rec} {name}')


# ---- e. prune ----
def test_prune_keeps_the_component_of_a_long_chain():
    """Min-label propagation over a 300-atom chain (many sweeps, several host round trips of four sweeps each): the
    kept atoms, edges and classes of generate_edges(prune=True) == the oracle's; the 20-atom chain far away goes."""
    from oracle.generate_edges_oracle import generate_edges as oracle_edges
    from pointvs_amd.radius_graph import generate_edges
    pos, bp = rc.chain_structure()
    keep_ref, (rows, cols), attrs_ref = oracle_edges(pos, bp, 4.0, 2.0, prune=True)
    assert len(keep_ref) == 301 and len(pos) == 321
    keep, ei, attrs = generate_edges(torch.from_numpy(pos).cuda(), torch.from_numpy(bp).cuda(), 4.0, 2.0, prune=True)
    assert np.array_equal(keep.cpu().numpy(), keep_ref)
    assert np.array_equal(ei[0].cpu().numpy(), rows) and np.array_equal(ei[1].cpu().numpy(), cols)
    assert np.array_equal(attrs.cpu().numpy(), attrs_ref)
