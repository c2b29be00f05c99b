"""Library screening (pointvs_amd/screening.py: LibraryScreen, ScreeningSweep.run_library): pose batches that mix
ligands of different sizes, built by pvs_screen_slots_build (PVS_SLOTS_RAGGED). Receptor of 130 atoms everywhere: three 64-bit
contact-mask words, the last one partial."""
import math
import tempfile

import numpy as np
import pytest
import torch

from tests._golden import needs_caching_allocator

pytestmark = pytest.mark.gpu

N_REC = 130
SIZES = (1, 64, 0, 7, 33, 20)
KW = dict(dim_input=12, k=32, dim_output=1, num_layers=2, residual=False, edge_residual=False,
          edge_attention=False, normalize=False, tanh=False, dropout=0.0, graphnorm=False, update_coords=True,
          permutation_invariance=False, node_attention=False, gated_residual=False, rezero=False,
          softmax_attention=False, model_task='classification')


def _model(seed=0, **flags):
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    torch.manual_seed(seed)
    return SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **dict(KW, **flags)).eval()


def _set(seed, n_lig=64):
    """(ligand [n_lig,3], receptor [130,3], ligand feats, receptor feats): the 130 receptor atoms of a
    screening_set nearest its centre."""
    from pointvs_amd.synthetic import screening_set
    lig, rec, feats = screening_set(seed=seed, n_nodes=n_lig + 400, n_lig=n_lig)
    near = torch.argsort((rec - lig.mean(0)).norm(dim=1))[:N_REC].sort().values
    return lig, rec[near].contiguous(), feats[:n_lig].contiguous(), feats[n_lig:][near].contiguous()


def _slots(lig, lig_feats, sizes, seed, rec=None, special=True):
    """One pose per slot: slot k holds the first sizes[k] ligand atoms (features rolled by k) in a random pose.
    special: the first atom of the 7-atom ligand sits exactly on receptor atom 5 (d = 0: excluded), the 33-atom
    ligand is 100 A away (no contacts, isolated ligand rows)."""
    from pointvs_amd.synthetic import random_poses
    slots = []
    for k, n in enumerate(sizes):
        if n == 0:
            slots.append((lig_feats[:0], lig[:0]))
            continue
        pose = random_poses(lig[:n], 1, seed=seed + k, max_shift=3.0)[0].contiguous()
        if special and n == 7:
            pose[0] = rec[5]
        if special and n == 33:
            pose = pose + torch.tensor([100.0, 0.0, 0.0])
        slots.append((lig_feats[:n].roll(k, 0).contiguous(), pose))
    return slots


def _oracle_items(slots, rec, rec_feats, r_inter, r_intra):
    """The batch's complexes as Data items with the oracle's edge lists (reference order)."""
    from oracle.generate_edges_oracle import generate_edges as oracle_edges
    from pointvs_amd.graph import Data
    items = []
    for feats, pose in slots:
        pos, x = torch.cat([pose, rec], 0), torch.cat([feats, rec_feats], 0)
        _, (rows, cols), attrs = oracle_edges(pos.numpy(), x[:, -1].numpy(), r_inter, r_intra, prune=False)
        items.append(Data(x=x, pos=pos, edge_index=torch.from_numpy(np.vstack([rows, cols])).long(),
                          edge_attr=torch.nn.functional.one_hot(torch.from_numpy(attrs).long(), 3),
                          y=torch.tensor(0), lig_fname='l', rec_fname='r'))
    return items


@pytest.mark.parametrize('radii', [(7.0, None), (6.0, 2.5)])
def test_ragged_builder_equals_the_reference_edge_lists(radii):
    """Per slot the full CSR == the oracle's generate_edges shifted by node_ptr[p]; the whole batch == the general
    builder on the compact mixed batch (full and ligand-touching); padding rows are empty; node tables == gathers."""
    from pointvs_amd.radius_graph import radius_graph
    from pointvs_amd.screening import LibraryScreen
    r_inter, r_intra = radii
    lig, rec, lig_feats, rec_feats = _set(6001)
    slots = _slots(lig, lig_feats, SIZES, seed=10, rec=rec)
    screen = LibraryScreen(_model(), rec.cuda(), rec_feats, len(SIZES), 64, r_inter, r_intra).load(slots)
    f = screen._build()
    screen.check()
    torch.cuda.synchronize()
    n_cap, n = screen.n_cap, sum(SIZES) + len(SIZES) * N_REC
    assert n_cap == len(SIZES) * (64 + N_REC)
    lig_ptr = np.concatenate([[0], np.cumsum(SIZES)])
    node_ptr = lig_ptr + np.arange(len(SIZES) + 1) * N_REC
    assert f['node_ptr'].cpu().tolist() == node_ptr.tolist()
    rowptr, e = f['rowptr'].cpu().numpy(), int(f['rowptr'][n_cap])
    row, col, etype = (f[k][:e].cpu().numpy() for k in ('row', 'col', 'etype'))
    # per slot: the oracle's list, rows gathered stably (inter block before intra block inside a row)
    items = _oracle_items(slots, rec, rec_feats, r_inter, r_inter if r_intra is None else r_intra)
    for p, item in enumerate(items):
        rows, cols = item.edge_index.numpy()
        attrs = item.edge_attr.argmax(1).numpy()
        order = np.argsort(rows, kind='stable')
        lo, hi = rowptr[node_ptr[p]], rowptr[node_ptr[p + 1]]
        assert hi - lo == len(rows), p
        assert np.array_equal(row[lo:hi], rows[order] + node_ptr[p]), p
        assert np.array_equal(col[lo:hi], cols[order] + node_ptr[p]), p
        assert np.array_equal(etype[lo:hi], attrs[order]), p
    isolated = np.arange(node_ptr[4], node_ptr[4] + 33)          # the far ligand: intra-ligand edges only
    assert (col[rowptr[isolated[0]]:rowptr[isolated[-1] + 1]] < node_ptr[4] + 33).all()
    # the whole batch: the general builder on the compact mixed batch
    pos = torch.cat([t for _, pose in slots for t in (pose, rec)], 0).cuda()
    x = torch.cat([t for feats, _ in slots for t in (feats, rec_feats)], 0).cuda()
    ptr = torch.from_numpy(node_ptr)
    for tag, only in (('', False), ('_l', True)):
        ref = radius_graph(pos, x[:, -1], ptr, r_inter, r_intra, need_backward=False, ligand_pairs_only=only)
        assert int(f['rowptr' + tag][n_cap]) == ref.n_edges
        assert torch.equal(f['rowptr' + tag][:n + 1], ref.t['rowptr'])
        for k in ('row', 'col', 'etype'):
            assert torch.equal(f[k + tag][:ref.n_edges], ref.t[k][:ref.n_edges]), k + tag
        assert bool((f['rowptr' + tag][n:] == ref.n_edges).all())         # padding rows: degree 0 ...
        if not only:
            assert torch.equal(f['inv_deg'][:n], ref.t['inv_deg'])
    assert bool((f['inv_deg'][n:] == 1).all())                          # ... and inv_deg 1
    # node tables == a torch gather
    graph_id = torch.arange(len(SIZES)).repeat_interleave(torch.from_numpy(np.diff(node_ptr)))
    assert torch.equal(f['node_graph'][:n].cpu(), graph_id.int()) and bool((f['node_graph'][n:] == -1).all())
    assert torch.equal(f['pos'][:n], pos) and torch.equal(f['x'][:n], x)
    is_rec = x[:, -1] > 0
    rec_index = torch.cat([torch.arange(N_REC) for _ in SIZES]).cuda()
    for name, src in (('base_magg', screen.rec_magg), ('base_xsum', screen.rec_xsum), ('base_deg', screen.rec_deg)):
        want = torch.zeros_like(f[name][:n])
        want[is_rec] = src[rec_index]
        assert torch.equal(f[name][:n], want), name
        assert bool((f[name][n:] == 0).all()), name
    assert bool((f['pos'][n:] == 0).all()) and bool((f['x'][n:] == 0).all())


def test_uniform_sizes_reproduce_the_pose_batch_builder():
    """Six slots of one 17-atom ligand: every output array == pvs_screen_graph_build's for the same poses."""
    from pointvs_amd.screening import LibraryScreen, ReceptorScreen
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(6002, n_lig=17)
    poses = random_poses(lig, 6, seed=9, max_shift=4.0)
    model = _model()
    for r_inter, r_intra in ((7.0, None), (6.0, 2.5)):
        old = ReceptorScreen(model, rec.cuda(), torch.cat([lig_feats, rec_feats], 0), 17, 6, r_inter, r_intra)
        assert old.fast_graph
        old._build_fast(poses.cuda())
        old.check()
        new = LibraryScreen(model, rec.cuda(), rec_feats, 6, 17, r_inter, r_intra)
        f = new.load([(lig_feats, pose) for pose in poses])._build()
        new.check()
        n = 6 * (17 + N_REC)
        assert new.n_cap == n
        for tag in ('', '_l'):
            e = int(old._fast['rowptr' + tag][n])
            assert torch.equal(f['rowptr' + tag], old._fast['rowptr' + tag])
            for k in ('row', 'col', 'etype'):
                assert torch.equal(f[k + tag][:e], old._fast[k + tag][:e]), k + tag
        assert torch.equal(f['inv_deg'], old._fast['inv_deg'])
        assert torch.equal(f['pos'], old.batcher.batch.pos) and torch.equal(f['x'], old.batcher.batch.x.float())
        assert torch.equal(f['node_ptr'], old._graph_ptr)
        for name in ('base_magg', 'base_xsum', 'base_deg'):
            assert torch.equal(f[name], getattr(old, name).reshape(f[name].shape)), name


def test_capacity_overflow_is_reported_and_nothing_is_written():
    from pointvs_amd.screening import LibraryScreen
    lig, rec, lig_feats, rec_feats = _set(6001)
    slots = _slots(lig, lig_feats, SIZES, seed=10, rec=rec)
    screen = LibraryScreen(_model(), rec.cuda(), rec_feats, len(SIZES), 64, 7.0).load(slots)
    f = screen._build()
    screen.check()
    e, el = int(f['rowptr'][screen.n_cap]), int(f['rowptr_l'][screen.n_cap])
    assert 0 < el < e
    for cap, cap_l in ((e - 1, el), (e, el - 1), (e // 2, el // 2)):
        f['cap'], f['cap_l'] = cap, cap_l
        for k in ('row', 'col', 'row_l', 'col_l'):
            f[k].fill_(-77)
        for k in ('etype', 'etype_l'):
            f[k].fill_(77)
        screen._build()
        with pytest.raises(RuntimeError, match='overflow'):
            screen.check()
        assert int(f['rowptr'][screen.n_cap]) == e and int(f['rowptr_l'][screen.n_cap]) == el
        for k in ('row', 'col', 'row_l', 'col_l'):       # the canaries, before and after `capacity` entries
            assert bool((f[k] == -77).all()), k
        for k in ('etype', 'etype_l'):
            assert bool((f[k] == 77).all()), k
    f['cap'], f['cap_l'] = e, el                          # exactly enough room: no flag
    screen._build()
    screen.check()
    assert bool((f['row'][:e] >= 0).all()) and bool((f['row'][e:] == -77).all())


FLAG_SETS = [dict(), dict(edge_attention=True, node_attention=True, tanh=True, residual=True),
             dict(k=64, normalize=True, graphnorm=True)]


@pytest.mark.parametrize('flags', FLAG_SETS + [dict(edge_residual=True)])
def test_library_screen_matches_the_plain_forward(flags):
    """Two consecutive mixed batches == model(Batch) of the same complexes built from oracle edge lists
    (rel 1e-5, the bound of the screening paths); edge_residual takes the plain forward on the mixed batch."""
    from pointvs_amd.graph import Batch
    from pointvs_amd.screening import LibraryScreen
    lig, rec, lig_feats, rec_feats = _set(6003)
    model = _model(1, num_layers=3, **flags)
    screen = LibraryScreen(model, rec.cuda(), rec_feats, len(SIZES), 64, 7.0)
    assert screen.reuse == (not flags.get('edge_residual', False))
    for k, sizes in enumerate((SIZES, (20, 0, 64, 33, 1, 7))):
        slots = _slots(lig, lig_feats, sizes, seed=40 + 10 * k, rec=rec)
        fast = screen(slots).reshape(-1)
        assert fast.shape[0] == len(sizes)
        with torch.no_grad():
            slow = model(Batch.from_data_list(_oracle_items(slots, rec, rec_feats, 7.0, 7.0)).to('cuda')).reshape(-1)
        err = float((fast - slow).abs().max() / slow.abs().max().clamp_min(1e-30))
        print(f'{flags} batch {k}: max|fast-slow|/max|slow| = {err:.3e}')
        assert err < 1e-5, err
    screen.check()


@needs_caching_allocator
def test_captured_library_step_replays_across_compositions():
    """ONE captured step, replayed on batches of other compositions (other sizes, an empty trailing slot, sizes
    summing to L_cap) == the eager LibraryScreen on the same batch, bit for bit."""
    from pointvs_amd.screening import LibraryScreen
    lig, rec, lig_feats, rec_feats = _set(6004)
    model = _model(2, num_layers=3, residual=True, edge_attention=True, tanh=True)
    comps = [(7, 20, 3), (5, 17, 1), (12, 9), (20, 20, 20)]           # B = 3, L_cap = 60
    batches = [_slots(lig, lig_feats, sizes, seed=70 + 10 * k, special=False) for k, sizes in enumerate(comps)]
    eager = LibraryScreen(model, rec.cuda(), rec_feats, 3, 20, 7.0)
    want = [eager(slots).reshape(-1).clone() for slots in batches]   # (first batch first: the same probe)
    eager.check()
    graph = LibraryScreen(model, rec.cuda(), rec_feats, 3, 20, 7.0).capture(batches[0])
    for k in (2, 3, 1, 0):
        got = graph.replay(batches[k]).reshape(-1).clone()
        assert torch.equal(got, want[k]), k
    graph.check()
    with pytest.raises(RuntimeError, match='graphnorm'):
        LibraryScreen(_model(2, graphnorm=True), rec.cuda(), rec_feats, 3, 20, 7.0).capture(batches[0])


@needs_caching_allocator
def test_run_library_end_to_end(tmp_path):
    """Five ligands (12, 9, 70, 12, 1 atoms; 7, 5, 3, 4, 2 poses), batch of 4: the 70-atom ligand takes its size
    bucket, the others 5 dense mixed batches; scores == the one-complex plain forward, 21 lines in library order."""
    from pointvs_amd.radius_graph import PoseBatcher
    from pointvs_amd.screening import ScreeningSweep
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(6005, n_lig=70)
    model = _model(2, num_layers=3)
    ligs = [('ligA', lig_feats[:12], lig[:12], 7), ('ligB', lig_feats[:9].roll(1, 0), lig[:9] * 0.9, 5),
            ('ligC', lig_feats, lig, 3), ('ligD', lig_feats[:12].roll(3, 0), lig[:12].flip(0), 4),
            ('ligE', lig_feats[5:6], lig[5:6], 2)]
    work = [(name, f, random_poses(pos, n, seed=20 + k, max_shift=3.0).cuda())
            for k, (name, f, pos, n) in enumerate(ligs)]
    sweep = ScreeningSweep(model, rec.cuda(), rec_feats, edge_radius=6.0, batch_size=4)
    got = sweep.run_library(work, predictions_file=tmp_path / 'library.txt')
    assert sorted(sweep.buckets) == [70]
    assert sweep.batches_run - math.ceil(3 / 4) == math.ceil(18 / 4) == 5
    assert list(got) == [name for name, _, _ in work]
    lines = (tmp_path / 'library.txt').read_text().splitlines()
    assert len(lines) == 21
    at = 0
    for name, f, poses in work:
        plain = PoseBatcher(rec.cuda(), torch.cat([f, rec_feats], 0), f.shape[0], 1, edge_radius=6.0)
        assert got[name].shape[0] == poses.shape[0]
        for k in range(poses.shape[0]):
            with torch.no_grad():
                want = torch.sigmoid(model(plain.load(poses[k:k + 1])).reshape(-1))[0]
            assert abs(float(got[name][k, 0]) - float(want)) < 1e-5 * max(1.0, abs(float(want))), (name, k)
            assert lines[at] == f'{float(got[name][k, 0]):.3f} | receptor {name}_pose{k}'
            at += 1


def _stale_case(kind, model, rec, rec_feats, lig, lig_feats):
    """(screen factory, batch) at the smallest shape with three contact-mask words and several ligand rows."""
    from pointvs_amd.screening import LibraryScreen, ReceptorScreen
    from pointvs_amd.synthetic import random_poses
    if kind == 'receptor':
        feats = torch.cat([lig_feats[:12], rec_feats], 0)
        return (lambda: ReceptorScreen(model, rec.cuda(), feats, 12, 3, 7.0),
                random_poses(lig[:12], 3, seed=5, max_shift=3.0).cuda())
    return (lambda: LibraryScreen(model, rec.cuda(), rec_feats, 3, 20, 7.0),
            _slots(lig, lig_feats, (7, 20, 3), seed=90, special=False))


def _change_first_layer(model):
    with torch.no_grad():
        model.layers[1].edge_mlp[0].weight.mul_(1.5)         # (in place: bumps the version counter)


@pytest.mark.parametrize('kind', ['receptor', 'library'])
def test_weights_changed_under_an_eager_screen_recomputes_the_sums(kind):
    """The first layer's weights change between two eager calls: the screen is stale, the next call recomputes the
    receptor-receptor sums (LibraryScreen: and re-points the builder's node-table struct at them) and equals a
    screen built on the changed model bit for bit (same kernels, inputs and order; no atomics)."""
    lig, rec, lig_feats, rec_feats = _set(6006)
    model = _model(3)
    make, batch = _stale_case(kind, model, rec, rec_feats, lig, lig_feats)
    screen = make()
    y0 = screen(batch).clone()
    assert not screen.stale()
    _change_first_layer(model)
    assert screen.stale()
    y1 = screen(batch).clone()
    assert not screen.stale()
    screen.check()
    fresh = make()
    y2 = fresh(batch).clone()
    fresh.check()
    assert torch.equal(y1, y2)
    assert not torch.equal(y0, y1)


@needs_caching_allocator
@pytest.mark.parametrize('kind', ['receptor', 'library'])
def test_weights_changed_under_a_captured_screen_is_refused(kind):
    """A captured step has the sums baked in: replay and the eager call both refuse once the weights changed."""
    lig, rec, lig_feats, rec_feats = _set(6006)
    model = _model(3)
    make, batch = _stale_case(kind, model, rec, rec_feats, lig, lig_feats)
    screen = make().capture(batch)
    screen.replay(batch)
    screen.check()
    _change_first_layer(model)
    assert screen.stale()
    with pytest.raises(RuntimeError, match='weights changed'):
        screen.replay(batch)
    with pytest.raises(RuntimeError, match='weights changed'):
        screen(batch)


def _fill_canaries(f):
    for k in ('row', 'col', 'row_l', 'col_l'):
        f[k].fill_(-77)
    for k in ('etype', 'etype_l'):
        f[k].fill_(77)


def _canaries_intact(f):
    return (all(bool((f[k] == -77).all()) for k in ('row', 'col', 'row_l', 'col_l')) and
            all(bool((f[k] == 77).all()) for k in ('etype', 'etype_l')))


def test_pose_batch_builder_at_capacity_reports_overflow_and_writes_nothing():
    """pvs_screen_graph_build (the uniform builder) at its capacities: one edge short in either CSR, or half of
    both, sets the overflow bit, keeps both edge counts and writes no entry; with exactly enough room there is no
    flag, every entry below the count is written and nothing behind it."""
    from pointvs_amd.screening import ReceptorScreen
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(6007, n_lig=5)
    poses = random_poses(lig, 2, seed=3, max_shift=2.0).cuda()
    screen = ReceptorScreen(_model(), rec.cuda(), torch.cat([lig_feats, rec_feats], 0), 5, 2, 6.0, 2.5)
    assert screen.fast_graph
    screen._build_fast(poses)
    screen.check()
    f, n = screen._fast, 2 * (5 + N_REC)
    e, el = int(f['rowptr'][n]), int(f['rowptr_l'][n])
    assert 0 < el < e
    for cap, cap_l in ((e - 1, el), (e, el - 1), (e // 2, el // 2)):
        f['cap'], f['cap_l'] = cap, cap_l
        _fill_canaries(f)
        screen._build_fast(poses)
        with pytest.raises(RuntimeError, match='overflow'):
            screen.check()
        assert int(f['rowptr'][n]) == e and int(f['rowptr_l'][n]) == el
        assert _canaries_intact(f)
    f['cap'], f['cap_l'] = e, el                          # exactly enough room: no flag
    _fill_canaries(f)
    screen._build_fast(poses)
    screen.check()
    for tag, count in (('', e), ('_l', el)):
        for k in ('row', 'col'):
            assert bool((f[k + tag][:count] >= 0).all()) and bool((f[k + tag][count:] == -77).all()), k + tag
        assert bool((f['etype' + tag][:count] <= 2).all()) and bool((f['etype' + tag][count:] == 77).all()), tag


BAD_LIG_PTR = [([1, 64, 64, 65, 129], 'first entry not 0'), ([0, 64, 60, 65, 129], 'descending'),
               ([0, 65, 65, 66, 129], 'a 65-atom slot'), ([0, 64, 64, 65, 257], 'beyond L_cap')]


def test_a_lig_ptr_that_is_no_table_gives_an_empty_graph():
    """Status bit 3 of pvs_screen_slots_build (PVS_SLOTS_RAGGED): a lig_ptr that is not a table of 0..64-atom slots inside L_cap
    (validated on the device) is reported as ValueError, the batch comes out as an empty graph of padding rows and
    no edge entry is written; the valid table afterwards reproduces the first build array for array."""
    from pointvs_amd.screening import LibraryScreen
    lig, rec, lig_feats, rec_feats = _set(6008)
    rec, rec_feats = rec[:65].contiguous(), rec_feats[:65].contiguous()
    sizes = (64, 0, 1, 64)
    slots = _slots(lig, lig_feats, sizes, seed=20, special=False)
    screen = LibraryScreen(_model(), rec.cuda(), rec_feats, 4, 64, 7.0).load(slots)
    assert screen.l_cap == 256
    f = screen._build()
    screen.check()
    torch.cuda.synchronize()
    names = ('rowptr', 'row', 'col', 'etype', 'rowptr_l', 'row_l', 'col_l', 'etype_l', 'inv_deg', 'node_ptr',
             'node_graph', 'pos', 'x', 'base_magg', 'base_xsum', 'base_deg')
    e, el = int(f['rowptr'][screen.n_cap]), int(f['rowptr_l'][screen.n_cap])
    assert 0 < el < e
    count = {'row': e, 'col': e, 'etype': e, 'row_l': el, 'col_l': el, 'etype_l': el}
    first = {k: f[k][:count.get(k)].clone() for k in names}
    good = screen.lig_ptr.clone()
    assert good.tolist() == [0, 64, 64, 65, 129]
    for table, what in BAD_LIG_PTR:
        screen.lig_ptr.copy_(torch.tensor(table, dtype=torch.int32))
        _fill_canaries(f)
        screen._build()
        with pytest.raises(ValueError, match='lig_ptr'):
            screen.check()
        assert bool((f['rowptr'] == 0).all()) and bool((f['rowptr_l'] == 0).all()), what
        assert _canaries_intact(f), what
        assert bool((f['inv_deg'] == 1).all()) and bool((f['node_graph'] == -1).all()), what
        for k in ('pos', 'x', 'base_magg', 'base_xsum', 'base_deg'):
            assert bool((f[k] == 0).all()), (what, k)
    screen.lig_ptr.copy_(good)
    screen._build()
    screen.check()
    for k in names:
        assert torch.equal(f[k][:count.get(k)], first[k]), k
