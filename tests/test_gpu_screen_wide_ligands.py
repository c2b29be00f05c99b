"""The pose-batch builders and the screening paths for ligands of more than 64 atoms (up to
screening.MAX_SCREEN_LIGAND_ATOMS = 1,024): a ligand atom's ligand-ligand contacts are ceil(n / 64) mask words, and every
lane-per-ligand-atom step of csrc/screen_graph.hip runs as that many trips. The builders are integer work: every array
is compared for equality with the numpy reference (tests/_radius_cases.py) and with radius_graph on the collated batch.
Shapes: 65 atoms (one word and one bit; the coincident atoms 0 and 64 in different words), 128 (two full words), 130
(the ligand-ligand probe 1-128 and the coincident atoms 0-129 both span words 0 and 2), 1,024 (the cap)."""
import ctypes as C
import math
import tempfile

import numpy as np
import pytest
import torch

from tests import _radius_cases as rc
from tests._golden import needs_caching_allocator

pytestmark = pytest.mark.gpu

N_REC = 130
KW = dict(dim_input=12, k=32, dim_output=1, num_layers=2, residual=False, edge_residual=False,
          edge_attention=False, normalize=False, tanh=False, dropout=0.0, graphnorm=False, update_coords=True,
          permutation_invariance=False, node_attention=False, gated_residual=False, rezero=False,
          softmax_attention=False, model_task='classification')
SHIFT = np.array([0.25, -0.5, 0.125], dtype=np.float32)


def _model(seed=0, **flags):
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    torch.manual_seed(seed)
    return SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **dict(KW, **flags)).eval()


def _feats(n_lig, n_rec, seed=3):
    """[n_lig + n_rec, 12] one-hot atom types, last column = bp (0 ligand, 1 receptor)."""
    rng = np.random.RandomState(seed)
    f = np.zeros((n_lig + n_rec, 12), dtype=np.float32)
    f[np.arange(n_lig + n_rec), rng.randint(0, 11, n_lig + n_rec)] = 1
    f[n_lig:, -1] = 1
    return torch.from_numpy(f)


def _csr(ref, n):
    """The CSR the builders make of a reference-order edge list: rows gathered stably (inside a row the inter block
    before the intra block, columns ascending in each)."""
    rows, cols, attrs = ref
    order = np.argsort(rows, kind='stable')
    deg = np.bincount(rows, minlength=n)
    return dict(rowptr=np.concatenate([[0], np.cumsum(deg)]).astype(np.int32), row=rows[order].astype(np.int32),
                col=cols[order].astype(np.int32), etype=attrs[order].astype(np.uint8),
                inv_deg=(np.float32(1) / np.maximum(deg, 1).astype(np.float32)))


def _assert_screen_csrs(f, n, n_alloc, pos, bp, ptr, inter, intra, what):
    """The builder's full and ligand-touching CSRs over the first n nodes == the reference per pose == radius_graph
    on the collated batch; rows from n on (padding) are empty. (tests/test_gpu_radius_decisions.py's helper.)"""
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
    return e


# ---- a. the uniform builder in the decision band ----
WIDE_POSE_SHAPES = ((65, 65), (128, 64), (130, 130))


@pytest.mark.parametrize('n_lig,n_rec,kind', [(n_lig, n_rec, kind) for n_lig, n_rec in WIDE_POSE_SHAPES
                                              for kind in ('inter', 'intra')])
def test_pose_batch_builder_in_the_band_with_several_ligand_words(n_lig, n_rec, kind):
    """pvs_screen_graph_build, two poses, the probed radius at the probe pair's distance -8..8 ulps (the ligand-
    receptor probe: last bit of the last receptor word; the ligand-ligand probe: atoms 1 and n_lig - 2)."""
    from pointvs_amd.screening import ReceptorScreen
    lig, rec = rc.pose_case(n_lig, n_rec)
    assert np.array_equal(lig[0], lig[-1]) and (n_lig - 1) // 64 != 0
    poses = np.stack([lig, lig + SHIFT])
    n = n_lig + n_rec
    pos = np.concatenate([np.concatenate([p, rec]) for p in poses]).astype(np.float32)
    feats = _feats(n_lig, n_rec)
    bp = np.tile(feats[:, -1].numpy().astype(np.int64), 2)
    ptr = np.array([0, n, 2 * n], dtype=np.int64)
    model = _model()
    sweeps = [sw for sw in rc.pose_sweeps(lig, rec) if sw[1] == kind]
    assert len(sweeps) == len(rc.KS) == 17
    counts = []
    for name, _, s, inter, intra in sweeps:
        screen = ReceptorScreen(model, torch.from_numpy(rec).cuda(), feats, n_lig, 2, inter, intra)
        assert screen.fast_graph
        screen._build_fast(torch.from_numpy(poses).cuda())
        screen.check()
        torch.cuda.synchronize()
        counts.append(_assert_screen_csrs(screen._fast, 2 * n, 2 * n, pos, bp, ptr, inter, intra,
                                          f'{n_lig}x{n_rec} {name}'))
    step = np.diff(counts)                 # the sweep crosses the decision between k = 0 and k = 1, nowhere else
    k0 = rc.KS.index(0)
    assert step[k0] > 0 and (np.delete(step, k0) == 0).all(), counts


# ---- b. the ragged builder ----
WIDE_SLOT_SIZES = (130, 0, 1, 65, 64, 128)


@pytest.mark.parametrize('n_rec,kind', [(n_rec, kind) for n_rec in (65, 130) for kind in ('inter', 'intra')])
def test_ragged_pose_builder_in_the_band_with_slots_of_up_to_130_atoms(n_rec, kind):
    """pvs_screen_slots_build (PVS_SLOTS_RAGGED) at slot_cap = 130 (three ligand words), slots of 130, 0, 1, 65, 64 and 128
    atoms: the same probes in slot 0."""
    from pointvs_amd.screening import LibraryScreen
    lig, rec = rc.pose_case(130, n_rec)
    feats = _feats(130, n_rec)
    lig_feats, rec_feats = feats[:130].contiguous(), feats[130:].contiguous()
    shifted = lig + SHIFT
    slot_pos = {0: lig, 2: shifted[5:6], 3: shifted[:65], 4: (lig - SHIFT)[:64], 5: (lig + 2 * SHIFT)[:128]}
    assert tuple(len(slot_pos.get(k, ())) for k in range(6)) == WIDE_SLOT_SIZES
    slots, parts, bps = [], [], []
    for k, size in enumerate(WIDE_SLOT_SIZES):
        p = slot_pos.get(k, lig[:0])
        slots.append((lig_feats[:size].contiguous(), torch.from_numpy(np.ascontiguousarray(p))))
        parts += [p, rec]
        bps += [np.zeros(size, dtype=np.int64), np.ones(n_rec, dtype=np.int64)]
    pos, bp = np.concatenate(parts).astype(np.float32), np.concatenate(bps)
    lig_ptr = np.concatenate([[0], np.cumsum(WIDE_SLOT_SIZES)])
    ptr = (lig_ptr + np.arange(7) * n_rec).astype(np.int64)
    n = int(ptr[-1])
    model = _model()
    sweeps = [sw for sw in rc.pose_sweeps(lig, rec) if sw[1] == kind]
    assert len(sweeps) == len(rc.KS)
    for name, _, s, inter, intra in sweeps:
        screen = LibraryScreen(model, torch.from_numpy(rec).cuda(), rec_feats, batch_size=6, max_lig_atoms=130,
                               edge_radius=inter, intra_radius=intra).load(slots)
        assert screen.slot_cap == 130 and screen.n_cap == 6 * (130 + n_rec)
        f = screen._build()
        screen.check()
        torch.cuda.synchronize()
        assert f['node_ptr'].cpu().tolist() == ptr.tolist()
        _assert_screen_csrs(f, n, screen.n_cap, pos, bp, ptr, inter, intra, f'ragged x{n_rec} {name}')
        assert bool((f['node_graph'][n:] == -1).all()) and bool((f['node_graph'][:n] >= 0).all())


def _set(seed, n_lig):
    """(ligand [n_lig,3], receptor [130,3], ligand feats, receptor feats): the 130 receptor atoms of a
    screening_set nearest its centre."""
    from pointvs_amd.synthetic import screening_set
    lig, rec, feats = screening_set(seed=seed, n_nodes=n_lig + 400, n_lig=n_lig)
    near = torch.argsort((rec - lig.mean(0)).norm(dim=1))[:N_REC].sort().values
    return lig, rec[near].contiguous(), feats[:n_lig].contiguous(), feats[n_lig:][near].contiguous()


def test_uniform_sizes_of_70_atoms_reproduce_the_pose_batch_builder():
    """Six slots of one 70-atom ligand: every output array == pvs_screen_graph_build's for the same poses."""
    from pointvs_amd.screening import LibraryScreen, ReceptorScreen
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(7002, n_lig=70)
    poses = random_poses(lig, 6, seed=9, max_shift=4.0)
    model = _model()
    for r_inter, r_intra in ((7.0, None), (6.0, 2.5)):
        old = ReceptorScreen(model, rec.cuda(), torch.cat([lig_feats, rec_feats], 0), 70, 6, r_inter, r_intra)
        assert old.fast_graph
        old._build_fast(poses.cuda())
        old.check()
        new = LibraryScreen(model, rec.cuda(), rec_feats, 6, 70, r_inter, r_intra)
        f = new.load([(lig_feats, pose) for pose in poses])._build()
        new.check()
        n = 6 * (70 + N_REC)
        assert new.n_cap == n
        for tag in ('', '_l'):
            e = int(old._fast['rowptr' + tag][n])
            assert e > 0 and torch.equal(f['rowptr' + tag], old._fast['rowptr' + tag])
            for k in ('row', 'col', 'etype'):
                assert torch.equal(f[k + tag][:e], old._fast[k + tag][:e]), k + tag
        assert torch.equal(f['inv_deg'], old._fast['inv_deg'])
        assert torch.equal(f['pos'], old.batcher.batch.pos) and torch.equal(f['x'], old.batcher.batch.x.float())
        assert torch.equal(f['node_ptr'], old._graph_ptr)
        for name in ('base_magg', 'base_xsum', 'base_deg'):
            assert torch.equal(f[name], getattr(old, name).reshape(f[name].shape)), name


# ---- c. the cap ----
@pytest.mark.parametrize('builder', ['uniform', 'ragged'])
def test_a_ligand_of_1024_atoms(builder):
    """At the cap: 1,024 ligand atoms (16 words) against 65 receptor atoms, one pose, inter 2.5 A / intra 1.5 A."""
    from pointvs_amd.screening import MAX_SCREEN_LIGAND_ATOMS, LibraryScreen, ReceptorScreen
    n_lig, n_rec, inter, intra = MAX_SCREEN_LIGAND_ATOMS, 65, 2.5, 1.5
    assert n_lig == 1024
    lig, rec = rc.pose_case(n_lig, n_rec)
    feats = _feats(n_lig, n_rec)
    n = n_lig + n_rec
    pos = np.concatenate([lig, rec]).astype(np.float32)
    bp = feats[:, -1].numpy().astype(np.int64)
    ptr = np.array([0, n], dtype=np.int64)
    if builder == 'uniform':
        screen = ReceptorScreen(_model(), torch.from_numpy(rec).cuda(), feats, n_lig, 1, inter, intra)
        assert screen.fast_graph
        screen._build_fast(torch.from_numpy(lig[None]).cuda())
        f = screen._fast
    else:
        screen = LibraryScreen(_model(), torch.from_numpy(rec).cuda(), feats[n_lig:].contiguous(), 1, n_lig, inter, intra)
        f = screen.load([(feats[:n_lig].contiguous(), torch.from_numpy(lig))])._build()
        assert f['node_ptr'].cpu().tolist() == [0, n]
    screen.check()
    torch.cuda.synchronize()
    e = _assert_screen_csrs(f, n, n, pos, bp, ptr, inter, intra, f'{builder} 1024')
    assert e > 10 * n_lig           # (a dense ligand: every word of most rows has bits)


def test_one_atom_above_the_cap_is_refused_by_name():
    from pointvs_amd import _lib
    from pointvs_amd.screening import LibraryScreen, ReceptorScreen, ScreeningSweep
    lig, rec = rc.pose_case(3, 65)
    trec, rec_feats = torch.from_numpy(rec).cuda(), _feats(0, 65)
    model = _model()
    with pytest.raises(ValueError, match='max_lig_atoms must be 1..1024'):
        LibraryScreen(model, trec, rec_feats, 2, 1025, 4.0)
    with pytest.raises(ValueError, match='max_lig_atoms must be 1..1024'):
        ScreeningSweep(model, trec, rec_feats, 4.0, batch_size=2).run_library([], max_lig_atoms=1025)
    screen = ReceptorScreen(model, trec, _feats(1025, 65), 1025, 1, 4.0)
    assert not screen.fast_graph
    with pytest.raises(RuntimeError, match='<= 1024 ligand atoms'):
        screen.capture(torch.zeros((1, 1025, 3), device='cuda'))
    # the C entry itself (host-side argument check: nothing is launched, the buffer is never touched)
    lib, buf = _lib.lib(), torch.zeros(64, dtype=torch.int32, device='cuda')
    p = _lib.ptr(buf)
    for n_lig in (1025, 0):
        code = lib.pvs_screen_graph_build(p, p, p, p, 1, n_lig, 65, 4.0, 4.0, 0, 0, p, p, p, p, p, p, p, p, p, p, p, 64,
                                          _lib.stream(buf.device))
        assert code != 0
        message = lib.pvs_last_error().decode()
        assert 'n_lig' in message and '1..1024' in message and str(n_lig) in message, message
    def state_bytes(slot_cap):       # of the shape (2, 64, 65): n_slots, lig_cap, n_rec
        job = _lib.PvsScreenSlotsJob(layout=_lib.SLOTS_RAGGED, n_slots=2, lig_cap=64, n_rec=65, slot_cap=slot_cap)
        return lib.pvs_screen_slots_state_bytes(C.byref(job))
    assert state_bytes(1025) == 0
    # (5644: what the positional entries before the job struct gave on the MI355X for slots of 64 atoms at this shape)
    assert state_bytes(1024) > state_bytes(64) == 5644


# ---- d. bad tables at a cap that is not 64 ----
def _fill_canaries(f):
    for k in ('row', 'col', 'row_l', 'col_l'):
        f[k].fill_(-77)
    for k in ('etype', 'etype_l'):
        f[k].fill_(77)


def _canaries_intact(f):
    return (all(bool((f[k] == -77).all()) for k in ('row', 'col', 'row_l', 'col_l')) and
            all(bool((f[k] == 77).all()) for k in ('etype', 'etype_l')))


def test_a_131_atom_slot_is_no_table_for_a_screen_of_130_atom_slots():
    """Status bit 3 at slot_cap = 130: a 131-atom slot is reported as ValueError, the batch comes out as an empty graph
    of padding rows and no edge entry is written; a 130-atom slot is accepted; the valid table afterwards reproduces
    the first build array for array."""
    from pointvs_amd.screening import LibraryScreen
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(7008, n_lig=130)
    rec, rec_feats = rec[:65].contiguous(), rec_feats[:65].contiguous()
    sizes = (130, 0, 1, 64)
    slots = [(lig_feats[:n].roll(k, 0).contiguous(), random_poses(lig[:n], 1, seed=20 + k, max_shift=3.0)[0].contiguous())
             for k, n in enumerate(sizes)]
    screen = LibraryScreen(_model(), rec.cuda(), rec_feats, 4, 130, 7.0).load(slots)
    assert screen.l_cap == 520 and screen.slot_cap == 130
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
    assert good.tolist() == [0, 130, 130, 131, 195]
    for table, what in (([0, 131, 131, 132, 196], 'a 131-atom slot'), ([0, 130, 130, 131, 521], 'beyond L_cap')):
        screen.lig_ptr.copy_(torch.tensor(table, dtype=torch.int32))
        _fill_canaries(f)
        screen._build()
        with pytest.raises(ValueError, match=r'lig_ptr.*0\.\.130-atom'):
            screen.check()
        assert bool((f['rowptr'] == 0).all()) and bool((f['rowptr_l'] == 0).all()), what
        assert _canaries_intact(f), what
        assert bool((f['inv_deg'] == 1).all()) and bool((f['node_graph'] == -1).all()), what
        for k in ('pos', 'x', 'base_magg', 'base_xsum', 'base_deg'):
            assert bool((f[k] == 0).all()), (what, k)
    screen.lig_ptr.copy_(good)             # (its first slot has 130 atoms)
    screen._build()
    screen.check()
    for k in names:
        assert torch.equal(f[k][:count.get(k)], first[k]), k


# ---- e. scores ----
def _plain_scores(model, rec, rec_feats, lig_feats, poses, radius, sigmoid):
    """The one-complex plain forward of every pose."""
    from pointvs_amd.radius_graph import PoseBatcher
    plain = PoseBatcher(rec.cuda(), torch.cat([lig_feats, rec_feats], 0), lig_feats.shape[0], 1, edge_radius=radius)
    out = []
    for k in range(poses.shape[0]):
        with torch.no_grad():
            y = model(plain.load(poses[k:k + 1])).reshape(-1)
        out.append(float(torch.sigmoid(y)[0] if sigmoid else y[0]))
    return out


def _assert_scores(got, want, what):
    for k, (g, w) in enumerate(zip(got, want)):
        print(f'{what} pose {k}: got {g:.8f} want {w:.8f} |diff| {abs(g - w):.2e}')
        assert abs(g - w) < 1e-5 * max(1.0, abs(w)), (what, k, g, w)


@needs_caching_allocator
@pytest.mark.parametrize('n_lig', [70, 130])
def test_receptor_screen_eager_and_captured_match_the_plain_forward(n_lig):
    """Batch of 4, 3-layer model, 130 receptor atoms: eager call and capture() + replay() on two different pose
    batches == model(batch) of each pose alone."""
    from pointvs_amd.screening import ReceptorScreen
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(7100 + n_lig, n_lig=n_lig)
    model = _model(1, num_layers=3)
    poses = random_poses(lig, 8, seed=31, max_shift=3.0).cuda()
    want = _plain_scores(model, rec, rec_feats, lig_feats, poses, 6.0, sigmoid=False)
    feats = torch.cat([lig_feats, rec_feats], 0)
    eager = ReceptorScreen(model, rec.cuda(), feats, n_lig, 4, 6.0)
    assert eager.fast_graph
    for k in (0, 4):
        _assert_scores(eager(poses[k:k + 4].contiguous()).reshape(-1).tolist(), want[k:k + 4], f'eager {n_lig} +{k}')
    eager.check()
    graph = ReceptorScreen(model, rec.cuda(), feats, n_lig, 4, 6.0).capture(poses[:4].contiguous())
    for k in (4, 0):
        _assert_scores(graph.replay(poses[k:k + 4]).reshape(-1).tolist(), want[k:k + 4], f'replay {n_lig} +{k}')
    graph.check()


LIBRARY = (('ligA', 12, 7), ('ligB', 70, 3), ('ligC', 130, 2), ('ligD', 9, 5), ('ligE', 140, 2))


@pytest.fixture(scope='module')
def library():
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(7005, n_lig=140)
    work = [(name, lig_feats[:n].roll(k, 0).contiguous(), random_poses(lig[:n], count, seed=20 + k, max_shift=3.0).cuda())
            for k, (name, n, count) in enumerate(LIBRARY)]
    return rec, rec_feats, work


@needs_caching_allocator
def test_run_library_with_a_boundary_of_130_atoms(library, tmp_path):
    """Ligands of 12, 70, 130, 9 and 140 atoms (7, 3, 2, 5, 2 poses), batch of 4, max_lig_atoms=130: the 140-atom
    ligand takes its size bucket, the others ceil(17 / 4) dense mixed batches; scores == the one-complex plain forward,
    19 lines in library order, then pose order."""
    from pointvs_amd.screening import ScreeningSweep
    rec, rec_feats, work = library
    model = _model(2, num_layers=3)
    sweep = ScreeningSweep(model, rec.cuda(), rec_feats, edge_radius=6.0, batch_size=4)
    got = sweep.run_library(work, tmp_path / 'library.txt', max_lig_atoms=130)
    assert sorted(sweep.buckets) == [140]
    assert sweep.library.max_lig_atoms == 130 and sweep.library.slot_cap == 130
    assert sweep.batches_run - math.ceil(2 / 4) == math.ceil(17 / 4) == 5
    assert list(got) == [name for name, _, _ in work]
    lines = (tmp_path / 'library.txt').read_text().splitlines()
    assert len(lines) == 19
    at = 0
    for name, f, poses in work:
        assert got[name].shape[0] == poses.shape[0]
        _assert_scores(got[name][:, 0].tolist(), _plain_scores(model, rec, rec_feats, f, poses, 6.0, sigmoid=True), name)
        for k in range(poses.shape[0]):
            assert lines[at] == f'{float(got[name][k, 0]):.3f} | receptor {name}_pose{k}'
            at += 1


@needs_caching_allocator
def test_run_library_keeps_its_default_boundary_of_64_atoms(library):
    from pointvs_amd.screening import ScreeningSweep
    rec, rec_feats, work = library
    sweep = ScreeningSweep(_model(2, num_layers=3), rec.cuda(), rec_feats, edge_radius=6.0, batch_size=4)
    got = sweep.run_library(work)
    assert sorted(sweep.buckets) == [70, 130, 140]
    assert sweep.library.max_lig_atoms == 12 and sweep.library.slot_cap == 64
    assert sweep.batches_run == math.ceil(12 / 4) + 3
    assert list(got) == [name for name, _, _ in work]
    assert all(sweep.buckets[n]._captured for n in (70, 130, 140))
