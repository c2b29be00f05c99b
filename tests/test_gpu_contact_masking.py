"""Contact and receptor-atom masking of hits through the library screen (ScreeningSweep.contact_masking /
receptor_atom_masking over LibraryScreen(struck=True)) against the fixtures recorded from the reference's bond_masking
and atom_masking (tests/golden/attr_*ball*.npz: 12 or 30 ligand atoms first, r = 4.0, three layers of k = 32, so the
first-layer reuse applies), against hand-built struck slots, against pointvs_amd.attribution one complex at a time, and
end to end after run_library.

Bounds: the project's parity bound of the fixture, AttrCase.bound() = 1e-5 * max|raw64| + 4 * noise32 (1.59e-6 for the
bond fixtures), on the raw rows; 2 * bound + 2 * noise32 on the scores against the reference's own fp32 scores
(tests/test_gpu_attribution.py). What tells a right copy from a wrong one: on column 1 the smallest recorded effect of
a pair is 1.0e-3; on column 0 every pair copy differs from the copy without its ligand atom alone by at least 1.79e-5
and from the copy without its receptor atom alone by at least 2.9e-4 (the fp64 oracle, computed in the test) - a packer
that forgets either atom cannot pass. (Not so on column 1: one contact's receptor atom moves it by only 1.5e-6.)

Screens built on other batches: each raw output of a screen is within 1e-5 * max|raw| of the plain forward (the
screening paths' bound, tests/test_gpu_two_head_screen.py), so a difference of two outputs of one route is within
4e-5 * max|raw| of the same difference of another (tests/test_gpu_ligand_masking.py).
"""
import re

import numpy as np
import pytest
import torch

from tests._attribution_ref import AttrCase, oracle_outputs
from tests._golden import needs_caching_allocator
from tests.test_gpu_ligand_masking import (_fixture_model, _library, _set, _single_head, _two_headed)

pytestmark = pytest.mark.gpu

N_LIG = 12


def _pairs_of(c):
    """(rows of `visited` - the first edge of every unordered pair, by ligand atom then receptor atom -, pairs [K, 2]
    with the receptor atom counted inside the receptor)."""
    d = c.drop_table()
    _, first = np.unique(d[:, 0] * c.n + d[:, 1], return_index=True)
    return first, d[first] - np.array([0, N_LIG])


_ORACLE = {}


def _single_atom_copies(c, pairs):
    """The fp64 oracle's column 0 for every pair copy's two wrong neighbours: without the ligand atom alone, without
    the receptor atom alone. Once per fixture."""
    if c.name not in _ORACLE:
        lig_only = oracle_outputs(c, drop=np.stack([pairs[:, 0], np.full(len(pairs), -1)], 1))[1:, 0]
        rec_only = oracle_outputs(c, drop=np.stack([pairs[:, 1] + N_LIG, np.full(len(pairs), -1)], 1))[1:, 0]
        _ORACLE[c.name] = (lig_only, rec_only)
    return _ORACLE[c.name]


@pytest.mark.parametrize('capture', [pytest.param(True, marks=needs_caching_allocator), False], ids=['captured', 'eager'])
@pytest.mark.parametrize('name', ['attr_dimout3_ball120', 'attr_multitask_reg_ball120'])
def test_parity_with_the_recorded_bond_masking(name, capture):
    from pointvs_amd.screening import ScreeningSweep
    c = AttrCase(name)
    assert c.fn == 'bond_masking' and int((c.x[:, -1] == 0).sum()) == N_LIG and bool((c.x[:N_LIG, -1] == 0).all())
    assert c.raw64.shape == (171, 3)
    first, want_pairs = _pairs_of(c)
    assert want_pairs.shape == (85, 2)
    model = _fixture_model(c)
    sweep = ScreeningSweep(model, c.pos[N_LIG:].cuda(), c.x[N_LIG:].float(), 4.0, batch_size=5, capture=capture)
    out = sweep.contact_masking([('hit', c.x[:N_LIG].float(), c.pos[:N_LIG])], sigmoid=c.sigmoid)
    assert sweep.struck.reuse and sweep.struck._captured == capture and sweep.library is None and sweep.masking is None
    assert sweep.batches_run == 1 + -(-(85 + 1) // 5)            # (a new screen: the sizing batch, then the steps)
    pairs, scores = out['hit']
    assert list(out) == ['hit'] and np.array_equal(pairs.cpu().numpy(), want_pairs) and scores.shape == (85,)
    raw = sweep.contact_masking_raw['hit'].double().cpu().numpy()
    ref = c.raw64[np.concatenate([[0], 1 + first])]             # the unmasked graph, then the first edge of each pair
    assert raw.shape == ref.shape == (86, 3)
    bound = c.bound()
    err = float(np.abs(raw - ref).max())
    effect = float(np.abs(ref[0, 1] - ref[1:, 1]).min())
    print(f'{name} capture={capture}: raw err {err:.3e} bound {bound:.3e} smallest pair effect (column 1) {effect:.3e}')
    assert effect > 10 * bound
    lig_only, rec_only = _single_atom_copies(c, want_pairs)
    gaps = (float(np.abs(ref[1:, 0] - lig_only).min()), float(np.abs(ref[1:, 0] - rec_only).min()))
    print(f'{name}: column 0, pair copy against ligand-atom-only copy {gaps[0]:.3e}, receptor-atom-only {gaps[1]:.3e}')
    assert min(gaps) > 10 * bound
    assert err <= bound, f'{name}: |raw - raw64| = {err:.3e} > {bound:.3e}'
    # the reference's rule picks column 1 of the three; scores against its own fp32 scores
    assert torch.equal(scores, sweep.contact_masking_raw['hit'][0, 1] - sweep.contact_masking_raw['hit'][1:, 1])
    s_err = float(np.abs(scores.double().cpu().numpy() - c.scores[c.visited[first]]).max())
    print(f'{name} capture={capture}: score err {s_err:.3e} bound {2 * bound + 2 * c.noise32:.3e}')
    assert s_err <= 2 * bound + 2 * c.noise32


@pytest.mark.parametrize('name,n_lig,n_contact,atoms', [('attr_clidefault_ball120', 12, 46, 'contacts'),
                                                        ('attr_clidefault_ball400', 30, 65, 'contacts'),
                                                        ('attr_clidefault_ball120', 12, 108, 'all'),
                                                        ('attr_sigmoid_ball120', 12, 46, 'contacts')])
def test_receptor_atoms_against_the_recorded_atom_masking(name, n_lig, n_contact, atoms):
    from pointvs_amd import functional as PF
    from pointvs_amd.screening import ScreeningSweep
    c = AttrCase(name)
    assert c.fn == 'atom_masking' and int((c.x[:, -1] == 0).sum()) == n_lig and c.raw64.shape[0] == 1 + c.n
    model = _fixture_model(c)
    sweep = ScreeningSweep(model, c.pos[n_lig:].cuda(), c.x[n_lig:].float(), 4.0, batch_size=5)
    out = sweep.receptor_atom_masking([('hit', c.x[:n_lig].float(), c.pos[:n_lig])], atoms=atoms, sigmoid=c.sigmoid)
    which, scores = out['hit']
    which = which.cpu().numpy()
    if atoms == 'contacts':
        pairs, _ = PF.contact_pairs(c.pos[:n_lig].float().cuda(), torch.tensor([0, n_lig], dtype=torch.int32).cuda(),
                                    c.pos[n_lig:].float().cuda(), 4.0)
        assert np.array_equal(which, np.unique(pairs[:, 1].cpu().numpy()))
    else:
        assert np.array_equal(which, np.arange(c.n - n_lig))
    assert len(which) == n_contact and scores.shape == (n_contact,)
    assert sweep.batches_run == 1 + -(-(n_contact + 1) // 5)
    raw = sweep.receptor_atom_masking_raw['hit'].double().cpu().numpy()
    ref = c.raw64[np.concatenate([[0], 1 + n_lig + which])]
    assert raw.shape == ref.shape
    bound = c.bound()
    err = float(np.abs(raw - ref).max())
    effect = float(np.abs(ref[0] - ref[1:]).min())
    print(f'{name} {atoms}: raw err {err:.3e} bound {bound:.3e} smallest atom effect {effect:.3e}')
    if atoms == 'contacts':
        assert effect > 10 * bound                  # (not over all atoms: 4 of the 108 move the output by less)
    assert err <= bound, f'{name}: |raw - raw64| = {err:.3e} > {bound:.3e}'
    if c.sigmoid:
        s_err = float(np.abs(scores.double().cpu().numpy() - c.scores[n_lig + which]).max())
        print(f'{name}: score err {s_err:.3e} bound {2 * bound + 2 * c.noise32:.3e}')
        assert s_err <= 2 * bound + 2 * c.noise32
    else:
        assert torch.equal(scores, sweep.receptor_atom_masking_raw['hit'][0, 0] - sweep.receptor_atom_masking_raw['hit'][1:, 0])


# ---------------------------------------------------------------- hand-built slots, one complex at a time

def _bond_scores_one_at_a_time(model, rec, rec_feats, feats, pose, pairs, radius):
    """attribution.bond_masking on the one complex (ligand atoms first); its score of every pair's ligand -> receptor
    edge."""
    from pointvs_amd import attribution
    from pointvs_amd.radius_graph import generate_edges
    n = int(pose.shape[0])
    pos = torch.cat([pose, rec], 0).cuda()
    x = torch.cat([feats, rec_feats], 0).cuda()
    _, ei, attrs = generate_edges(pos, x[:, -1].contiguous(), radius, radius, prune=False)
    scores = attribution.bond_masking(model, pos[None], x[None], edge_indices=ei,
                                      edge_attrs=torch.nn.functional.one_hot(attrs, 3))
    ei, cls = ei.cpu().numpy(), attrs.cpu().numpy()
    where = {(int(a), int(b)): e for e, (a, b) in enumerate(ei.T) if cls[e] == 1}
    return np.array([scores[where[int(a), n + int(r)]] for a, r in pairs])


@pytest.mark.parametrize('kind', [pytest.param('two-headed', marks=needs_caching_allocator), 'graphnorm'])
def test_same_bits_as_hand_built_slots_and_scores_of_one_complex_at_a_time(kind):
    from pointvs_amd.screening import LibraryScreen, ScreeningSweep
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(8301, 70)
    items = []
    for k, n in enumerate((3, 17, 70)):
        pose = random_poses(lig[:n], 1, seed=300 + k, max_shift=3.0)[0].contiguous()
        items.append((f'lig{n}', lig_feats[:n].roll(k, 0).contiguous(), pose))
    if kind == 'two-headed':
        model, tasks, width = _two_headed(11, dim_output=3, num_layers=3), 'both', 4
    else:
        model, tasks, width = _single_head(12, graphnorm=True), None, 1
    sweep = ScreeningSweep(model, rec.cuda(), rec_feats, 4.0, batch_size=4, tasks=tasks)
    if tasks == 'both':
        with pytest.raises(ValueError, match='column must be named'):
            sweep.contact_masking(items, sigmoid=False)
    out = sweep.contact_masking(items, sigmoid=False, column=0)
    assert sweep.struck.graphnorm == (kind == 'graphnorm') and sweep.struck._captured == (kind == 'two-headed')
    counts = [int(out[name][0].shape[0]) for name, _, _ in items]
    total = sum(counts) + len(items)
    print(f'{kind}: pairs per hit {counts}, {total} copies')
    assert 100 < total < 600 and all(counts)
    assert sweep.batches_run == 1 + -(-total // 4)
    slots, drops = [], []
    for name, feats, pose in items:
        slots.append((feats, pose))
        drops.append(-1)
        for a, r in out[name][0].cpu().tolist():
            keep = [i for i in range(pose.shape[0]) if i != a]
            slots.append((feats[keep].contiguous(), pose[keep].contiguous()))
            drops.append(r)
    screen = LibraryScreen(model, rec.cuda(), rec_feats, 4, 70, 4.0, tasks=tasks, struck=True)
    screen([(f, p) for _, f, p in reversed(items)])         # sized as the sweep's screen is: the largest whole ligands first
    want = torch.cat([screen.load(slots[k:k + 4], rec_drop=drops[k:k + 4])().reshape(4, -1).clone()
                      for k in range(0, len(slots), 4)], 0)[:len(slots)]
    screen.check()
    alone = out
    if kind == 'graphnorm':
        # GraphNorm takes its statistics over ALL nodes of a batch (attribution.couples_graphs), so the copies of one
        # batch normalise each other and attribution.bond_masking scores such a model one copy per forward: what a
        # sweep of batch_size 1 computes. (At batch 4 the two differ by the coupling itself, 7.4e-4 against a bound of
        # 5.3e-6 here: a property of the model, not of the route.) Same complexes, same bound.
        alone = ScreeningSweep(model, rec.cuda(), rec_feats, 4.0, batch_size=1).contact_masking(items, sigmoid=False,
                                                                                                column=0)
    at = 0
    for name, feats, pose in items:
        pairs, scores = out[name]
        k = pairs.shape[0]
        raw = sweep.contact_masking_raw[name]
        assert raw.shape == (k + 1, width)
        assert torch.equal(raw, want[at:at + k + 1]), name
        assert torch.equal(scores, raw[0, 0] - raw[1:, 0])
        assert torch.equal(alone[name][0], pairs)
        ref = _bond_scores_one_at_a_time(model, rec, rec_feats, feats, pose, pairs.cpu().tolist(), 4.0)
        gap = float(np.abs(alone[name][1].double().cpu().numpy() - ref).max())
        bound = 4e-5 * float(raw.abs().max())
        print(f'{kind} {name}: against bond_masking of the one complex {gap:.3e} bound {bound:.3e} '
              f'largest score {np.abs(ref).max():.3e}')
        assert gap <= bound and float(scores.abs().max()) > 0
        at += k + 1


@needs_caching_allocator
def test_all_whole_receptors_give_the_plain_screens_bits():
    """A struck screen whose every rec_drop is -1 against a plain LibraryScreen on the same batches, both with the same
    edge room: the edge kernels plan their grids and chunks from the room of the CSR they are given (edge_dispatch.h),
    so two screens of different room - a struck screen adds the touched rows' to its ligand-touching CSR - agree to
    the screening paths' bound, as any two screens sized from different first batches do, and bit for bit only at equal
    room (measured with the struck screen's larger room: the first two batches equal, the third off in the last bit).
    The builder itself writes the same bytes at any room (tests/test_gpu_struck_slots.py)."""
    from pointvs_amd.screening import LibraryScreen
    lig, rec, lig_feats, rec_feats = _set(8302, 70)
    model = _single_head(7, num_layers=3)
    batches = [[(lig_feats[:n].contiguous(), (lig[:n] + 0.1 * k).contiguous()) for n in sizes]
               for k, sizes in enumerate(([70, 3, 17, 1], [5, 0, 64], [65, 66, 9, 12]))]
    plain = LibraryScreen(model, rec.cuda(), rec_feats, 4, 70, 4.0)
    struck = LibraryScreen(model, rec.cuda(), rec_feats, 4, 70, 4.0, struck=True)
    f = struck.load(batches[0])._build()
    plain.load(batches[0])._build(capacities=(f['cap'], f['cap_l']))
    assert struck._struck_room() > 0 and plain._fast['cap_l'] == f['cap_l']
    for eager in (True, False):
        if not eager:
            plain.capture(batches[0])
            struck.capture(batches[0])
        for k, batch in enumerate(batches):
            a = (plain(batch) if eager else plain.replay(batch)).clone()
            b = (struck.load(batch, rec_drop=[-1] * len(batch))() if eager else struck.replay(batch)).clone()
            assert torch.equal(a, b) and bool(a.abs().sum() > 0), (eager, k)
    plain.check()
    struck.check()


# ---------------------------------------------------------------- end to end, errors

@needs_caching_allocator
def test_end_to_end_after_run_library(tmp_path):
    from pointvs_amd.screening import ScreeningSweep
    lig, rec, lig_feats, rec_feats = _set(8102, 70)
    work = _library(lig, lig_feats)
    model = _single_head(5, num_layers=3)
    sweep = ScreeningSweep(model, rec.cuda(), rec_feats, edge_radius=4.0, batch_size=4)
    sweep.run_library(work, hits_file=tmp_path / 'hits.txt')
    assert sweep.hits['ligNone'][0] == -1                         # a ligand without poses is skipped
    hits = list(sweep.best_poses(work))
    names = [name for name, _, _ in hits]
    assert names == ['ligA', 'ligB', 'ligC', 'ligD', 'ligE']
    before = sweep.batches_run
    out = sweep.contact_masking(sweep.best_poses(work), scores_file=tmp_path / 'contacts.txt')
    counts = [int(out[name][0].shape[0]) for name in names]
    assert list(out) == names and sum(counts) > 20
    assert sweep.batches_run - before == 1 + -(-(sum(counts) + len(names)) // 4)
    assert sweep.struck.max_lig_atoms == 70 and sweep.struck._captured and sweep.masking is None
    lines = (tmp_path / 'contacts.txt').read_text().splitlines()
    assert len(lines) == sum(counts)
    at = 0
    for name in names:
        pairs, scores = out[name]
        raw = sweep.contact_masking_raw[name]
        # one output: column 0; a classification model: the sigmoid
        assert torch.allclose(scores, torch.sigmoid(raw[0, 0]) - torch.sigmoid(raw[1:, 0]), rtol=0, atol=1e-6)
        for (a, r), v in zip(pairs.tolist(), scores.tolist()):
            assert re.fullmatch(r'-?\d+\.\d{6} \| receptor ' + re.escape(f'{name}_atom{a} atom{r}'), lines[at]), lines[at]
            assert lines[at] == f'{v:.6f} | receptor {name}_atom{a} atom{r}'
            at += 1
    # the same screen serves the receptor atoms of the same hits: no sizing batch again
    before = sweep.batches_run
    atoms = sweep.receptor_atom_masking(hits, scores_file=tmp_path / 'atoms.txt')
    m = [int(atoms[name][0].shape[0]) for name in names]
    assert sweep.batches_run - before == -(-(sum(m) + len(names)) // 4)
    for name in names:
        assert atoms[name][0].tolist() == sorted(set(out[name][0][:, 1].tolist()))
    lines = (tmp_path / 'atoms.txt').read_text().splitlines()
    assert len(lines) == sum(m)
    at = 0
    for name in names:                                             # (a hit without a contact has no line)
        for r, v in zip(atoms[name][0].tolist(), atoms[name][1].tolist()):
            assert lines[at] == f'{v:.6f} | receptor {name} atom{r}'
            at += 1
    # an index tensor applies to every hit
    picked = sweep.receptor_atom_masking(hits[:2], atoms=torch.tensor([3, 0, 149]), sigmoid=False)
    assert all(picked[n][0].tolist() == [3, 0, 149] and picked[n][1].shape == (3,) for n in names[:2])
    assert sweep.contact_masking([]) == {} and sweep.contact_masking_raw == {}
    assert sweep.receptor_atom_masking([]) == {} and sweep.receptor_atom_masking_raw == {}


def test_errors():
    from pointvs_amd.screening import MAX_SCREEN_LIGAND_ATOMS, LibraryScreen, ScreeningSweep
    lig, rec, lig_feats, rec_feats = _set(8103, 20)
    model = _single_head(6)
    sweep = ScreeningSweep(model, rec.cuda(), rec_feats, edge_radius=6.0, batch_size=4, capture=False)
    item = ('twice', lig_feats[:5], lig[:5])
    for method in (sweep.contact_masking, sweep.receptor_atom_masking):
        with pytest.raises(ValueError, match='unique'):
            method([item, ('other', lig_feats[:3], lig[:3]), item])
        n = MAX_SCREEN_LIGAND_ATOMS + 1
        with pytest.raises(ValueError, match="'huge' has 1025 atoms"):
            method([('huge', lig_feats[:1].expand(n, -1), torch.zeros(n, 3))])
        with pytest.raises(ValueError, match='column 1 of 1'):
            method([item], column=1)
    with pytest.raises(ValueError, match="'contacts', 'all'"):
        sweep.receptor_atom_masking([item], atoms='some')
    with pytest.raises(ValueError, match='receptor atoms 0..149'):
        sweep.receptor_atom_masking([item], atoms=torch.tensor([150]))
    with pytest.raises(NotImplementedError, match='fp32 only'):
        ScreeningSweep(_single_head(6).double(), rec.cuda().double(), rec_feats.double(), edge_radius=6.0,
                       batch_size=4).contact_masking([item])
    # models outside the first-layer reuse, by name
    for flags in (dict(edge_residual=True), dict(edge_attention=True, softmax_attention=True), dict(k=48)):
        other = ScreeningSweep(_single_head(6, **flags), rec.cuda(), rec_feats, edge_radius=6.0, batch_size=4)
        with pytest.raises(ValueError, match='pointvs_amd.attribution.bond_masking'):
            other.contact_masking([item])
    with pytest.raises(ValueError, match='cam'):
        LibraryScreen(model, rec.cuda(), rec_feats, 4, 20, 6.0, struck=True, cam=True)
    with pytest.raises(ValueError, match='contact_attention'):
        LibraryScreen(_single_head(6, edge_attention=True), rec.cuda(), rec_feats, 4, 20, 6.0, struck=True,
                      contact_attention=1)
    with pytest.raises(ValueError, match='column must be named'):
        ScreeningSweep(_two_headed(3), rec.cuda(), rec_feats, edge_radius=6.0, batch_size=4,
                       tasks='both').contact_masking([item])
    # a pair table the packer refuses, through the screen
    assert list(sweep.contact_masking([item])) == ['twice']
    screen = sweep.struck
    screen.load_leave_out_pairs(lig[:5].cuda(), lig_feats[:5].cuda(), torch.tensor([0, 5], dtype=torch.int32).cuda(),
                                torch.tensor([[5, 0]], dtype=torch.int32).cuda(),
                                torch.tensor([0, 1], dtype=torch.int32).cuda(), [0] * 4, 0,
                                torch.zeros(1, dtype=torch.int32).cuda())
    assert not screen.lig_ptr.any() and bool((screen.rec_drop == -1).all())
    with pytest.raises(ValueError, match='pair table'):
        screen.check_leave_out()
    with pytest.raises(ValueError, match='struck=True'):
        LibraryScreen(model, rec.cuda(), rec_feats, 4, 20, 6.0).load_leave_out_pairs(
            lig[:5].cuda(), lig_feats[:5].cuda(), torch.tensor([0, 5], dtype=torch.int32).cuda(),
            torch.zeros((0, 2), dtype=torch.int32).cuda(), torch.tensor([0, 0], dtype=torch.int32).cuda(), [5], 0,
            torch.zeros(1, dtype=torch.int32).cuda())
    assert list(sweep.contact_masking([item])) == ['twice']              # (the sweep is still usable)
