"""slot_graphnorm=True: every slot of a GraphNorm model's pose batch is normalised by its own rows (the slots' node_ptr as
the layers' segment table, PVS_GRAPHNORM_SEGMENTS), so a batched screen gives what a batch_size=1 screen gives.

A. The setup of tests/test_gpu_contact_masking.py (GraphNorm model, ligands of 3, 17 and 70 atoms, batch of 4):
   contact_masking against attribution.bond_masking one complex at a time within 4e-5 * max|raw| (the bound of that
   file) - which the same sweep WITHOUT the keyword misses; ligand_atom_masking and receptor_atom_masking likewise against
   the batch_size=1 sweep.
B. LibraryScreen(batch_size=4): a pose's score against the same pose in a batch_size=1 screen and against the fp64 oracle
   on that complex alone, within the screening paths' bound (1e-5 of the largest output, tests/test_gpu_graphnorm_screen.py),
   in two compositions, with an empty slot, with a struck slot; replays of the one captured step equal the eager step bit
   for bit; a cropped screen at batch 4 against the cropped screen at batch 1.
C. Keyword off, and models without GraphNorm: the same bits and the same launches; the refusals.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests._golden import needs_caching_allocator
from tests.test_gpu_contact_masking import _bond_scores_one_at_a_time
from tests.test_gpu_graphnorm_screen import MAX_LIG, N_REC, RADIUS, REL, _gn_model, _items, _oracle, _receptor
from tests.test_gpu_library_screen import _model, _slots
from tests.test_gpu_ligand_masking import _set, _single_head

pytestmark = pytest.mark.gpu

B = 4
# (pose 0 is in both; the second has an empty last slot)
COMPOSITIONS = [(7, 20, 3, 12), (7, 17, 9, 0)]
PROFILED = ('edge_fwd', 'edge_bwd', 'col_gather', 'graph_prepare', 'edge_fwd_partial', 'mask_graph', 'linear_mfma',
            'linear_chunk64', 'linear_chunk256', 'linear_generic', 'tsgemm_mfma', 'tsgemm_wide', 'tsgemm_colchunk',
            'tsgemm_narrow', 'tsgemm_tn8', 'tsgemm_tn32', 'colreduce4', 'colreduce', 'colreduce_chunk', 'node_mlp_fwd',
            'node_mlp_bwd', 'node_out_fwd', 'node_out_bwd', 'node_tail', 'node_wgrads', 'colreduce4_rows',
            'colreduce_rows', 'node_tail_rows', 'colreduce4_segments', 'colreduce_segments', 'node_tail_segments')


# ---- A. masking of hits ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _hits():
    """Model, receptor and the three hits of tests/test_gpu_contact_masking.py's GraphNorm case."""
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(8301, 70)
    items = []
    for k, n in enumerate((3, 17, 70)):
        pose = random_poses(lig[:n], 1, seed=300 + k, max_shift=3.0)[0].contiguous()
        items.append((f'lig{n}', lig_feats[:n].roll(k, 0).contiguous(), pose))
    return _single_head(12, graphnorm=True), rec, rec_feats, items


def _sweep(batch_size, **kw):
    from pointvs_amd.screening import ScreeningSweep
    model, rec, rec_feats, _ = _hits()
    return ScreeningSweep(model, rec.cuda(), rec_feats, 4.0, batch_size=batch_size, **kw)


@needs_caching_allocator
def test_contact_masking_of_a_batch_equals_bond_masking_one_complex_at_a_time():
    model, rec, rec_feats, items = _hits()
    slotted, coupled = _sweep(B, slot_graphnorm=True), _sweep(B)
    out = slotted.contact_masking(items, sigmoid=False, column=0)
    assert slotted.struck.graphnorm and slotted.struck._gn_slots and slotted.struck._captured      # the ONE captured step
    other = coupled.contact_masking(items, sigmoid=False, column=0)
    assert not coupled.struck._gn_slots and not coupled.struck._captured
    worst = 0.0
    for name, feats, pose in items:
        pairs, scores = out[name]
        assert torch.equal(other[name][0], pairs) and pairs.shape[0] > 0
        ref = _bond_scores_one_at_a_time(model, rec, rec_feats, feats, pose, pairs.cpu().tolist(), 4.0)
        bound = 4e-5 * float(slotted.contact_masking_raw[name].abs().max())
        gap = float(np.abs(scores.double().cpu().numpy() - ref).max())
        gap_coupled = float(np.abs(other[name][1].double().cpu().numpy() - ref).max())
        print(f'{name}: slot_graphnorm {gap:.3e}, without {gap_coupled:.3e}, bound {bound:.3e}, '
              f'largest score {np.abs(ref).max():.3e}')
        assert gap <= bound and float(scores.abs().max()) > 0, name
        worst = max(worst, gap_coupled / bound)
    assert worst > 1.0, 'without the keyword the copies of a batch normalise each other: the inputs must show it'


@needs_caching_allocator
@pytest.mark.parametrize('method', ['ligand_atom_masking', 'receptor_atom_masking'])
def test_atom_masking_of_a_batch_equals_the_batch_of_one(method):
    _, _, _, items = _hits()
    kw = dict(sigmoid=False, column=0, **(dict(atoms='contacts') if method == 'receptor_atom_masking' else {}))
    slotted, coupled, alone = _sweep(B, slot_graphnorm=True), _sweep(B), _sweep(1)
    got, other, want = (getattr(s, method)(items, **kw) for s in (slotted, coupled, alone))
    raws = slotted.atom_masking_raw if method == 'ligand_atom_masking' else slotted.receptor_atom_masking_raw
    pick = (lambda v: v) if method == 'ligand_atom_masking' else (lambda v: v[1])
    worst = 0.0
    for name, _, _ in items:
        if method == 'receptor_atom_masking':
            assert torch.equal(got[name][0], want[name][0])
        bound = 4e-5 * float(raws[name].abs().max())
        gap = float((pick(got[name]) - pick(want[name])).abs().max())
        gap_coupled = float((pick(other[name]) - pick(want[name])).abs().max())
        print(f'{method} {name}: slot_graphnorm {gap:.3e}, without {gap_coupled:.3e}, bound {bound:.3e}')
        assert pick(got[name]).numel() > 0 and gap <= bound, (method, name)
        worst = max(worst, gap_coupled / bound)
    assert worst > 1.0, 'without the keyword the copies of a batch normalise each other: the inputs must show it'


# ---- B. the library screen -------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _batches():
    lig, _, lig_feats, _ = _receptor()
    first = _slots(lig, lig_feats, COMPOSITIONS[0], seed=900, special=False)
    second = [first[0]] + _slots(lig, lig_feats, COMPOSITIONS[1], seed=950, special=False)[1:]
    return [first, second]


def _screen(batch_size, name='k32', **kw):
    from pointvs_amd.screening import LibraryScreen
    _, rec, _, rec_feats = _receptor()
    return LibraryScreen(_gn_model(name), rec.cuda(), rec_feats, batch_size, MAX_LIG, RADIUS, **kw)


def _one_by_one(slots, rec_drop=None, **kw):
    """Every non-empty slot through a screen of batch size 1 (its own batch: GraphNorm over that complex alone)."""
    single = _screen(1, **kw)
    out = []
    for k, slot in enumerate(slots):
        if slot[1].shape[0] == 0:
            out.append(None)
            continue
        y = single.load([slot], rec_drop=[rec_drop[k]])() if rec_drop is not None else single([slot])
        out.append(y.reshape(-1).clone())
    single.check()
    return out


def _assert_slots(got, want, slots, what, oracle_drop='whole'):
    """got [B] against the batch-of-one scores `want` and, per slot, against the fp64 oracle on that complex alone."""
    scale = max(float(w.abs().max()) for w in want if w is not None)
    for k, slot in enumerate(slots):
        if want[k] is None:
            continue
        gap = float((got[k] - want[k]).abs().max())
        print(f'{what} slot {k} ({slot[1].shape[0]} atoms): against the batch of one {gap:.3e}, bound {REL * scale:.3e}')
        assert gap <= REL * scale, (what, k)
        if oracle_drop is not None:
            drop = None if oracle_drop == 'whole' else [oracle_drop[k]]
            ref = _oracle('k32', _items([slot], drop))
            err = float((got[k].double().cpu() - ref).abs().max() / ref.abs().max().clamp_min(1e-30))
            assert err < REL, (what, k, err)


@needs_caching_allocator
def test_a_poses_score_does_not_depend_on_what_shares_its_batch():
    batches = _batches()
    eager = _screen(B, slot_graphnorm=True)
    assert eager.reuse and eager.graphnorm and eager._gn_padded and eager._gn_slots and not eager.padded_graphnorm
    kept = [eager(slots).reshape(-1).clone() for slots in batches]
    eager.check()
    assert set(eager._fast['pgs']) == {eager.n_cap}                     # one graph pair, at the padded shape
    pg, g_lig = eager._fast['pgs'][eager.n_cap]
    assert pg.norm_segments is eager._fast['node_ptr'] and g_lig.n_graphs == B
    assert g_lig.n_norm_rows_dev == eager._fast['node_ptr'].data_ptr()
    for slots, got, sizes in zip(batches, kept, COMPOSITIONS):
        _assert_slots(got, _one_by_one(slots), slots, f'composition {sizes}')
    # the shared pose: one score, whatever shares its batch (two fp32 evaluations of the same complex)
    assert float((kept[0][0] - kept[1][0]).abs()) <= REL * float(kept[0].abs().max())
    # ... which the same screen under whole-batch statistics does not give
    coupled = _screen(B, padded_graphnorm=True)
    a, b = (coupled(slots).reshape(-1).clone() for slots in batches)
    assert float((a[0] - b[0]).abs()) > REL * float(a.abs().max()), 'the compositions must show the coupling'
    # replays of ONE captured step: the eager step's bits; padded_graphnorm beside the keyword changes nothing
    graph = _screen(B, slot_graphnorm=True, padded_graphnorm=True).capture(batches[0])
    assert graph._captured and graph._gn_slots
    for k in (1, 0, 1):
        assert torch.equal(graph.replay(batches[k]).reshape(-1), kept[k]), k
    graph.check()


@needs_caching_allocator
def test_a_struck_slot_is_a_shorter_segment():
    slots = _batches()[0]
    rec_drop = [-1, 17, -1, 3]
    screen = _screen(B, struck=True, slot_graphnorm=True)
    screen.load(slots, rec_drop=rec_drop)
    got = screen().reshape(-1).clone()
    screen.check()
    assert int(screen._fast['node_ptr'][B]) == sum(COMPOSITIONS[0]) + B * N_REC - 2
    _assert_slots(got, _one_by_one(slots, rec_drop, struck=True), slots, 'struck', oracle_drop=rec_drop)
    screen.capture()
    screen.load(slots, rec_drop=rec_drop)
    assert torch.equal(screen.replay().reshape(-1), got)


@needs_caching_allocator
def test_a_cropped_screen_at_batch_four_equals_the_cropped_screen_at_batch_one():
    crop = 5.0
    for slots, sizes in zip(_batches(), COMPOSITIONS):
        screen = _screen(B, crop_radius=crop, slot_graphnorm=True)
        assert screen.route == 'cropped' and screen._gn_slots
        got = screen(slots).reshape(-1).clone()
        screen.check()
        assert screen._fast['pg'].norm_segments is screen._fast['node_ptr']
        kept_rows = int(screen._fast['node_ptr'][B])
        assert sum(sizes) < kept_rows < sum(sizes) + B * N_REC          # (the crop drops receptor atoms)
        want = _one_by_one(slots, crop_radius=crop, padded_graphnorm=True)
        _assert_slots(got, want, slots, f'cropped {sizes}', oracle_drop=None)
        screen.capture()
        assert torch.equal(screen.replay(slots).reshape(-1), got)


# ---- C. off means off; refusals -----------------------------------------------------------------------------------------
def _launches(run):
    """({name: launches} over every profiled category, the result) of run()."""
    from pointvs_amd import _lib
    lib = _lib.lib()
    lib.pvs_profile_reset()
    lib.pvs_profile_enable(1 | sum(1 << (k + 1) for k in range(len(PROFILED))))
    try:
        out = run()
        torch.cuda.synchronize()
    finally:
        lib.pvs_profile_enable(0)
    counts = {}
    ms, cnt = C.c_double(), C.c_int64()
    for name in PROFILED:
        assert lib.pvs_profile_read(name.encode(), C.byref(ms), C.byref(cnt)) == 0, name
        counts[name] = cnt.value
    lib.pvs_profile_reset()
    return counts, out


def test_the_keyword_off_and_models_without_graphnorm_launch_what_they_launched():
    from pointvs_amd.screening import LibraryScreen
    _, rec, _, rec_feats = _receptor()
    batches = _batches()
    plain = _model(3, num_layers=2).cuda()
    made = [LibraryScreen(plain, rec.cuda(), rec_feats, B, MAX_LIG, RADIUS, **kw) for kw in ({}, dict(slot_graphnorm=True))]
    assert not made[1]._gn_slots and not made[1]._gn_padded
    for screen in made:
        screen(batches[0])          # (the probe and the lazy allocations)
    (base, y0), (with_kw, y1) = (_launches(lambda s=s: s(batches[1]).clone()) for s in made)
    assert torch.equal(y0, y1) and base == with_kw and sum(base.values()) > 0
    assert not with_kw['colreduce4_segments'] and not with_kw['node_tail_segments']
    assert not made[1]._fast['pgs'][made[1].n_cap][0].c.n_norm_rows_dev
    # a GraphNorm model with the keyword off: the exact-count route as always
    off = [_screen(B), _screen(B, slot_graphnorm=False)]
    for screen in off:
        screen(batches[0])
    (base, y0), (with_kw, y1) = (_launches(lambda s=s: s(batches[1]).clone()) for s in off)
    assert torch.equal(y0, y1) and base == with_kw and not base['node_tail_segments'] and base['node_tail'] > 0
    # and on: the segment kernels run instead of the whole-batch ones
    on = _screen(B, slot_graphnorm=True)
    on(batches[0])
    counts, _ = _launches(lambda: on(batches[1]).clone())
    n_gn = sum(1 for layer in on.egnn if layer.graphnorm)
    assert counts['node_tail_segments'] == n_gn and counts['colreduce4_segments'] == 2 * n_gn and not counts['node_tail']


def test_refusals():
    from pointvs_amd.screening import LibraryScreen, ScreeningSweep
    lig, rec, lig_feats, rec_feats = _receptor()
    args = (rec.cuda(), rec_feats, B, MAX_LIG, RADIUS)
    # the plain route (a hidden size the first-layer reuse is not built for) has no fixed-shape step to normalise in
    wide = _model(3, k=48, graphnorm=True, num_layers=2).cuda()
    with pytest.raises(NotImplementedError, match='slot_graphnorm'):
        LibraryScreen(wide, *args, slot_graphnorm=True)
    assert not LibraryScreen(wide, *args).reuse
    # ... a model without GraphNorm there: the keyword changes nothing
    assert not LibraryScreen(_model(3, k=48, num_layers=2).cuda(), *args, slot_graphnorm=True)._gn_slots
    with pytest.raises(NotImplementedError, match='fp32 only'):
        LibraryScreen(_model(3, graphnorm=True, num_layers=2).double().cuda(), *args, slot_graphnorm=True)
    # a cropped screen of a GraphNorm model takes either keyword
    with pytest.raises(ValueError, match='slot_graphnorm=True'):
        LibraryScreen(_gn_model('k32'), *args, crop_radius=5.0)
    assert LibraryScreen(_gn_model('k32'), *args, crop_radius=5.0, slot_graphnorm=True)._gn_slots
    # the per-ligand route of the sweep
    sweep = ScreeningSweep(_gn_model('k32'), rec.cuda(), rec_feats, RADIUS, batch_size=B, slot_graphnorm=True)
    poses = lig[:9].unsqueeze(0).cuda()
    with pytest.raises(ValueError, match='run_library'):
        sweep.run([('a', lig_feats[:9], poses)])
    with pytest.raises(ValueError, match='run_library'):          # a ligand above max_lig_atoms would take that route too
        sweep.run_library([('a', lig_feats[:9], poses)], sigmoid=False, max_lig_atoms=4)
    got = sweep.run_library([('a', lig_feats[:9], poses)], sigmoid=False, max_lig_atoms=MAX_LIG)
    assert sweep.library._gn_slots and got['a'].shape[0] == 1
    # a sweep of a model without GraphNorm runs as always
    free = ScreeningSweep(_model(3, num_layers=2).cuda(), rec.cuda(), rec_feats, RADIUS, batch_size=B, slot_graphnorm=True)
    assert free.run([('a', lig_feats[:9], poses)], sigmoid=False)['a'].shape[0] == 1
