"""Ligand-atom masking of hits through the library screen: the leave-one-atom-out packer (PF.leave_out_ligand_pack,
pvs_leave_out_ligand_pack) bit for bit against a numpy construction, and ScreeningSweep.ligand_atom_masking against the
fixtures recorded from the reference's atom_masking (tests/golden/attr_*ball*.npz: ligand atoms first, r = 4.0, three
layers of k = 32, so the first-layer reuse applies), against hand-built leave-out slots, and end to end after
run_library.

Bounds: the project's parity bound of the fixture, AttrCase.bound() = 1e-5 * max|raw64| + 4 * noise32, on the raw rows;
2 * bound + 2 * noise32 on the scores against the reference's own fp32 scores (tests/test_gpu_attribution.py). The
smallest ligand-atom effect in these fixtures, |raw64[0] - raw64[1 + a]|, is 6.2e-4 (ball120) and 3.7e-5 (ball400)
against a bound of 1.3e-6: returning the unmasked score for every copy cannot pass.
"""
import re
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import _many_slots_cases as mc
from tests._attribution_ref import AttrCase
from tests._golden import needs_caching_allocator

pytestmark = pytest.mark.gpu

SIZES = [0, 1, 2, 5, 64, 65, 130]
F, N_SLOTS, SLOT_CAP, SENTINEL = 12, 7, 130, -7.0


# ---------------------------------------------------------------- the packer

def _ligands(sizes, n_feats=F):
    return mc.ligands(sizes, n_feats)


def _copies(pos, feats, ptr):
    """Every copy in order: (pos rows, feats rows)."""
    return [c[:2] for c in mc.ligand_copies(pos, feats, ptr)]


def _want(copies, first, n_slots, slot_cap, n_feats=F):
    return mc.packed_batch([c + (-1,) for c in copies], first, n_slots, slot_cap, n_feats, SENTINEL)[:3]


def _pack(pos, feats, ptr, first, n_slots, slot_cap):
    """One launch into sentinel-filled outputs; (pos, feats, ptr, status) as numpy."""
    from pointvs_amd import functional as PF
    rows = n_slots * slot_cap
    out = (torch.full((rows, 3), SENTINEL).cuda(), torch.full((rows, feats.shape[1]), SENTINEL).cuda(),
           torch.full((n_slots + 1,), 12345, dtype=torch.int32).cuda(), torch.full((1,), 77, dtype=torch.int32).cuda())
    got = PF.leave_out_ligand_pack(torch.from_numpy(pos).cuda(), torch.from_numpy(feats).cuda(),
                                   torch.from_numpy(ptr).cuda(), torch.tensor([first], dtype=torch.int32).cuda(),
                                   n_slots, slot_cap, out=out)
    assert all(g is o for g, o in zip(got, out))
    return tuple(t.cpu().numpy() for t in got)


def _firsts():
    total = sum(SIZES) + len(SIZES)
    firsts = list(range(0, total, N_SLOTS))
    assert total % N_SLOTS and firsts[-1] + N_SLOTS > total          # the last batch is partly empty
    return firsts + [total + 6]                                       # and one with every slot empty


def _run_all():
    pos, feats, ptr = _ligands(SIZES)
    return [_pack(pos, feats, ptr, first, N_SLOTS, SLOT_CAP) for first in _firsts()]


_RUNS = {}


def _first_run():
    if 'runs' not in _RUNS:
        _RUNS['runs'] = _run_all()
    return _RUNS['runs']


def test_packer_is_exact():
    pos, feats, ptr = _ligands(SIZES)
    copies = _copies(pos, feats, ptr)
    assert len(copies) == sum(SIZES) + len(SIZES) == 274
    for first, (got_pos, got_feats, got_ptr, status) in zip(_firsts(), _first_run()):
        want_pos, want_feats, want_ptr = _want(copies, first, N_SLOTS, SLOT_CAP)
        assert status[0] == 0, first
        assert np.array_equal(got_ptr, want_ptr), (first, got_ptr, want_ptr)
        # the written rows and the sentinels beyond out_ptr[n_slots], bit for bit
        assert got_pos.tobytes() == want_pos.tobytes(), first
        assert got_feats.tobytes() == want_feats.tobytes(), first
    assert not _first_run()[-1][2].any()                 # first_copy >= total: every slot empty
    # the allocating form gives the same rows
    from pointvs_amd import functional as PF
    out_pos, out_feats, out_ptr, status = PF.leave_out_ligand_pack(
        torch.from_numpy(pos).cuda(), torch.from_numpy(feats).cuda(), torch.from_numpy(ptr).cuda(),
        torch.tensor([35], dtype=torch.int32).cuda(), N_SLOTS, SLOT_CAP)
    want_pos, want_feats, want_ptr = _want(copies, 35, N_SLOTS, SLOT_CAP)
    n = int(want_ptr[-1])
    assert out_pos.shape == (N_SLOTS * SLOT_CAP, 3) and int(status) == 0
    assert np.array_equal(out_ptr.cpu().numpy(), want_ptr)
    assert np.array_equal(out_pos[:n].cpu().numpy(), want_pos[:n])
    assert np.array_equal(out_feats[:n].cpu().numpy(), want_feats[:n])


def test_packer_refuses_bad_tables():
    pos, feats, _ = _ligands([9])
    bad_tables = [(np.array([0, 5, 3, 9], dtype=np.int32), 1024),                 # descending
                  (np.array([0, 9], dtype=np.int32), 8),                          # a ligand of slot_cap + 1 atoms
                  (np.array([0, 4, 10], dtype=np.int32), 1024)]                   # ends outside the 9 rows
    for ptr, slot_cap in bad_tables:
        got_pos, got_feats, got_ptr, status = _pack(pos, feats, ptr, 0, 3, slot_cap)
        assert status[0] & 8, ptr
        assert not got_ptr.any(), (ptr, got_ptr)
        assert np.all(got_pos == SENTINEL) and np.all(got_feats == SENTINEL), ptr
    got = _pack(pos, feats, np.array([0, 9], dtype=np.int32), 0, 3, 9)            # (slot_cap atoms: fine)
    assert got[3][0] == 0 and got[2].tolist() == [0, 9, 17, 25]


def test_packer_is_reproducible():
    for a, b in zip(_first_run(), _run_all()):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_packer_wrapper_refuses_wrong_arguments():
    from pointvs_amd import functional as PF
    pos, feats, ptr = (torch.from_numpy(a).cuda() for a in _ligands([3, 2]))
    first = torch.zeros(1, dtype=torch.int32).cuda()
    with pytest.raises(TypeError):
        PF.leave_out_ligand_pack(pos.double(), feats, ptr, first, 2, 4)
    with pytest.raises(ValueError):
        PF.leave_out_ligand_pack(pos, feats, ptr.long(), first, 2, 4)
    with pytest.raises(ValueError):
        PF.leave_out_ligand_pack(pos, feats[:4], ptr, first, 2, 4)
    with pytest.raises(ValueError):
        PF.leave_out_ligand_pack(pos, feats, ptr, first.long(), 2, 4)
    with pytest.raises(ValueError):          # outputs too small for n_slots * slot_cap rows
        PF.leave_out_ligand_pack(pos, feats, ptr, first, 2, 4, out=(pos.new_zeros((7, 3)), feats.new_zeros((8, F)),
                                                                   ptr.new_zeros(3), ptr.new_zeros(1)))
    with pytest.raises(RuntimeError):
        PF.leave_out_ligand_pack(pos.cpu(), feats.cpu(), ptr.cpu(), first.cpu(), 2, 4)


# ---------------------------------------------------------------- parity with the reference's atom_masking

def _fixture_model(c):
    from pointvs_amd.egnn_multitask import MultitaskSatorrasEGNN
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    cls = SartorrasEGNN if c.meta['class'] == 'SartorrasEGNN' else MultitaskSatorrasEGNN
    model = cls(Path(tempfile.mkdtemp()), 2e-3, 1e-4, None, None, silent=True, **c.meta['kwargs'])
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in c.sd.items()})
    return model.to('cuda').eval()


@pytest.mark.parametrize('capture', [pytest.param(True, marks=needs_caching_allocator), False], ids=['captured', 'eager'])
@pytest.mark.parametrize('name,n_lig', [('attr_clidefault_ball120', 12), ('attr_clidefault_ball400', 30),
                                        ('attr_sigmoid_ball120', 12)])
def test_parity_with_the_reference_fixtures(name, n_lig, capture):
    from pointvs_amd.screening import ScreeningSweep
    c = AttrCase(name)
    assert c.fn == 'atom_masking' and int((c.x[:, -1] == 0).sum()) == n_lig and bool((c.x[:n_lig, -1] == 0).all())
    assert c.raw64.shape[0] == 1 + c.n
    model = _fixture_model(c)
    sweep = ScreeningSweep(model, c.pos[n_lig:].cuda(), c.x[n_lig:].float(), 4.0, batch_size=5, capture=capture)
    scores = sweep.ligand_atom_masking([('hit', c.x[:n_lig].float(), c.pos[:n_lig])], sigmoid=c.sigmoid)
    assert sweep.masking.reuse and sweep.masking._captured == capture and sweep.library is None
    assert sweep.batches_run == 1 + -(-(n_lig + 1) // 5)         # (a new screen: the sizing batch, then the steps)
    raw = sweep.atom_masking_raw['hit'].double().cpu().numpy()
    ref = c.raw64[:n_lig + 1]                      # the unmasked graph, then without ligand atom a (ligand atoms first)
    assert raw.shape == ref.shape
    bound = c.bound()
    err = float(np.abs(raw - ref).max())
    effect = float(np.abs(ref[0] - ref[1:]).min())
    print(f'{name} capture={capture}: raw err {err:.3e} bound {bound:.3e} smallest atom effect {effect:.3e}')
    assert effect > 10 * bound                      # (the bound tells a masked copy from the unmasked one)
    assert err <= bound, f'{name}: |raw - raw64| = {err:.3e} > {bound:.3e}'
    assert list(scores) == ['hit'] and scores['hit'].shape == (n_lig,)
    if c.sigmoid:
        s_err = float(np.abs(scores['hit'].double().cpu().numpy() - c.scores[:n_lig]).max())
        print(f'{name} capture={capture}: score err {s_err:.3e} bound {2 * bound + 2 * c.noise32:.3e}')
        assert s_err <= 2 * bound + 2 * c.noise32
        # the sweeps' default rule: a classification model's column gets the sigmoid
        again = sweep.ligand_atom_masking([('hit', c.x[:n_lig].float(), c.pos[:n_lig])])
        assert torch.equal(again['hit'], scores['hit'])


# ---------------------------------------------------------------- hand-built slots, end to end, errors

N_REC = 150
KW = dict(dim_input=12, k=32, dim_output=1, num_layers=2, residual=False, edge_residual=False,
          edge_attention=False, normalize=False, tanh=False, dropout=0.0, graphnorm=False, update_coords=True,
          permutation_invariance=False, node_attention=False, gated_residual=False, rezero=False,
          softmax_attention=False, model_task='classification')


def _two_headed(seed, **flags):
    from pointvs_amd.egnn_multitask import MultitaskSatorrasEGNN
    torch.manual_seed(seed)
    return MultitaskSatorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True,
                                 **dict(KW, final_softplus=True, **flags)).eval().cuda()


def _single_head(seed, **flags):
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    torch.manual_seed(seed)
    return SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **dict(KW, **flags)).eval().cuda()


def _set(seed, n_lig):
    """(ligand [n_lig,3], receptor [150,3], ligand feats, receptor feats): the 150 receptor atoms of a screening_set
    nearest its centre."""
    from pointvs_amd.synthetic import screening_set
    lig, rec, feats = screening_set(seed=seed, n_nodes=n_lig + 400, n_lig=n_lig)
    near = torch.argsort((rec - lig.mean(0)).norm(dim=1))[:N_REC].sort().values
    return lig, rec[near].contiguous(), feats[:n_lig].contiguous(), feats[n_lig:][near].contiguous()


@pytest.mark.parametrize('kind', [pytest.param('two-headed', marks=needs_caching_allocator), 'graphnorm'])
def test_same_bits_as_hand_built_slots(kind):
    """Ligands of 3, 17 and 130 atoms, batch of 4: the raw rows are what LibraryScreen gives for the same leave-out
    slots put together on the host (the packed inputs are the same, so the builder and the kernels are)."""
    from pointvs_amd.screening import LibraryScreen, ScreeningSweep
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(8101, 130)
    items = []
    for k, n in enumerate((3, 17, 130)):
        pose = random_poses(lig[:n], 1, seed=300 + k, max_shift=3.0)[0].contiguous()
        items.append((f'lig{n}', lig_feats[:n].roll(k, 0).contiguous(), pose))
    if kind == 'two-headed':
        model, tasks, width = _two_headed(11, dim_output=3, num_layers=3), 'both', 4
    else:
        model, tasks, width = _single_head(12, graphnorm=True), None, 1
    sweep = ScreeningSweep(model, rec.cuda(), rec_feats, 7.0, batch_size=4, tasks=tasks)
    scores = sweep.ligand_atom_masking(items, sigmoid=False, column=width - 1)
    assert sweep.masking.graphnorm == (kind == 'graphnorm') and sweep.masking._captured == (kind == 'two-headed')
    assert sweep.batches_run == 1 + -(-(3 + 17 + 130 + 3) // 4)
    slots = []
    for _, feats, pose in items:
        slots.append((feats, pose))
        for a in range(pose.shape[0]):
            keep = [i for i in range(pose.shape[0]) if i != a]
            slots.append((feats[keep].contiguous(), pose[keep].contiguous()))
    screen = LibraryScreen(model, rec.cuda(), rec_feats, 4, 130, 7.0, tasks=tasks)
    screen([(f, p) for _, f, p in reversed(items)])         # sized as the sweep's screen is: the largest whole ligands first
    want = torch.cat([screen(slots[k:k + 4]).reshape(4, -1).clone() for k in range(0, len(slots), 4)], 0)[:len(slots)]
    screen.check()
    at = 0
    for name, _, pose in items:
        n = pose.shape[0]
        raw = sweep.atom_masking_raw[name]
        assert raw.shape == (n + 1, width)
        assert torch.equal(raw, want[at:at + n + 1]), name
        assert torch.equal(scores[name], raw[0, width - 1] - raw[1:, width - 1])
        assert float(scores[name].abs().max()) > 0           # (an atom's removal changes the output)
        at += n + 1


def _library(lig, lig_feats):
    from pointvs_amd.synthetic import random_poses
    ligs = [('ligA', lig_feats[:12], lig[:12], 7), ('ligB', lig_feats[:9].roll(1, 0), lig[:9] * 0.9, 5),
            ('ligC', lig_feats, lig, 3), ('ligNone', lig_feats[:5], lig[:5], 0),
            ('ligD', lig_feats[:12].roll(3, 0), lig[:12].flip(0), 4), ('ligE', lig_feats[5:6], lig[5:6], 2)]
    return [(name, f, random_poses(pos, n, seed=20 + k, max_shift=3.0).cuda()) for k, (name, f, pos, n) in enumerate(ligs)]


@needs_caching_allocator
def test_end_to_end_after_run_library(tmp_path):
    """run_library with a hits file, then the masking of every hit: ligands of 12, 9, 70, 12 and 1 atoms (the 70-atom
    one went through its size bucket in the sweep) and one without poses, which is skipped."""
    from pointvs_amd.screening import ScreeningSweep
    lig, rec, lig_feats, rec_feats = _set(8102, 70)
    work = _library(lig, lig_feats)
    model = _single_head(5, num_layers=3)
    sweep = ScreeningSweep(model, rec.cuda(), rec_feats, edge_radius=6.0, batch_size=4)
    sweep.run_library(work, hits_file=tmp_path / 'hits.txt')
    assert sweep.hits['ligNone'][0] == -1
    hits = list(sweep.best_poses(work))
    assert [name for name, _, _ in hits] == ['ligA', 'ligB', 'ligC', 'ligD', 'ligE']
    for (name, feats, pose), (_, f, poses) in zip(hits, [w for w in work if w[0] != 'ligNone']):
        assert feats is f and torch.equal(pose, poses[sweep.hits[name][0]])
    before = sweep.batches_run
    scores = sweep.ligand_atom_masking(sweep.best_poses(work), scores_file=tmp_path / 'atoms.txt')
    sizes = [12, 9, 70, 12, 1]
    assert sweep.batches_run - before == 1 + -(-(sum(sizes) + len(sizes)) // 4)
    assert list(scores) == [name for name, _, _ in hits] and [int(s.shape[0]) for s in scores.values()] == sizes
    assert sweep.masking.max_lig_atoms == 70 and sweep.masking._captured and sweep.library.max_lig_atoms == 12
    lines = (tmp_path / 'atoms.txt').read_text().splitlines()
    assert len(lines) == sum(sizes)
    at = 0
    for name, s in scores.items():
        for a, v in enumerate(s.tolist()):
            assert re.fullmatch(r'-?\d+\.\d{6} \| receptor ' + re.escape(f'{name}_atom{a}'), lines[at]), lines[at]
            assert lines[at] == f'{v:.6f} | receptor {name}_atom{a}'
            at += 1
    # one ligand alone, raw differences: the same scores from another batch composition. Each raw output of a screen is
    # within 1e-5 * max|raw| of the plain forward (the screening paths' bound, tests/test_gpu_two_head_screen.py), so
    # two screens' outputs differ by at most 2e-5 and a difference of two outputs by 4e-5 * max|raw|.
    raw_all = sweep.ligand_atom_masking(hits, sigmoid=False)
    name, feats, pose = hits[1]
    raw_rows = sweep.atom_masking_raw[name].clone()
    alone = sweep.ligand_atom_masking([(name, feats, pose)], sigmoid=False)
    gap = float((alone[name] - raw_all[name]).abs().max())
    bound = 4e-5 * float(raw_rows.abs().max())
    print(f'{name}: alone against in the library {gap:.3e} bound {bound:.3e}')
    assert gap <= bound
    assert torch.equal(raw_all[name], raw_rows[0, 0] - raw_rows[1:, 0])
    # with the sigmoid (the default for this classification model): s(whole) - s(without a)
    assert torch.allclose(scores[name], torch.sigmoid(raw_rows[0, 0]) - torch.sigmoid(raw_rows[1:, 0]), rtol=0, atol=1e-6)
    assert sweep.ligand_atom_masking([]) == {} and sweep.atom_masking_raw == {}


def test_errors():
    from pointvs_amd.screening import MAX_SCREEN_LIGAND_ATOMS, ScreeningSweep
    lig, rec, lig_feats, rec_feats = _set(8103, 20)
    model = _single_head(6)
    sweep = ScreeningSweep(model, rec.cuda(), rec_feats, edge_radius=6.0, batch_size=4, capture=False)
    item = ('twice', lig_feats[:5], lig[:5])
    with pytest.raises(ValueError, match='unique'):
        sweep.ligand_atom_masking([item, ('other', lig_feats[:3], lig[:3]), item])
    n = MAX_SCREEN_LIGAND_ATOMS + 1
    with pytest.raises(ValueError, match="'huge' has 1025 atoms"):
        sweep.ligand_atom_masking([('huge', lig_feats[:1].expand(n, -1), torch.zeros(n, 3))])
    with pytest.raises(ValueError, match='column 1 of 1'):
        sweep.ligand_atom_masking([item], column=1)
    with pytest.raises(NotImplementedError, match='fp32 only'):
        ScreeningSweep(_single_head(6).double(), rec.cuda().double(), rec_feats.double(), edge_radius=6.0,
                       batch_size=4).ligand_atom_masking([item])
    # a table the packer refuses, through the screen: an empty batch and a ValueError from check_leave_out()
    screen = sweep.masking
    screen.load_leave_out(lig[:5].cuda(), lig_feats[:5].cuda(), torch.tensor([0, 5, 3], dtype=torch.int32).cuda(),
                          [0] * 4, torch.zeros(1, dtype=torch.int32).cuda())
    assert not screen.lig_ptr.any()
    with pytest.raises(ValueError, match='not a table'):
        screen.check_leave_out()
    with pytest.raises(ValueError, match='a batch holds up to 4 slots'):
        screen.load_leave_out(lig[:5].cuda(), lig_feats[:5].cuda(), torch.tensor([0, 5], dtype=torch.int32).cuda(),
                              [5, 4, 4, 4, 4], torch.zeros(1, dtype=torch.int32).cuda())
    assert list(sweep.ligand_atom_masking([item])) == ['twice']              # (the sweep is still usable)
