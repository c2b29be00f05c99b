"""ScreeningSweep.receptor_hotspots with attribution='atom_masking', use_rank and top, end to end: a receptor of 100
atoms, 5 hits of 3..20 atoms at batch_size 2 (three steps, the last partial), a 2-layer, 32-channel model with edge
attention. The masking map against the sweep's own receptor_atom_masking / ligand_atom_masking (bit for bit) and the
numpy reduction; the ranks of all three attributions against the numpy ranks (tests/_hit_rank_ref.py) of the values
the same call returns, exactly; the defaults; a cropped sweep (crop 7, edge radius 6) against
pointvs_amd.attribution.atom_masking on each hit's cropped complex within 4e-5 * max|raw|, the bound of
tests/test_gpu_crop_copies.py; the errors. The poses are chosen so that no atom pair lies within 1e-4 of either radius
(asserted from the fp64 distances), so which atoms are listed is decided the same way everywhere."""
import tempfile

import numpy as np
import pytest
import torch

from tests import _contact_ref as cref
from tests import _crop_copies_ref as crop_ref
from tests import _hit_rank_ref as ref
from tests._golden import needs_caching_allocator

pytestmark = [pytest.mark.gpu, needs_caching_allocator]

N_REC, R_EDGE, CROP, B, SEED = 100, 6.0, 7.0, 2, 7303
SIZES = (3, 7, 12, 20, 5)
KW = dict(dim_input=12, k=32, dim_output=1, num_layers=2, residual=False, edge_residual=False,
          edge_attention=True, normalize=False, tanh=False, dropout=0.0, graphnorm=False, update_coords=True,
          permutation_invariance=False, node_attention=False, gated_residual=False, rezero=False,
          softmax_attention=False, model_task='classification')
ATTRIBUTIONS = ('edge_attention', 'cam', 'atom_masking')
_MADE = {}


def fixture():
    """(items, rec [100, 3], rec_feats, the model on the device); made once."""
    if not _MADE:
        from pointvs_amd.egnn_satorras import SartorrasEGNN
        from pointvs_amd.synthetic import random_poses, screening_set
        lig, rec, feats = screening_set(seed=SEED, n_nodes=max(SIZES) + 400, n_lig=max(SIZES))
        near = torch.argsort((rec - lig.mean(0)).norm(dim=1))[:N_REC].sort().values
        rec, lig_feats, rec_feats = rec[near].contiguous(), feats[:max(SIZES)], feats[max(SIZES):][near].contiguous()
        items = [(f'hit{k}', lig_feats[:n].roll(k, 0).contiguous(),
                  random_poses(lig[:n], 1, seed=SEED + k, max_shift=3.0)[0].contiguous()) for k, n in enumerate(SIZES)]
        for radius in (R_EDGE, CROP):
            assert cref.radius_gap(items, rec, radius) > 1e-4, radius
        torch.manual_seed(11)
        model = SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **KW).eval()
        _MADE.update(items=items, rec=rec, rec_feats=rec_feats, model=model.cuda())
    return _MADE['items'], _MADE['rec'], _MADE['rec_feats'], _MADE['model']


def _sweep(**kw):
    from pointvs_amd.screening import ScreeningSweep
    items, rec, rec_feats, model = fixture()
    return ScreeningSweep(model, rec.cuda(), rec_feats, edge_radius=R_EDGE, batch_size=B, **kw)


def _np(t):
    return t.cpu().numpy()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _reduced(per_hit):
    """(mean, count, max) of rows [hits, n_rec] in hit order."""
    rec_sum, count, top = ref.accumulate(per_hit, *ref.fresh_accumulators(per_hit.shape[1]))
    with np.errstate(invalid='ignore', divide='ignore'):
        return rec_sum / count, count, top


def _check_value_keys(out, what):
    mean, count, top = _reduced(_np(out['per_hit']))
    assert np.array_equal(_np(out['mean']), mean, equal_nan=True) and _np(out['mean']).dtype == np.float64, what
    assert _same(_np(out['count']), count) and _same(_np(out['max']), top), what


# ---------------------------------------------------------------- attribution='atom_masking'

@pytest.mark.parametrize('atoms', ['contacts', 'all'])
def test_masking_map_is_the_sweeps_own_masking_reduced_over_the_hits(atoms, tmp_path):
    items = fixture()[0]
    names = [name for name, _, _ in items]
    sweep = _sweep()
    out = sweep.receptor_hotspots(items, attribution='atom_masking', atoms=atoms, per_hit=True,
                                  scores_file=tmp_path / 'map.txt', ligand_scores_file=tmp_path / 'ligand.txt')
    assert set(out) == {'mean', 'count', 'max', 'ligand', 'per_hit'} and list(out['ligand']) == names
    assert out['per_hit'].shape == (len(items), N_REC) and out['per_hit'].dtype == torch.float32
    raw_rec, raw_lig = dict(sweep.receptor_atom_masking_raw), dict(sweep.atom_masking_raw)
    assert list(raw_rec) == names and list(raw_lig) == names                     # (left filled by the call)
    by_hit = sweep.receptor_atom_masking(items, atoms=atoms)
    ligand = sweep.ligand_atom_masking(items)
    per_hit = _np(out['per_hit'])
    for h, (name, _, pose) in enumerate(items):
        which, scores = by_hit[name]
        want = np.full(N_REC, np.nan, dtype=np.float32)
        want[_np(which)] = _np(scores)
        assert _same(per_hit[h], want), name
        assert which.numel() == (N_REC if atoms == 'all' else int((~np.isnan(per_hit[h])).sum()))
        assert _same(_np(out['ligand'][name]), _np(ligand[name])) and out['ligand'][name].shape == (pose.shape[0],)
        assert torch.equal(raw_rec[name], sweep.receptor_atom_masking_raw[name])
    listed = (~np.isnan(per_hit)).sum(0)
    assert (listed == len(items)).all() if atoms == 'all' else (0 < listed.max() and listed.min() < len(items))
    _check_value_keys(out, atoms)
    assert np.array_equal(_np(out['count']), listed)
    mean, count = _np(out['mean']), _np(out['count'])
    lines = (tmp_path / 'map.txt').read_text().splitlines()
    assert lines == [f'{mean[j]:.6f} {count[j]} | receptor atom{j}' for j in range(N_REC) if count[j] > 0]
    lines = (tmp_path / 'ligand.txt').read_text().splitlines()
    assert lines == [f'{v:.6f} | receptor {name}_atom{a}' for name in names
                     for a, v in enumerate(out['ligand'][name].tolist())]
    assert float(np.nanmax(np.abs(per_hit))) > 0


# ---------------------------------------------------------------- use_rank, order, top

def _want_ranks(out, items, with_ligand):
    """(per_hit_rank, {name: ligand ranks}) by numpy from the values `out` holds."""
    per_hit = _np(out['per_hit'])
    rows, lig = np.full_like(per_hit, np.nan), {}
    for h, (name, _, _) in enumerate(items):
        values = _np(out['ligand'][name]) if with_ligand else np.zeros(0, dtype=np.float32)
        got = ref.ranks_of(np.concatenate([values, per_hit[h]]))
        lig[name], rows[h] = got[:len(values)], got[len(values):]
    return rows, lig


def _want_order(key, count):
    atoms = np.flatnonzero(count > 0)
    return atoms[np.lexsort((atoms, key[atoms]))]


@pytest.mark.parametrize('attribution', ATTRIBUTIONS)
def test_ranks_order_and_top(attribution, tmp_path):
    items = fixture()[0]
    sweep = _sweep()
    plain = sweep.receptor_hotspots(items, attribution=attribution, per_hit=True, top=3)
    out = sweep.receptor_hotspots(items, attribution=attribution, per_hit=True, use_rank=True,
                                  scores_file=tmp_path / 'ranks.txt')
    with_ligand = attribution != 'edge_attention'
    extra = {'rank_mean', 'per_hit_rank', 'order'} | ({'ligand_rank'} if with_ligand else set())
    assert set(plain) == {'mean', 'count', 'max', 'ligand', 'per_hit', 'order'} and set(out) == set(plain) | extra
    # the value keys: the bits of the call without use_rank
    for key in ('mean', 'count', 'max', 'per_hit'):
        assert _same(_np(out[key]), _np(plain[key])), key
    for name in plain['ligand']:
        assert _same(_np(out['ligand'][name]), _np(plain['ligand'][name])), name
    _check_value_keys(out, attribution)
    # the ranks of the returned values, exactly
    rows, lig = _want_ranks(out, items, with_ligand)
    got = _np(out['per_hit_rank'])
    assert got.dtype == np.float32 and np.array_equal(got, rows, equal_nan=True)
    assert np.array_equal(np.isnan(got), np.isnan(_np(out['per_hit'])))
    if with_ligand:
        assert list(out['ligand_rank']) == [name for name, _, _ in items]
        for name in lig:
            assert np.array_equal(_np(out['ligand_rank'][name]), lig[name], equal_nan=True), name
        assert max(float(np.nanmax(v)) for v in lig.values() if len(v)) > 0
    rank_mean, count, _ = _reduced(rows)
    assert np.array_equal(_np(out['rank_mean']), rank_mean, equal_nan=True) and np.array_equal(count, _np(out['count']))
    assert int(count.max()) >= 2 and len(set(rank_mean[count > 0].tolist())) > 3
    # order: by rank_mean ascending under use_rank, else by mean descending; ties to the lower atom; top cuts
    order = _want_order(rank_mean, count)
    assert out['order'].dtype == torch.int64 and np.array_equal(_np(out['order']), order) and len(order) == (count > 0).sum()
    assert np.array_equal(_np(plain['order']), _want_order(-_np(plain['mean']), count)[:3]) and len(plain['order']) == 3
    lines = (tmp_path / 'ranks.txt').read_text().splitlines()
    assert lines == [f'{rank_mean[j]:.6f} {count[j]} | receptor atom{j}' for j in range(N_REC) if count[j] > 0]
    if attribution == 'edge_attention':
        cut = sweep.receptor_hotspots(items, use_rank=True, top=3)
        assert np.array_equal(_np(cut['order']), order[:3]) and 'per_hit_rank' not in cut and 'ligand_rank' not in cut
        assert len(sweep.receptor_hotspots(items, top=0)['order']) == 0
        none = sweep.receptor_hotspots([], use_rank=True, per_hit=True)
        assert none['per_hit_rank'].shape == (0, N_REC) and len(none['order']) == 0
        assert bool(torch.isnan(none['rank_mean']).all())


# ---------------------------------------------------------------- the defaults

@pytest.mark.parametrize('attribution', ['edge_attention', 'cam'])
def test_a_default_call_has_todays_keys_and_bits(attribution):
    items = fixture()[0]
    first = _sweep().receptor_hotspots(items, attribution=attribution)
    assert set(first) == {'mean', 'count', 'max', 'ligand'}
    second = _sweep().receptor_hotspots(items, attribution=attribution, per_hit=True)
    assert set(second) == {'mean', 'count', 'max', 'ligand', 'per_hit'}
    for key in ('mean', 'count', 'max'):
        assert _same(_np(first[key]), _np(second[key])), key
    for name in first['ligand']:
        assert _same(_np(first['ligand'][name]), _np(second['ligand'][name]))
    assert int(first['count'].max()) >= 2


# ---------------------------------------------------------------- cropped sweeps

def _kept(items, rec):
    """Per hit the receptor atoms PF.crop_keep keeps, from its masks."""
    from pointvs_amd import functional as PF
    pos = torch.cat([pose for _, _, pose in items], 0).cuda().contiguous()
    ptr = torch.tensor([0] + [int(pose.shape[0]) for _, _, pose in items]).cumsum(0).to(device='cuda', dtype=torch.int32)
    keep = PF.crop_keep(pos, ptr, rec.cuda().float().contiguous(), CROP)[0].cpu().numpy().view(np.uint64)
    return [[j for j in range(N_REC) if (int(words[j // 64]) >> (j % 64)) & 1] for words in keep]


def _one_at_a_time(model, item, rec, rec_feats):
    """pointvs_amd.attribution.atom_masking over the hit's cropped complex: scores [n + kept], the kept atoms."""
    from pointvs_amd import attribution
    from pointvs_amd.radius_graph import generate_edges
    _, feats, pose = item
    x, pos, kept = crop_ref.copy_complex(feats.numpy(), pose.numpy(), rec_feats.numpy(), rec.numpy(), CROP)
    x, pos = torch.from_numpy(x).cuda(), torch.from_numpy(pos).cuda()
    _, ei, attrs = generate_edges(pos, x[:, -1].contiguous(), R_EDGE, R_EDGE, prune=False)
    scores = attribution.atom_masking(model, pos[None], x[None], edge_indices=ei,
                                      edge_attrs=torch.nn.functional.one_hot(attrs, 3))
    return scores, kept


def test_cropped_masking_map_lists_the_kept_atoms_and_matches_one_hit_at_a_time():
    items, rec, rec_feats, model = fixture()
    with pytest.raises(NotImplementedError):
        _sweep(crop_radius=CROP).receptor_hotspots(items, attribution='atom_masking')
    with pytest.raises(NotImplementedError):            # (the maps' keyword does not opt the masking in)
        _sweep(crop_radius=CROP, cropped_hotspots=True).receptor_hotspots(items, attribution='atom_masking')
    sweep = _sweep(crop_radius=CROP, cropped_attribution=True)
    out = sweep.receptor_hotspots(items, attribution='atom_masking', atoms='all', sigmoid=False, per_hit=True)
    per_hit, kept = _np(out['per_hit']), _kept(items, rec)
    assert 0 < min(map(len, kept)) and max(map(len, kept)) < N_REC
    for h, item in enumerate(items):
        name, n = item[0], int(item[2].shape[0])
        assert np.flatnonzero(~np.isnan(per_hit[h])).tolist() == kept[h], name
        want, kept_ref = _one_at_a_time(model, item, rec, rec_feats)
        assert kept_ref.tolist() == kept[h]
        for what, got, w, raw in (('receptor', per_hit[h][kept[h]], want[n:], sweep.receptor_atom_masking_raw[name]),
                                  ('ligand', _np(out['ligand'][name]), want[:n], sweep.atom_masking_raw[name])):
            gap, bound = float(np.abs(got.astype(np.float64) - w).max()), 4e-5 * float(raw.abs().max())
            print(f'{name} {what}: against attribution.atom_masking on the cropped complex {gap:.3e} bound {bound:.3e}')
            assert gap <= bound, (name, what)
    _check_value_keys(out, 'cropped')
    assert np.array_equal(_np(out['count']), np.bincount(np.concatenate(kept), minlength=N_REC))


def test_ranks_on_a_cropped_hotspot_sweep_skip_the_dropped_atoms():
    items, rec, _, _ = fixture()
    out = _sweep(crop_radius=CROP, cropped_hotspots=True).receptor_hotspots(items, per_hit=True, use_rank=True)
    kept = _kept(items, rec)
    ranks, values = _np(out['per_hit_rank']), _np(out['per_hit'])
    dropped = np.ones_like(ranks, dtype=bool)
    for h, atoms in enumerate(kept):
        dropped[h, atoms] = False
    assert dropped.any() and np.isnan(ranks[dropped]).all() and np.isnan(values[dropped]).all()
    assert np.array_equal(ranks, _want_ranks(out, items, False)[0], equal_nan=True)
    rank_mean, count, _ = _reduced(ranks)
    assert np.array_equal(count, _np(out['count'])) and (count <= (~dropped).sum(0)).all() and count.max() >= 2
    assert np.array_equal(_np(out['rank_mean']), rank_mean, equal_nan=True)


# ---------------------------------------------------------------- errors

def test_errors():
    items = fixture()[0]
    sweep = _sweep(capture=False)
    with pytest.raises(ValueError, match="attribution='atom_masking'"):
        sweep.receptor_hotspots(items, attribution='cam', atoms='all')
    with pytest.raises(ValueError, match="attribution='atom_masking'"):
        sweep.receptor_hotspots(items, attribution='cam', sigmoid=False)
    with pytest.raises(ValueError, match="attribution='atom_masking'"):
        sweep.receptor_hotspots(items, atoms=torch.tensor([1, 2]))
    with pytest.raises(ValueError, match='more than once'):
        sweep.receptor_hotspots(items, attribution='atom_masking', atoms=torch.tensor([4, 9, 4]))
    with pytest.raises(ValueError, match='top=-1'):
        sweep.receptor_hotspots(items, top=-1)
    with pytest.raises(ValueError, match="'edge_attention', 'cam' or 'atom_masking'"):
        sweep.receptor_hotspots(items, attribution='nonsense')
    assert sweep.batches_run == 0                                                  # (all refused before any step)
    picked = sweep.receptor_hotspots(items[:2], attribution='atom_masking', atoms=torch.tensor([9, 4]), per_hit=True)
    assert np.flatnonzero(~np.isnan(_np(picked['per_hit'][0]))).tolist() == [4, 9]
    assert _np(picked['count']).tolist() == [2 if j in (4, 9) else 0 for j in range(N_REC)]
