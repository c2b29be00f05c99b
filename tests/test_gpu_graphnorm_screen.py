"""GraphNorm models through the captured fixed-shape library step: LibraryScreen / ScreeningSweep with
padded_graphnorm=True run at the padded shape N_cap with GraphNorm's statistics over the node_ptr[batch_size] real rows
(PvsGraph.n_norm_rows_dev). Replays of ONE captured step on batches of other compositions against the same screen's
eager call (bit for bit) and against the fp64 oracle on the batch's real nodes as one batch (the reference's semantics:
statistics over all nodes of the batch; bound: 1e-5 of the largest output, the bound of the screening paths in
tests/test_gpu_library_screen.py); the unchanged default; the struck screen; the sweep and ligand-atom masking.
"""
import functools

import numpy as np
import pytest
import torch

from tests._golden import needs_caching_allocator
from tests.test_gpu_library_screen import KW, _model, _oracle_items, _set, _slots

pytestmark = pytest.mark.gpu

N_REC, B, MAX_LIG, RADIUS = 50, 3, 20, 7.0
MODELS = {'k32': dict(graphnorm=True, num_layers=2), 'k64': dict(k=64, normalize=True, graphnorm=True, num_layers=3)}
# (captured on the first; then: the largest ligands, mixed sizes, an empty last slot, one atom more than the first)
COMPOSITIONS = [(7, 20, 3), (20, 20, 20), (5, 17, 12), (12, 9, 0), (7, 20, 4)]
REL = 1e-5


@functools.lru_cache(maxsize=None)
def _receptor():
    """(ligand [64, 3], receptor [50, 3], ligand features, receptor features): the 50 receptor atoms nearest the ligand."""
    lig, rec, lig_feats, rec_feats = _set(6011)
    near = torch.argsort((rec - lig.mean(0)).norm(dim=1))[:N_REC].sort().values
    return lig, rec[near].contiguous(), lig_feats, rec_feats[near].contiguous()


@functools.lru_cache(maxsize=None)
def _gn_model(name):
    return _model(3, **MODELS[name]).cuda()


@functools.lru_cache(maxsize=None)
def _batches():
    lig, _, lig_feats, _ = _receptor()
    return [_slots(lig, lig_feats, sizes, seed=300 + 10 * k, special=False) for k, sizes in enumerate(COMPOSITIONS)]


def _oracle(name, items):
    """fp64 oracle outputs [len(items)] of the complexes `items` as ONE batch."""
    from oracle import egnn_oracle as orc
    from pointvs_amd.graph import Batch
    model = _gn_model(name)
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items() if v.is_floating_point()}
    b = Batch.from_data_list(items)
    with torch.no_grad():
        return orc.model_forward(sd, dict(KW, **MODELS[name]), b.x, b.pos, b.edge_index, b.edge_attr.double(), b.batch,
                                 n_graphs=len(items)).reshape(-1)


def _items(slots, rec_drop=None):
    _, rec, _, rec_feats = _receptor()
    items = []
    for k, slot in enumerate(slots):
        keep = torch.ones(N_REC, dtype=torch.bool)
        if rec_drop is not None and rec_drop[k] >= 0:
            keep[rec_drop[k]] = False
        items += _oracle_items([slot], rec[keep], rec_feats[keep], RADIUS, RADIUS)
    return items


def _assert_within(got, want, what):
    err = float((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-30))
    print(f'{what}: max|got-oracle|/max|oracle| = {err:.3e}')
    assert err < REL, (what, err)


def _screen(name, **kw):
    from pointvs_amd.screening import LibraryScreen
    _, rec, _, rec_feats = _receptor()
    return LibraryScreen(_gn_model(name), rec.cuda(), rec_feats, B, MAX_LIG, RADIUS, **kw)


@needs_caching_allocator
@pytest.mark.parametrize('name', list(MODELS))
def test_one_captured_step_serves_every_composition(name):
    batches = _batches()
    eager = _screen(name, padded_graphnorm=True)
    assert eager.reuse and eager.graphnorm and eager._gn_padded
    want = [eager(slots).reshape(-1).clone() for slots in batches]      # (first batch first: the same probe)
    eager.check()
    assert set(eager._fast['pgs']) == {eager.n_cap}                     # one graph pair, at the padded shape
    graph = _screen(name, padded_graphnorm=True).capture(batches[0])
    assert graph._captured
    for k in (1, 2, 3, 4, 0):
        got = graph.replay(batches[k]).reshape(-1).clone()
        n_real = sum(COMPOSITIONS[k]) + B * N_REC
        assert int(graph._fast['node_ptr'][B]) == n_real <= graph.n_cap
        assert torch.equal(got, want[k]), (k, got, want[k])
        _assert_within(got, _oracle(name, _items(batches[k])), f'{name} replay of composition {COMPOSITIONS[k]}')
    graph.check()


def test_the_default_is_unchanged():
    batches = _batches()
    with pytest.raises(RuntimeError, match='graphnorm'):
        _screen('k32').capture(batches[0])
    with pytest.raises(RuntimeError, match='graphnorm'):
        _screen('k32', padded_graphnorm=False).capture(batches[0])
    # the eager exact-count route and the padded one are the same numbers (not the same bits: another row split)
    exact, padded = _screen('k32'), _screen('k32', padded_graphnorm=True)
    assert not exact._gn_padded
    a, b = exact(batches[2]).reshape(-1), padded(batches[2]).reshape(-1)
    assert set(exact._fast['pgs']) == {sum(COMPOSITIONS[2]) + B * N_REC}
    assert float((a - b).abs().max()) <= REL * float(a.abs().max())
    # a model without GraphNorm: the keyword changes nothing, bit for bit
    from pointvs_amd.screening import LibraryScreen
    _, rec, _, rec_feats = _receptor()
    plain = _model(3, num_layers=2).cuda()
    with_kw = LibraryScreen(plain, rec.cuda(), rec_feats, B, MAX_LIG, RADIUS, padded_graphnorm=True)
    without = LibraryScreen(plain, rec.cuda(), rec_feats, B, MAX_LIG, RADIUS)
    assert not with_kw._gn_padded
    for slots in batches[:3]:
        assert torch.equal(with_kw(slots), without(slots))
    assert not with_kw._fast['pgs'][with_kw.n_cap][0].c.n_norm_rows_dev


@needs_caching_allocator
def test_struck_screen_counts_its_rows_on_the_device():
    batches = _batches()
    screen = _screen('k32', struck=True, padded_graphnorm=True)
    rec_drop = [-1, 17, -1]
    screen.load(batches[2], rec_drop=rec_drop)
    got = screen().reshape(-1).clone()
    screen.check()
    n_atoms, n_struck = sum(COMPOSITIONS[2]), 1
    assert int(screen._fast['node_ptr'][B]) == n_atoms + B * N_REC - n_struck
    want = _oracle('k32', _items(batches[2], rec_drop))
    _assert_within(got, want, 'struck slot 1 without receptor atom 17')
    # captured, the same bits; and without a struck slot the count is the whole batch's
    screen.capture()
    screen.load(batches[2], rec_drop=rec_drop)
    assert torch.equal(screen.replay().reshape(-1), got)
    screen.load(batches[1], rec_drop=[-1, -1, -1])
    out = screen.replay().reshape(-1).clone()
    assert int(screen._fast['node_ptr'][B]) == sum(COMPOSITIONS[1]) + B * N_REC
    _assert_within(out, _oracle('k32', _items(batches[1])), 'struck screen, no slot struck')


@needs_caching_allocator
def test_sweep_captures_the_library_step_and_the_masking_step():
    from pointvs_amd.screening import ScreeningSweep
    lig, rec, lig_feats, rec_feats = _receptor()
    sizes = (12, 20, 3, 9, 17, 5)
    slots = _slots(lig, lig_feats, sizes, seed=500, special=False)
    library = [(f'lig{k}', feats, pose.unsqueeze(0).cuda()) for k, (feats, pose) in enumerate(slots)]
    model = _gn_model('k32')
    sweep = ScreeningSweep(model, rec.cuda(), rec_feats, RADIUS, batch_size=B, capture=True, padded_graphnorm=True)
    got = sweep.run_library(library, sigmoid=False, max_lig_atoms=MAX_LIG)
    assert sweep.library._captured and sweep.library._gn_padded
    assert sweep.batches_run == 2                                     # ceil(6 poses / 3)
    for first in (0, 3):                                               # the plan: library order, three poses a batch
        want = _oracle('k32', _items(slots[first:first + B]))
        mine = torch.cat([got[f'lig{k}'].reshape(-1) for k in range(first, first + B)])
        _assert_within(mine, want, f'run_library batch of ligands {first}..{first + B - 1}')
    hits = [(name, feats, poses[0]) for name, feats, poses in (library[0], library[3])]
    sweep.ligand_atom_masking(hits, sigmoid=False)
    assert sweep.masking._captured and sweep.masking._gn_padded
    off = ScreeningSweep(model, rec.cuda(), rec_feats, RADIUS, batch_size=B, capture=True)
    off.ligand_atom_masking(hits, sigmoid=False)
    assert not off.masking._captured
    for name, _, _ in hits:
        a, b = sweep.atom_masking_raw[name].double().cpu(), off.atom_masking_raw[name].double().cpu()
        assert a.shape == b.shape and a.shape[0] == dict(lig0=13, lig3=10)[name]
        assert float((a - b).abs().max()) <= REL * float(b.abs().max()), name
    # the default sweep still runs a graphnorm model eager
    assert not off.padded_graphnorm
    off.run_library(library[:3], sigmoid=False, max_lig_atoms=MAX_LIG)
    assert not off.library._captured
