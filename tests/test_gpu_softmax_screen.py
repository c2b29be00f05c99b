"""Softmax-attention models through the first-layer reuse (`softmax_reuse=True` of ReceptorScreen, LibraryScreen and
ScreeningSweep): the receptor side of the first layer kept as softmax statistics (pvs_egnn_layer_edge_stats_softmax),
merged per row with the ligand-touching edges' (pvs_egnn_layer_fwd_partial_softmax); the layers behind the first run the
softmax forward over a CSR whose edge count lives on the device and whose trailing rows are padding. Shapes, slots and
bounds are those of tests/test_gpu_library_screen.py, tests/test_gpu_contact_masking.py and
tests/test_gpu_contact_attention.py for the sigmoid-attention models."""
import numpy as np
import pytest
import torch

from tests._golden import needs_caching_allocator
from tests.test_gpu_contact_attention import KW as ORACLE_KW, _close, _oracle_pair
from tests.test_gpu_contact_masking import _bond_scores_one_at_a_time
from tests.test_gpu_library_screen import N_REC, SIZES, _change_first_layer, _model, _oracle_items, _set, _slots

pytestmark = pytest.mark.gpu

SOFT = dict(edge_attention=True, softmax_attention=True)
RICH = dict(SOFT, node_attention=True, tanh=True, residual=True)
MODELS = {
    'soft-k32': (dict(SOFT), {}),
    'soft-k64': (dict(SOFT, k=64), {}),
    'rich-k32': (dict(RICH), {}),
    'rich-k64': (dict(RICH, k=64), {}),
    'graphnorm-k32': (dict(SOFT, graphnorm=True, residual=True), dict(padded_graphnorm=True)),
}
RADIUS = 7.0


def _soft_model(seed, name):
    flags, screen_kw = MODELS[name]
    return _model(seed, num_layers=3, **flags), dict(screen_kw, softmax_reuse=True)


def _rel(fast, slow):
    return float((fast - slow).abs().max() / slow.abs().max().clamp_min(1e-30))


@pytest.mark.parametrize('name', list(MODELS))
def test_library_screen_matches_the_plain_forward(name):
    """Two consecutive mixed batches (a coincident atom, a far ligand, an empty slot) == model(Batch) of the same
    complexes built from the oracle's edge lists: max|fast - slow| / max|slow| < 1e-5."""
    from pointvs_amd.graph import Batch
    from pointvs_amd.screening import LibraryScreen
    lig, rec, lig_feats, rec_feats = _set(6003)
    model, kw = _soft_model(1, name)
    screen = LibraryScreen(model, rec.cuda(), rec_feats, len(SIZES), 64, RADIUS, **kw)
    assert screen.reuse is True and screen.rec_magg.shape == (N_REC, model.layers[1].hidden_nf + 4)
    for k, sizes in enumerate((SIZES, (20, 0, 64, 33, 1, 7))):
        slots = _slots(lig, lig_feats, sizes, seed=40 + 10 * k, rec=rec)
        fast = screen(slots).reshape(-1)
        with torch.no_grad():
            slow = model(Batch.from_data_list(_oracle_items(slots, rec, rec_feats, RADIUS, RADIUS)).to('cuda')).reshape(-1)
        err = _rel(fast, slow)
        print(f'{name} batch {k}: max|fast-slow|/max|slow| = {err:.3e}; scores {fast.cpu().numpy().round(5).tolist()}')
        assert err < 1e-5, err
        assert float(slow.std()) > 1e-3 * float(slow.abs().max()), 'the slots score alike: the case tells nothing apart'
    screen.check()


@pytest.mark.parametrize('name', ['soft-k32', 'rich-k64'])
def test_receptor_screen_matches_the_plain_forward(name):
    from pointvs_amd.graph import Batch
    from pointvs_amd.screening import ReceptorScreen
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(6002, n_lig=17)
    model, kw = _soft_model(4, name)
    poses = random_poses(lig, 3, seed=9, max_shift=4.0)
    screen = ReceptorScreen(model, rec.cuda(), torch.cat([lig_feats, rec_feats], 0), 17, 3, RADIUS, **kw)
    assert screen.reuse is True and screen.fast_graph
    fast = screen(poses.cuda()).reshape(-1)
    with torch.no_grad():
        items = _oracle_items([(lig_feats, pose) for pose in poses], rec, rec_feats, RADIUS, RADIUS)
        slow = model(Batch.from_data_list(items).to('cuda')).reshape(-1)
    err = _rel(fast, slow)
    print(f'{name} receptor screen: {err:.3e}')
    assert err < 1e-5, err
    screen.check()


@needs_caching_allocator
@pytest.mark.parametrize('name', ['rich-k32', 'graphnorm-k32'])
def test_captured_step_replays_across_compositions(name):
    """ONE captured step, replayed on batches of other compositions == the eager screen on the same batch, bit for bit."""
    from pointvs_amd.screening import LibraryScreen
    lig, rec, lig_feats, rec_feats = _set(6004)
    model, kw = _soft_model(2, name)
    comps = [(7, 20, 3), (5, 17, 1), (12, 9), (20, 20, 20)]           # B = 3, L_cap = 60
    batches = [_slots(lig, lig_feats, sizes, seed=70 + 10 * k, special=False) for k, sizes in enumerate(comps)]
    eager = LibraryScreen(model, rec.cuda(), rec_feats, 3, 20, RADIUS, **kw)
    want = [eager(slots).reshape(-1).clone() for slots in batches]   # (first batch first: the same probe)
    eager.check()
    graph = LibraryScreen(model, rec.cuda(), rec_feats, 3, 20, RADIUS, **kw).capture(batches[0])
    for k in (2, 3, 1, 0):
        got = graph.replay(batches[k]).reshape(-1).clone()
        assert torch.equal(got, want[k]), k
    graph.check()


@needs_caching_allocator
def test_captured_receptor_screen_replays():
    from pointvs_amd.screening import ReceptorScreen
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(6002, n_lig=17)
    model, kw = _soft_model(4, 'rich-k32')
    feats = torch.cat([lig_feats, rec_feats], 0)
    poses = random_poses(lig, 9, seed=9, max_shift=4.0).cuda()
    eager = ReceptorScreen(model, rec.cuda(), feats, 17, 3, RADIUS, **kw)
    want = [eager(poses[k:k + 3].contiguous()).reshape(-1).clone() for k in (0, 3, 6)]
    graph = ReceptorScreen(model, rec.cuda(), feats, 17, 3, RADIUS, **kw).capture(poses[:3].contiguous())
    for i in (2, 0, 1):
        assert torch.equal(graph.replay(poses[3 * i:3 * i + 3]).reshape(-1), want[i]), i
    graph.check()


def _hits(lig, lig_feats):
    from pointvs_amd.synthetic import random_poses
    return [(f'lig{n}', lig_feats[:n].roll(k, 0).contiguous(),
             random_poses(lig[:n], 1, seed=300 + k, max_shift=3.0)[0].contiguous()) for k, n in enumerate((5, 17))]


@needs_caching_allocator
def test_sweep_masking_of_hits_equals_masking_one_complex_at_a_time():
    """contact_masking and ligand_atom_masking of a sweep with softmax_reuse=True on two hits == attribution.bond_masking
    / atom_masking per hit, within the bound tests/test_gpu_contact_masking.py holds the sigmoid model to
    (4e-5 of the largest raw output)."""
    from pointvs_amd import attribution
    from pointvs_amd.radius_graph import generate_edges
    from pointvs_amd.screening import ScreeningSweep
    lig, rec, lig_feats, rec_feats = _set(8301, 20)
    items = _hits(lig, lig_feats)
    model, kw = _soft_model(12, 'rich-k32')
    model = model.cuda()
    sweep = ScreeningSweep(model, rec.cuda(), rec_feats, 4.0, batch_size=4, **kw)
    contacts = sweep.contact_masking(items, sigmoid=False, column=0)
    assert sweep.struck.reuse and sweep.struck._captured and sweep.struck.struck
    atoms = sweep.ligand_atom_masking(items, sigmoid=False)
    assert sweep.masking.reuse and sweep.masking._captured
    for name, feats, pose in items:
        pairs, scores = contacts[name]
        raw = sweep.contact_masking_raw[name]
        assert pairs.shape[0] > 0 and torch.equal(scores, raw[0, 0] - raw[1:, 0])
        ref = _bond_scores_one_at_a_time(model, rec, rec_feats, feats, pose, pairs.cpu().tolist(), 4.0)
        gap, bound = float(np.abs(scores.double().cpu().numpy() - ref).max()), 4e-5 * float(raw.abs().max())
        print(f'{name}: contact masking against bond_masking {gap:.3e} bound {bound:.3e} largest {np.abs(ref).max():.3e}')
        assert gap <= bound and float(scores.abs().max()) > 0
        pos = torch.cat([pose, rec], 0).cuda()
        x = torch.cat([feats, rec_feats], 0).cuda()
        _, ei, attrs = generate_edges(pos, x[:, -1].contiguous(), 4.0, 4.0, prune=False)
        ref = attribution.atom_masking(model, pos[None], x[None], edge_indices=ei,
                                       edge_attrs=torch.nn.functional.one_hot(attrs, 3))[:pose.shape[0]]
        raw = sweep.atom_masking_raw[name]
        gap, bound = float(np.abs(atoms[name].double().cpu().numpy() - ref).max()), 4e-5 * float(raw.abs().max())
        print(f'{name}: atom masking against atom_masking {gap:.3e} bound {bound:.3e} largest {np.abs(ref).max():.3e}')
        assert gap <= bound and float(atoms[name].abs().max()) > 0


def _attention_map(model, items, rec, rec_feats, radius, gnn_layer):
    """attribution.edge_attention of every hit, one complex at a time, reduced on the host: per atom the largest value
    over its class-1 edges (NaN without one) -> (ligand {name: [n]}, per_hit [hits, n_rec])."""
    from pointvs_amd import attribution
    from pointvs_amd.radius_graph import generate_edges
    ligand, per_hit = {}, []
    for name, feats, pose in items:
        n = int(pose.shape[0])
        pos = torch.cat([pose, rec], 0).cuda()
        x = torch.cat([feats, rec_feats], 0).cuda()
        _, ei, attrs = generate_edges(pos, x[:, -1].contiguous(), radius, radius, prune=False)
        att = attribution.edge_attention(model, pos[None], x[None], edge_indices=ei,
                                         edge_attrs=torch.nn.functional.one_hot(attrs, 3), gnn_layer=gnn_layer)
        att = np.asarray(att.detach().cpu() if torch.is_tensor(att) else att, dtype=np.float64).reshape(-1)
        rows, cls = ei[0].cpu().numpy(), attrs.cpu().numpy()
        top = np.full(n + rec.shape[0], -np.inf)
        np.maximum.at(top, rows[cls == 1], att[cls == 1])
        top[np.isinf(top)] = np.nan
        ligand[name] = top[:n]
        per_hit.append(top[n:])
    return ligand, np.stack(per_hit)


@needs_caching_allocator
@pytest.mark.parametrize('gnn_layer', [1, 2])
def test_receptor_hotspots_equal_edge_attention_one_complex_at_a_time(gnn_layer):
    """The map of layer 1 reduces attention values normalised over ALL edges of a row (the reference's att_val), though
    the first layer only ran over the ligand-touching ones; layer 2's comes from the softmax forward under a device-side
    edge count. Bound: 1e-5 max|att64| + 4 x the fp32 oracle's distance from the fp64 oracle, as
    tests/test_gpu_contact_attention.py derives it; the fp64 oracle's own map is held to it as well."""
    from pointvs_amd.screening import ScreeningSweep
    lig, rec, lig_feats, rec_feats = _set(8204, 20)
    items = _hits(lig, lig_feats)
    model, kw = _soft_model(31, 'soft-k32')
    cfg = dict(ORACLE_KW, num_layers=3, _class='SartorrasEGNN', **SOFT)
    want64, bound = _oracle_pair(model, cfg, items, rec, rec_feats, gnn_layer)      # (RADIUS of that file: 6.0)
    model = model.cuda()
    sweep = ScreeningSweep(model, rec.cuda(), rec_feats, 6.0, batch_size=2, **kw)
    out = sweep.receptor_hotspots(items, gnn_layer=gnn_layer, per_hit=True)
    assert sweep.hotspot.reuse and sweep.hotspot._captured and sweep.hotspot.contact_attention == gnn_layer
    ligand, per_hit = _attention_map(model, items, rec, rec_feats, 6.0, gnn_layer)
    assert int((~np.isnan(per_hit)).sum()) > 20
    what = f'softmax hotspots layer {gnn_layer}'
    for name, values in out['ligand'].items():
        _close(values.cpu().numpy(), ligand[name], bound, f'{what} ligand {name}')
        _close(values.cpu().numpy(), want64['ligand'][name], bound, f'{what} ligand {name} (fp64 oracle)')
    _close(out['per_hit'].cpu().numpy(), per_hit, bound, f'{what} per_hit')
    _close(out['per_hit'].cpu().numpy(), want64['per_hit'], bound, f'{what} per_hit (fp64 oracle)')
    _close(out['max'].cpu().numpy(), want64['max'], bound, f'{what} max (fp64 oracle)')
    _close(out['mean'].cpu().numpy(), want64['mean'], bound, f'{what} mean (fp64 oracle)')
    # a value normalised over the ligand-touching edges alone would be larger wherever the row has other edges
    assert float(np.nanmax(per_hit)) < 1.0


def test_default_keyword_keeps_the_plain_route():
    """Without softmax_reuse: no reuse, capture() raises as before, and the scores are the plain forward's bits."""
    from pointvs_amd.screening import LibraryScreen, ReceptorScreen
    lig, rec, lig_feats, rec_feats = _set(6003)
    model, _ = _soft_model(1, 'rich-k32')
    slots = _slots(lig, lig_feats, SIZES, seed=40, rec=rec)
    screen = LibraryScreen(model, rec.cuda(), rec_feats, len(SIZES), 64, RADIUS)
    assert screen.reuse is False and screen.softmax_reuse is False
    with pytest.raises(RuntimeError, match='capture needs the first-layer reuse'):
        screen.capture(slots)
    got = screen(slots).clone()
    explicit = LibraryScreen(model, rec.cuda(), rec_feats, len(SIZES), 64, RADIUS, softmax_reuse=False)
    assert torch.equal(got, explicit.load(slots)._plain_forward())
    with pytest.raises(ValueError, match='pointvs_amd.attribution.bond_masking'):
        LibraryScreen(model, rec.cuda(), rec_feats, 3, 20, RADIUS, struck=True)
    with pytest.raises(NotImplementedError, match='first-layer reuse'):
        LibraryScreen(model, rec.cuda(), rec_feats, 3, 20, RADIUS, contact_attention=1)
    rs = ReceptorScreen(model, rec.cuda(), torch.cat([lig_feats[:12], rec_feats], 0), 12, 3, RADIUS)
    assert rs.reuse is False and not rs.fast_graph
    # a softmax flag without edge attention stays on the plain route whatever the keyword says
    bare = _model(1, num_layers=3, softmax_attention=True)
    assert LibraryScreen(bare, rec.cuda(), rec_feats, 3, 20, RADIUS, softmax_reuse=True).reuse is False
    # as do the cases the reuse never covered
    for flags in (dict(SOFT, edge_residual=True), dict(SOFT, k=48)):
        other = _model(1, num_layers=3, **flags)
        assert LibraryScreen(other, rec.cuda(), rec_feats, 3, 20, RADIUS, softmax_reuse=True).reuse is False


def test_sigmoid_model_scores_the_same_bits_with_the_keyword():
    from pointvs_amd.screening import LibraryScreen
    lig, rec, lig_feats, rec_feats = _set(6003)
    model = _model(1, num_layers=3, edge_attention=True, node_attention=True, tanh=True, residual=True)
    slots = _slots(lig, lig_feats, SIZES, seed=40, rec=rec)
    off = LibraryScreen(model, rec.cuda(), rec_feats, len(SIZES), 64, RADIUS)
    on = LibraryScreen(model, rec.cuda(), rec_feats, len(SIZES), 64, RADIUS, softmax_reuse=True)
    assert off.reuse and on.reuse and on.rec_magg.shape == off.rec_magg.shape == (N_REC, 32)
    assert torch.equal(off(slots), on(slots))


@pytest.mark.parametrize('kind', ['receptor', 'library'])
def test_weights_changed_under_an_eager_screen_recompute_the_statistics(kind):
    from pointvs_amd.screening import LibraryScreen, ReceptorScreen
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(6006)
    model, kw = _soft_model(3, 'rich-k32')
    if kind == 'receptor':
        feats = torch.cat([lig_feats[:12], rec_feats], 0)
        make = lambda: ReceptorScreen(model, rec.cuda(), feats, 12, 3, RADIUS, **kw)
        batch = random_poses(lig[:12], 3, seed=5, max_shift=3.0).cuda()
    else:
        make = lambda: LibraryScreen(model, rec.cuda(), rec_feats, 3, 20, RADIUS, **kw)
        batch = _slots(lig, lig_feats, (7, 20, 3), seed=90, special=False)
    screen = make()
    y0 = screen(batch).clone()
    assert screen.reuse and not screen.stale()
    _change_first_layer(model)
    assert screen.stale()
    y1 = screen(batch).clone()
    assert not screen.stale() and not torch.equal(y0, y1)
    assert torch.equal(y1, make()(batch))


@needs_caching_allocator
def test_weights_changed_under_a_captured_screen_are_refused():
    from pointvs_amd.screening import LibraryScreen
    lig, rec, lig_feats, rec_feats = _set(6006)
    model, kw = _soft_model(3, 'rich-k32')
    batch = _slots(lig, lig_feats, (7, 20, 3), seed=90, special=False)
    screen = LibraryScreen(model, rec.cuda(), rec_feats, 3, 20, RADIUS, **kw).capture(batch)
    screen.replay(batch)
    _change_first_layer(model)
    with pytest.raises(RuntimeError, match='weights changed after capture'):
        screen.replay(batch)
