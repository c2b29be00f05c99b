"""Receptor hotspot map from edge attention over a sweep's hits: the reduction (PF.contact_attention,
pvs_contact_attention) bit for bit against its numpy restatement (tests/_contact_ref.py) on a hand-built CSR, the first
layer's attention out of the partial forward (pvs_egnn_layer_fwd_partial_att) against the full layer entry, and
ScreeningSweep.receptor_hotspots against the fp64 oracle, twice on one sweep, end to end after run_library, and its errors.

Bound of the parity tests: the project's parity bound, 1e-5 * max|att64| + 4 * noise32 - att64: the fp64 oracle's values
that are compared (the row maxima of the layer's attention over ligand-receptor edges), noise32: the largest distance of
the fp32 oracle (one thread) from the fp64 oracle on the same values. Counts are exact: the poses are chosen so that no
atom pair lies within 1e-4 of the radius (asserted from the fp64 distances).
"""
import re
import tempfile

import numpy as np
import pytest
import torch

from tests import _contact_ref as ref
from tests._golden import needs_caching_allocator

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------- the operator, exact

SIZES = [0, 1, 5, 64, 65, 130, 0]          # ligand atoms per slot; the last slot is empty too
N_REC, PAD_ROWS, SENTINEL = 70, 10, -7.0
WIDE = 5                                    # the slot of 130 ligand atoms


def _row(rng, n1, n_other, layout):
    """Edge classes of one row: n1 of class 1, n_other of classes 0 / 2; class 1 first (the builders' order), last, or
    interleaved with the others."""
    other = rng.choice(np.array([0, 2], dtype=np.uint8), size=n_other)
    ones = np.ones(n1, dtype=np.uint8)
    if layout == 0:
        return np.concatenate([ones, other])
    if layout == 1:
        return np.concatenate([other, ones])
    return rng.permutation(np.concatenate([ones, other]))


def _hand_built():
    """rowptr / etype / att of a pose batch of SIZES, N_REC receptor atoms and PAD_ROWS rows of padding; att: distinct
    small integers (every sum exact in float64), some NaN. Returns the arrays and the rows made special."""
    rng = np.random.default_rng(77)
    lig_ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    node_ptr = (lig_ptr + np.arange(len(SIZES) + 1) * N_REC).astype(np.int32)
    rows, special = [], {}
    for p, n in enumerate(SIZES):
        for i in range(n):                                   # ligand rows: class-1 edges to receptor atoms
            n1 = 0 if rng.random() < 0.15 else int(rng.integers(1, N_REC + 1))
            n_other = 0 if rng.random() < 0.1 else int(rng.integers(0, 25))
            layout = len(rows) % 3
            if p == WIDE and i == 0:
                n1, layout = N_REC, 2                        # 70 class-1 edges, interleaved: more than one stride
            if p == 3 and i == 7:
                n1, special['lig_all_nan'] = 3, len(rows)
            rows.append(_row(rng, n1, n_other, layout))
        for j in range(N_REC):                               # receptor rows: class-1 edges to the slot's ligand atoms
            n1 = 0 if (n == 0 or rng.random() < 0.3) else int(rng.integers(1, n + 1))
            n_other = 0 if rng.random() < 0.1 else int(rng.integers(0, 40))
            layout = len(rows) % 3
            if p == WIDE and j == 0:
                n1, n_other, layout = 130, 33, 1             # 130 class-1 edges behind 33 others
            if p == 4 and j == 3:
                n1, special['rec_one_nan'] = 4, len(rows)
            if p == 3 and j == 5:
                n1, special['rec_all_nan'] = 2, len(rows)
            rows.append(_row(rng, n1, n_other, layout))
    n_nodes = len(rows) + PAD_ROWS
    assert len(rows) == int(node_ptr[-1]) == sum(SIZES) + len(SIZES) * N_REC
    counts = [len(r) for r in rows] + [0] * PAD_ROWS
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    etype = np.concatenate(rows).astype(np.uint8)
    att = rng.permutation(len(etype)).astype(np.float32)
    for key, row in special.items():
        ones = rowptr[row] + np.nonzero(etype[rowptr[row]:rowptr[row + 1]] == 1)[0]
        att[ones[1:2] if key == 'rec_one_nan' else ones] = np.nan
    assert n_nodes + 1 == len(rowptr) and len(etype) < 2 ** 24
    return rowptr, etype, att, node_ptr, lig_ptr, special


def _want(calls):
    rowptr, etype, att, node_ptr, lig_ptr, _ = _hand_built()
    lig_att = np.full(len(rowptr) - 1 - len(SIZES) * N_REC, SENTINEL, dtype=np.float32)
    acc = ref.fresh_accumulators(N_REC)
    for _ in range(calls):
        lig_att, slot_rec, *acc = ref.contact_attention(rowptr, etype, att, node_ptr, lig_ptr, N_REC, *acc, lig_att)
    return (lig_att, slot_rec, *acc)


def _run(calls):
    """`calls` launches into sentinel-filled outputs and fresh accumulators; the five outputs as numpy after each."""
    from pointvs_amd import functional as PF
    rowptr, etype, att, node_ptr, lig_ptr, _ = (torch.from_numpy(a).cuda() if isinstance(a, np.ndarray) else a
                                                for a in _hand_built())
    out = (torch.full((rowptr.numel() - 1 - len(SIZES) * N_REC,), SENTINEL).cuda(),
           torch.full((len(SIZES), N_REC), SENTINEL).cuda()) + PF.new_contact_accumulators(N_REC, 'cuda')
    after = []
    for _ in range(calls):
        got = PF.contact_attention(rowptr, etype, att, node_ptr, lig_ptr, N_REC, out=out)
        assert all(g is o for g, o in zip(got, out))
        after.append(tuple(t.cpu().numpy() for t in got))
    return after


_RUNS = {}


def _first_run():
    if 'runs' not in _RUNS:
        _RUNS['runs'] = _run(2)
    return _RUNS['runs']


NAMES = ('lig_att', 'slot_rec_att', 'rec_sum', 'rec_count', 'rec_max')


def test_operator_is_exact():
    rowptr, etype, att, node_ptr, lig_ptr, special = _hand_built()
    want = _want(1)
    # the inputs hold what the issue asks for
    wide_rec, wide_lig = int(node_ptr[WIDE]) + SIZES[WIDE], int(node_ptr[WIDE])
    assert int((etype[rowptr[wide_rec]:rowptr[wide_rec + 1]] == 1).sum()) == 130
    assert int((etype[rowptr[wide_lig]:rowptr[wide_lig + 1]] == 1).sum()) == 70
    assert np.isnan(want[1]).any() and np.isnan(want[0][:sum(SIZES)]).any()           # rows without a class-1 edge
    assert np.isnan(want[0][int(lig_ptr[3]) + 7])                                       # the rows with NaN only
    assert np.isnan(want[1][3, 5]) and not np.isnan(want[1][4, 3])                      # ... and the row with one NaN
    assert np.isnan(want[1][0]).all() and np.isnan(want[1][-1]).all()                   # the empty slots
    assert int(want[3].max()) >= 3 and len(set(want[3].tolist())) > 1
    got = _first_run()[0]
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert g.tobytes() == w.tobytes(), (name, np.nonzero(~((g == w) | (np.isnan(g) & np.isnan(w)))))
    assert (got[0][sum(SIZES):] == SENTINEL).all() and len(got[0]) == sum(SIZES) + PAD_ROWS


def test_operator_accumulates_across_calls():
    once, twice = _first_run()
    want = _want(2)
    for name, g, w in zip(NAMES, twice, want):
        assert g.tobytes() == w.tobytes(), name
    assert np.array_equal(twice[2], 2 * once[2]) and np.array_equal(twice[3], 2 * once[3])
    assert twice[0].tobytes() == once[0].tobytes() and twice[1].tobytes() == once[1].tobytes()
    assert twice[4].tobytes() == once[4].tobytes()


def test_operator_is_reproducible_and_allocates():
    from pointvs_amd import functional as PF
    for a, b in zip(_first_run(), _run(2)):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    rowptr, etype, att, node_ptr, lig_ptr, _ = _hand_built()
    got = PF.contact_attention(*(torch.from_numpy(a).cuda() for a in (rowptr, etype, att, node_ptr, lig_ptr)), N_REC)
    want = _want(1)
    n = sum(SIZES)
    assert got[0].shape == (n + PAD_ROWS,) and got[1].shape == (len(SIZES), N_REC)
    assert got[0][:n].cpu().numpy().tobytes() == want[0][:n].tobytes()
    for g, w in zip(got[1:], want[1:]):
        assert g.cpu().numpy().tobytes() == w.tobytes()
    # no slots, no receptor: nothing to do
    empty = torch.zeros(1, dtype=torch.int32).cuda()
    out = PF.contact_attention(torch.from_numpy(rowptr).cuda(), torch.from_numpy(etype).cuda(),
                               torch.from_numpy(att).cuda(), empty, empty, N_REC)
    assert out[1].shape == (0, N_REC) and not out[3].any() and bool(torch.isnan(out[4]).all())


def test_operator_wrapper_refuses_wrong_arguments():
    from pointvs_amd import functional as PF
    rowptr, etype, att, node_ptr, lig_ptr = (torch.from_numpy(a).cuda() for a in _hand_built()[:5])
    n_lig, n_slots = rowptr.numel() - 1 - len(SIZES) * N_REC, len(SIZES)

    def out(lig=n_lig, slots=n_slots, rec=N_REC, sum_dtype=torch.float64):
        return (torch.zeros(lig).cuda(), torch.zeros((slots, N_REC)).cuda(), torch.zeros(rec, dtype=sum_dtype).cuda(),
                torch.zeros(N_REC, dtype=torch.int32).cuda(), torch.zeros(N_REC).cuda())
    with pytest.raises(TypeError):
        PF.contact_attention(rowptr, etype, att.double(), node_ptr, lig_ptr, N_REC)
    with pytest.raises(ValueError):
        PF.contact_attention(rowptr.long(), etype, att, node_ptr, lig_ptr, N_REC)
    with pytest.raises(ValueError):
        PF.contact_attention(rowptr, etype.int(), att, node_ptr, lig_ptr, N_REC)
    with pytest.raises(ValueError):
        PF.contact_attention(rowptr, etype, att[:-1], node_ptr, lig_ptr, N_REC)           # att shorter than the edges
    with pytest.raises(ValueError):
        PF.contact_attention(rowptr, etype, att, node_ptr, lig_ptr[:-1], N_REC)
    with pytest.raises(ValueError):
        PF.contact_attention(rowptr, etype, att, node_ptr, lig_ptr, 2 * N_REC)            # more receptor rows than rows
    for bad in (out(lig=n_lig - 1), out(slots=n_slots - 1), out(rec=N_REC - 1), out(sum_dtype=torch.float32)):
        with pytest.raises(ValueError, match='out ='):
            PF.contact_attention(rowptr, etype, att, node_ptr, lig_ptr, N_REC, out=bad)
    with pytest.raises(RuntimeError):
        PF.contact_attention(rowptr.cpu(), etype.cpu(), att.cpu(), node_ptr.cpu(), lig_ptr.cpu(), N_REC)
    with pytest.raises(RuntimeError):
        PF.contact_attention(rowptr, etype, att, node_ptr, lig_ptr, N_REC, out=tuple(t.cpu() for t in out()))
    PF.contact_attention(rowptr, etype, att, node_ptr, lig_ptr, N_REC, out=out())           # (the sizes above: fine)


# ---------------------------------------------------------------- the model, the receptor, the hits

N_REC_SCREEN, RADIUS, SEED = 150, 6.0, 8204       # (this seed: the nearest atom pair is 8.0e-4 from the radius)
KW = dict(dim_input=12, k=32, dim_output=1, num_layers=2, residual=False, edge_residual=False,
          edge_attention=False, normalize=False, tanh=False, dropout=0.0, graphnorm=False, update_coords=True,
          permutation_invariance=False, node_attention=False, gated_residual=False, rezero=False,
          softmax_attention=False, model_task='classification')


def attention_model(seed, **flags):
    """SartorrasEGNN, k = 32, three layers, sigmoid edge attention; on the CPU."""
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    torch.manual_seed(seed)
    return SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True,
                         **{**KW, 'edge_attention': True, 'num_layers': 3, **flags}).eval()


def _set(seed, n_lig):
    """(ligand [n_lig,3], receptor [150,3], ligand feats, receptor feats): the 150 receptor atoms of a screening_set
    nearest its centre (as tests/test_gpu_ligand_masking.py)."""
    from pointvs_amd.synthetic import screening_set
    lig, rec, feats = screening_set(seed=seed, n_nodes=n_lig + 400, n_lig=n_lig)
    near = torch.argsort((rec - lig.mean(0)).norm(dim=1))[:N_REC_SCREEN].sort().values
    return lig, rec[near].contiguous(), feats[:n_lig].contiguous(), feats[n_lig:][near].contiguous()


def hits_and_receptor(seed=SEED):
    """Hits of 1, 12, 12 and 70 atoms in one pose each (made on the CPU), the receptor, its features."""
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(seed, 70)
    specs = [('hit1', lig_feats[5:6], lig[5:6]), ('hitA', lig_feats[:12], lig[:12]),
             ('hitB', lig_feats[:12].roll(3, 0), lig[:12].flip(0) * 0.9), ('hitC', lig_feats, lig)]
    items = [(name, feats.contiguous(), random_poses(pos, 1, seed=seed + k, max_shift=3.0)[0].contiguous())
             for k, (name, feats, pos) in enumerate(specs)]
    return items, rec, rec_feats


_YARD = {}


def _yardstick():
    """The oracle's maps of layers 1 and 3 (= -1) in fp64, the same from the fp32 oracle on one thread, and per layer
    noise32, max|att64| and the bound; computed once."""
    if not _YARD:
        items, rec, rec_feats = hits_and_receptor()
        model = attention_model(31)
        sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        cfg = dict(KW, edge_attention=True, num_layers=3, _class='SartorrasEGNN')
        y64 = ref.oracle_hotspots(sd, cfg, items, rec, rec_feats, RADIUS, (1, 3), torch.float64)
        threads = torch.get_num_threads()
        torch.set_num_threads(1)
        try:
            y32 = ref.oracle_hotspots(sd, cfg, items, rec, rec_feats, RADIUS, (1, 3), torch.float32)
        finally:
            torch.set_num_threads(threads)
        _YARD.update(items=items, rec=rec, rec_feats=rec_feats, model=model, y64=y64, bound={}, noise32={})
        for layer in (1, 3):
            a, b = y64[layer], y32[layer]
            assert np.array_equal(a['count'], b['count'])
            pairs = [(a[k], b[k]) for k in ('per_hit', 'mean', 'max')] + [(a['ligand'][n], b['ligand'][n])
                                                                           for n in a['ligand']]
            assert all(np.array_equal(np.isnan(u), np.isnan(v)) for u, v in pairs)
            noise = max(float(np.nanmax(np.abs(u - v))) for u, v in pairs)
            scale = float(np.nanmax(np.abs(a['per_hit'])))
            _YARD['noise32'][layer], _YARD['bound'][layer] = noise, 1e-5 * scale + 4 * noise
            print(f'layer {layer}: max|att64| {scale:.4f} noise32 {noise:.3e} bound {_YARD["bound"][layer]:.3e}')
        _check_yardstick(_YARD)
    return _YARD


def _check_yardstick(y):
    """On the oracle's numbers alone: no atom pair within 1e-4 of the radius (so the counts are exact), and the inputs
    tell implementations apart - with a factor of 10 over the bound the two layers' maps differ, some receptor atom's
    values differ between its contacts, and the mean is not the max."""
    gap = ref.radius_gap(y['items'], y['rec'], RADIUS)
    print(f'nearest pair to the radius: {gap:.3e}')
    assert gap > 1e-4
    bound = max(y['bound'].values())
    first, last = y['y64'][1], y['y64'][3]
    assert np.array_equal(first['count'], last['count']) and int(first['count'].max()) >= 2
    assert int((first['count'] == 0).sum()) > 0
    assert float(np.nanmax(np.abs(first['mean'] - last['mean']))) > 10 * bound
    for m in (first, last):
        has = ~np.isnan(m['per_hit'])
        spread = np.where(has, m['per_hit'], -np.inf).max(0) - np.where(has, m['per_hit'], np.inf).min(0)
        assert float(spread[m['count'] >= 2].max()) > 10 * bound
        assert float(np.nanmax(np.abs(m['mean'] - m['max']))) > 10 * bound


def _close(got, want, bound, what):
    """NaN in the same places, the rest within `bound`; the figure is printed first."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    err = float(np.nanmax(np.abs(got - want))) if (~np.isnan(want)).any() else 0.0
    print(f'{what}: err {err:.3e} bound {bound:.3e}')
    assert err <= bound, f'{what}: {err:.3e} > {bound:.3e}'


# ---------------------------------------------------------------- the partial entry

def test_partial_entry_hands_out_the_first_layers_attention():
    """pvs_egnn_layer_fwd_partial_att over a ligand-touching graph that holds ALL of each row's edges, on bases of zero,
    is the layer itself: its att_out against the att_out of pvs_egnn_layer_fwd on the same graph, bit for bit; h_out and
    x_out the same bits with att_out NULL and given."""
    from pointvs_amd.radius_graph import radius_graph
    from pointvs_amd.screening import LibraryScreen
    items, rec, rec_feats = hits_and_receptor()
    model = attention_model(31).cuda()
    _, feats, pose = items[1]
    pos = torch.cat([pose, rec], 0).cuda().contiguous()
    x_in = torch.cat([feats, rec_feats], 0).cuda().float()
    pg = radius_graph(pos, x_in[:, -1], None, RADIUS, RADIUS, need_backward=False, ligand_pairs_only=True)
    n, e = pg.n_nodes, pg.n_edges
    assert e > 200 and int((pg.t['etype'][:e] == 1).sum()) > 50
    layer = model.layers[1]
    with torch.no_grad():
        h = model.layers[0].embed(x_in, pos).contiguous()
        layer.forward_prepared(pg, h, pos)
        att_full = layer._att_sorted[:e].clone()
        screen = LibraryScreen(model, rec.cuda(), rec_feats, 1, 12, RADIUS)
        zeros = [torch.zeros((n, w), device='cuda') for w in (32, 3)] + [torch.zeros(n, device='cuda')]
        h_a, x_a = screen._partial_first_layer(pg.c, h, pos, *zeros, n, e)
        att_out = torch.full((e + 5,), SENTINEL, device='cuda')
        h_b, x_b = screen._partial_first_layer(pg.c, h, pos, *zeros, n, e, att_out=att_out)
    assert torch.equal(att_out[:e], att_full) and bool((att_out[e:] == SENTINEL).all())
    assert float(att_full.min()) > 0 and float(att_full.max()) < 1 and float(att_full.std()) > 1e-3
    assert torch.equal(h_a, h_b) and torch.equal(x_a, x_b)
    assert bool(torch.isfinite(h_b).all()) and not torch.equal(x_b, pos)


# ---------------------------------------------------------------- parity with the fp64 oracle

def _sweep(capture, batch_size=3):
    from pointvs_amd.screening import ScreeningSweep
    y = _yardstick()
    return ScreeningSweep(y['model'].cuda(), y['rec'].cuda(), y['rec_feats'], RADIUS, batch_size=batch_size,
                          capture=capture)


@pytest.mark.parametrize('capture', [pytest.param(True, marks=needs_caching_allocator), False], ids=['captured', 'eager'])
@pytest.mark.parametrize('gnn_layer', [1, -1])
def test_parity_with_the_fp64_oracle(gnn_layer, capture):
    y = _yardstick()
    layer = 3 if gnn_layer == -1 else gnn_layer
    want, bound = y['y64'][layer], y['bound'][layer]
    sweep = _sweep(capture)
    out = sweep.receptor_hotspots(y['items'], gnn_layer=gnn_layer, per_hit=True)
    assert sweep.hotspot.contact_attention == layer and sweep.hotspot._captured == capture
    assert sweep.batches_run == 1 + 2                      # the sizing batch, then ceil(4 / 3) steps
    assert out['count'].dtype == torch.int32 and out['per_hit'].shape == (4, N_REC_SCREEN)
    count = out['count'].cpu().numpy()
    print(f'layer {gnn_layer} capture={capture}: contacts {int(count.sum())} on {int((count > 0).sum())} atoms')
    assert np.array_equal(count, want['count'])
    what = f'layer {gnn_layer} capture={capture}'
    assert list(out['ligand']) == [name for name, _, _ in y['items']]
    for name, values in out['ligand'].items():
        _close(values.cpu().numpy(), want['ligand'][name], bound, f'{what} ligand {name}')
    _close(out['per_hit'].cpu().numpy(), want['per_hit'], bound, f'{what} per_hit')
    _close(out['mean'].cpu().numpy(), want['mean'], bound, f'{what} mean')
    _close(out['max'].cpu().numpy(), want['max'], bound, f'{what} max')


def _oracle_pair(model, cfg, items, rec, rec_feats, layer):
    """(the fp64 oracle's map of `layer`, the parity bound from the fp32 oracle's distance to it) for `model`."""
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    a = ref.oracle_hotspots(sd, cfg, items, rec, rec_feats, RADIUS, (layer,), torch.float64)[layer]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        b = ref.oracle_hotspots(sd, cfg, items, rec, rec_feats, RADIUS, (layer,), torch.float32)[layer]
    finally:
        torch.set_num_threads(threads)
    noise = max(float(np.nanmax(np.abs(a[k] - b[k]))) for k in ('per_hit', 'mean', 'max'))
    return a, 1e-5 * float(np.nanmax(np.abs(a['per_hit']))) + 4 * noise


def test_graphnorm_model_runs_eager_at_the_exact_node_count():
    """GraphNorm takes its statistics over the batch's nodes: one hit per step is the oracle's one graph per forward, so
    the same yardstick and bound hold (a padded shape would shift every value by far more)."""
    from pointvs_amd.screening import ScreeningSweep
    items, rec, rec_feats = hits_and_receptor()
    items = items[:3]
    model = attention_model(32, graphnorm=True)
    cfg = dict(KW, edge_attention=True, num_layers=3, graphnorm=True, _class='SartorrasEGNN')
    want, bound = _oracle_pair(model, cfg, items, rec, rec_feats, 1)
    sweep = ScreeningSweep(model.cuda(), rec.cuda(), rec_feats, RADIUS, batch_size=1)
    out = sweep.receptor_hotspots(items, per_hit=True)
    assert sweep.hotspot.graphnorm and not sweep.hotspot._captured and sweep.batches_run == 1 + 3
    assert np.array_equal(out['count'].cpu().numpy(), want['count']) and int(want['count'].max()) >= 2
    _close(out['per_hit'].cpu().numpy(), want['per_hit'], bound, 'graphnorm per_hit')
    _close(out['mean'].cpu().numpy(), want['mean'], bound, 'graphnorm mean')
    _close(out['max'].cpu().numpy(), want['max'], bound, 'graphnorm max')


# ---------------------------------------------------------------- accumulator hygiene, end to end, errors

@needs_caching_allocator
def test_nothing_leaks_into_the_accumulators():
    """A fresh sweep: the sizing batch, the capture (two warm-up steps and the captured one), then the run. The counts
    add up to the oracle's, and a second call on the same sweep gives the same bytes."""
    y = _yardstick()
    sweep = _sweep(True)
    first = sweep.receptor_hotspots(y['items'], per_hit=True)
    assert sweep.batches_run == 3 and sweep.hotspot._captured
    screen = sweep.hotspot
    again = sweep.receptor_hotspots(y['items'], per_hit=True)
    assert sweep.hotspot is screen and sweep.batches_run == 5
    assert int(first['count'].sum()) == int(y['y64'][1]['count'].sum()) > 0
    for key in ('mean', 'count', 'max', 'per_hit'):
        assert first[key].cpu().numpy().tobytes() == again[key].cpu().numpy().tobytes(), key
    for name in first['ligand']:
        assert first['ligand'][name].cpu().numpy().tobytes() == again['ligand'][name].cpu().numpy().tobytes()
    # another layer: a new screen; an eager sweep: the same counts
    sweep.receptor_hotspots(y['items'], gnn_layer=2)
    assert sweep.hotspot is not screen and sweep.hotspot.contact_attention == 2
    eager = _sweep(False).receptor_hotspots(y['items'])
    assert torch.equal(eager['count'], first['count']) and 'per_hit' not in eager
    # no items: nothing to run
    none = sweep.receptor_hotspots([], per_hit=True)
    assert bool(torch.isnan(none['mean']).all()) and bool(torch.isnan(none['max']).all()) and not none['count'].any()
    assert none['ligand'] == {} and none['per_hit'].shape == (0, N_REC_SCREEN)


def _library(lig, lig_feats):
    from pointvs_amd.synthetic import random_poses
    ligs = [('ligA', lig_feats[:12], lig[:12], 7), ('ligB', lig_feats[:9].roll(1, 0), lig[:9] * 0.9, 5),
            ('ligC', lig_feats, lig, 3), ('ligNone', lig_feats[:5], lig[:5], 0),
            ('ligD', lig_feats[:12].roll(3, 0), lig[:12].flip(0), 4), ('ligE', lig_feats[5:6], lig[5:6], 2)]
    return [(name, f, random_poses(pos, n, seed=20 + k, max_shift=3.0).cuda()) for k, (name, f, pos, n) in enumerate(ligs)]


@needs_caching_allocator
def test_end_to_end_after_run_library(tmp_path):
    """run_library with a hits file, then the hotspot map of every hit: ligands of 12, 9, 70, 12 and 1 atoms and one
    without poses, which is skipped."""
    from pointvs_amd.screening import ScreeningSweep
    lig, rec, lig_feats, rec_feats = _set(8102, 70)
    work = _library(lig, lig_feats)
    sweep = ScreeningSweep(attention_model(5).cuda(), rec.cuda(), rec_feats, edge_radius=RADIUS, batch_size=4)
    sweep.run_library(work, hits_file=tmp_path / 'hits.txt')
    assert sweep.hits['ligNone'][0] == -1
    before = sweep.batches_run
    out = sweep.receptor_hotspots(sweep.best_poses(work), scores_file=tmp_path / 'hotspots.txt')
    sizes = {'ligA': 12, 'ligB': 9, 'ligC': 70, 'ligD': 12, 'ligE': 1}
    assert sweep.batches_run - before == 1 + -(-len(sizes) // 4)
    assert {name: int(v.shape[0]) for name, v in out['ligand'].items()} == sizes
    assert sweep.hotspot.max_lig_atoms == 70 and sweep.hotspot._captured and sweep.library.contact is None
    mean, count = out['mean'].cpu().numpy(), out['count'].cpu().numpy()
    assert mean.dtype == np.float64 and 0 < int((count > 0).sum()) < N_REC_SCREEN and int(count.max()) <= len(sizes)
    assert np.array_equal(np.isnan(mean), count == 0)
    lines = (tmp_path / 'hotspots.txt').read_text().splitlines()
    atoms = np.nonzero(count > 0)[0]
    assert len(lines) == len(atoms)
    for line, j in zip(lines, atoms):
        assert re.fullmatch(r'\d\.\d{6} \d+ \| receptor atom\d+', line), line
        assert line == f'{mean[j]:.6f} {count[j]} | receptor atom{j}'
    # no items: an empty file
    sweep.receptor_hotspots([], scores_file=tmp_path / 'none.txt')
    assert (tmp_path / 'none.txt').read_text() == ''


def test_errors():
    from pointvs_amd.screening import MAX_SCREEN_LIGAND_ATOMS, LibraryScreen, ScreeningSweep
    items, rec, rec_feats = hits_and_receptor()
    item = items[1]

    def sweep_of(model, **kw):
        return ScreeningSweep(model, rec.cuda(), rec_feats, edge_radius=RADIUS, batch_size=3, capture=False, **kw)
    plain = attention_model(6, edge_attention=False).cuda()
    with pytest.raises(ValueError, match=r'no edge attention \(the layers that have it: \[\], of 4\)'):
        sweep_of(plain).receptor_hotspots([item])
    sweep = sweep_of(attention_model(6).cuda())
    with pytest.raises(ValueError, match=r'the layers that have it: \[1, 2, 3\]'):
        sweep.receptor_hotspots([item], gnn_layer=0)                  # the embedding
    with pytest.raises(ValueError, match='no edge attention'):
        sweep.receptor_hotspots([item], gnn_layer=4)
    with pytest.raises(NotImplementedError, match='first-layer reuse'):
        sweep_of(attention_model(6, softmax_attention=True).cuda()).receptor_hotspots([item])
    with pytest.raises(NotImplementedError, match='fp32 only'):
        ScreeningSweep(attention_model(6).double().cuda(), rec.cuda().double(), rec_feats.double(), edge_radius=RADIUS,
                       batch_size=3).receptor_hotspots([item])
    with pytest.raises(ValueError, match='receptor_hotspots: names must be unique'):
        sweep.receptor_hotspots([item, items[0], item])
    n = MAX_SCREEN_LIGAND_ATOMS + 1
    with pytest.raises(ValueError, match="'huge' has 1025 atoms"):
        sweep.receptor_hotspots([('huge', item[1][:1].expand(n, -1), torch.zeros(n, 3))])
    with pytest.raises(RuntimeError, match='without contact_attention'):
        LibraryScreen(plain, rec.cuda(), rec_feats, 3, 12, RADIUS).reset_contact_attention()
    assert list(sweep.receptor_hotspots([item])['ligand']) == ['hitA']              # (the sweep is still usable)
