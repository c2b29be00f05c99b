"""Class-activation maps of a sweep's hits: the per-node heads (PF.node_heads, pvs_node_heads_fwd) bit for bit against the
pooled heads on one-row graphs, exact on integers and within the dot-product bound on normal data; the slot operator
(PF.slot_node_values, pvs_slot_node_values) bit for bit against its numpy restatement (tests/_cam_ref.py); and
ScreeningSweep.receptor_hotspots(attribution='cam') against the fp64 oracle, the screen's own scores and
pointvs_amd.attribution.cam, twice on one sweep, for the other head shapes and routes, end to end, and its errors.

Bound of the parity tests: 1e-5 * max|cam64| + 4 * noise32 - cam64: the fp64 oracle's values that are compared, noise32:
the largest distance of the fp32 oracle (one thread) from them (tests/_cam_ref.py: noise_and_bound). On the set-up of the
main test (tests/test_cam_host.py prints the same): max|cam64| 0.452, noise32 4.3e-7 to 5.7e-7 with the CPU the oracle runs
on, bound 6.2e-6 to 6.8e-6; the sweep was measured 3.5e-7 from the oracle at most.
"""
import re
import tempfile

import numpy as np
import pytest
import torch

from tests import _cam_ref as ref
from tests import _dense_ref as dense
from tests._golden import needs_caching_allocator
from tests.test_gpu_contact_attention import KW, N_REC_SCREEN, RADIUS, _close, _library, _set, attention_model, hits_and_receptor

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------- the heads on every row

WIDTHS = [1, 20, 32, 64, 128]
ROWS = [0, 1, 63, 64, 65, 127, 128, 129, 1000]      # the tile has 128 rows up to width 76 and 64 at width 128
HEAD_SETS = {'one column': [(1, None)], 'three, softplus': [(3, 'softplus')], 'pose + three, relu': [(1, None), (3, 'relu')],
             'four heads': [(1, None), (2, 'relu'), (3, 'softplus'), (5, None)]}
PIECEWISE_LINEAR = {'one column': [(1, None)], 'pose + three, relu': [(1, None), (3, 'relu')],
                    'four heads': [(1, None), (2, 'relu'), (3, None), (5, 'relu')]}


def _heads(rng, width, spec, integer):
    """[(W [C, width], b [C] or None, act)] on the device and as numpy; the second head, if any, has no bias."""
    host = [(dense.make_data(rng, (c, width), np.float32, integer),
             None if i == 1 else dense.make_data(rng, (c,), np.float32, integer), act) for i, (c, act) in enumerate(spec)]
    dev = [(torch.from_numpy(w).cuda(), None if b is None else torch.from_numpy(b).cuda(), act) for w, b, act in host]
    return host, dev


def _rows(rng, n, width, integer):
    h = dense.make_data(rng, (n, width), np.float32, integer)
    h[h == 0] = 0.0                                     # (no -0.0: a pooled row is 0 + x)
    return h


@pytest.mark.parametrize('width', WIDTHS)
def test_heads_are_the_pooled_heads_on_one_row_graphs(width):
    from pointvs_amd import functional as PF
    rng = np.random.default_rng(width)
    for n in ROWS:
        h = torch.from_numpy(_rows(rng, n, width, False)).cuda()
        ptr = torch.arange(n + 1, dtype=torch.int32, device='cuda')
        for name, spec in HEAD_SETS.items():
            _, heads = _heads(rng, width, spec, False)
            got, want = PF.node_heads(h, heads), PF.pool_heads(h, ptr, heads)
            assert got.shape == want.shape == (n, sum(c for c, _ in spec)) and got.dtype == torch.float32
            assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes(), (width, n, name)
            assert PF.node_heads(h, heads).cpu().numpy().tobytes() == got.cpu().numpy().tobytes()      # run twice
            assert n == 0 or bool(torch.isfinite(got).all())


@pytest.mark.parametrize('width', WIDTHS)
def test_heads_on_integers_and_on_normal_data(width):
    """Integers in [-4, 4]: bit for bit the int64 product (ReLU of it). Normal data: within gamma(width + 3) S of the
    fp64 product (ReLU does not stretch a distance)."""
    from pointvs_amd import functional as PF
    rng = np.random.default_rng(100 + width)
    for integer in (True, False):
        for n in (1, 129, 1000):
            x = _rows(rng, n, width, integer)
            for name, spec in PIECEWISE_LINEAR.items():
                host, heads = _heads(rng, width, spec, integer)
                got, at = PF.node_heads(torch.from_numpy(x).cuda(), heads).cpu().numpy(), 0
                for w, b, act in host:
                    r = dense.linear_ref(x, w, b, np.zeros((n, w.shape[0]), dtype=np.float32), integer)['y']
                    if act == 'relu':
                        r = r._replace(value=np.maximum(r.value, 0))
                    dense.assert_matches(got[:, at:at + w.shape[0]], r, integer, f'width {width} rows {n} {name} {act}')
                    at += w.shape[0]


def test_heads_write_into_a_buffer_and_refuse_what_pool_heads_refuses():
    from pointvs_amd import functional as PF
    rng = np.random.default_rng(5)
    h = torch.from_numpy(_rows(rng, 70, 32, False)).cuda()
    _, heads = _heads(rng, 32, [(1, None), (3, 'relu')], False)
    out = torch.full((80, 4), -7.0, device='cuda')
    got = PF.node_heads(h, heads, out=out)
    assert got.data_ptr() == out.data_ptr() and torch.equal(got, PF.node_heads(h, heads)) and bool((out[70:] == -7.0).all())
    # an unaligned base takes the 4-byte path: the same bits
    shifted = torch.cat([h.new_zeros(1), h.reshape(-1)])[1:].reshape(70, 32)
    assert shifted.data_ptr() % 16 != 0 and torch.equal(PF.node_heads(shifted, heads), got)
    w, b, _ = heads[0]
    with pytest.raises(ValueError, match='node_heads: activation'):
        PF.node_heads(h, [(w, b, 'gelu')])
    with pytest.raises(ValueError, match='node_heads: head 0'):
        PF.node_heads(h, [(w[:, :31], b, None)])
    with pytest.raises(TypeError):
        PF.node_heads(h.double(), heads)
    with pytest.raises(RuntimeError, match=r'5 heads \(1\.\.4'):
        PF.node_heads(h, [(w, b, None)] * 5)
    with pytest.raises(RuntimeError, match='forward only'):
        with torch.enable_grad():
            PF.node_heads(h.clone().requires_grad_(), heads)
    with pytest.raises(RuntimeError):
        PF.node_heads(h.cpu(), heads)
    with pytest.raises(ValueError, match='out ='):
        PF.node_heads(h, heads, out=torch.zeros((69, 4), device='cuda'))
    with pytest.raises(RuntimeError, match='width 1025 unsupported'):
        PF.node_heads(torch.zeros((2, 1025), device='cuda'), [(torch.zeros((1, 1025), device='cuda'), None, None)])
    wide = torch.from_numpy(_rows(rng, 9, 1024, False)).cuda()          # the widest row: tiles of 8 rows
    _, wide_heads = _heads(rng, 1024, [(2, None)], False)
    assert torch.equal(PF.node_heads(wide, wide_heads), PF.pool_heads(wide, torch.arange(10, dtype=torch.int32, device='cuda'), wide_heads))


# ---------------------------------------------------------------- the slot operator, exact

SIZES = [0, 1, 5, 64, 65, 130, 0]          # ligand atoms per slot; the last slot is empty too
N_REC, PAD_ROWS, SENTINEL = 70, 10, -7.0
NAMES = ('lig_val', 'slot_rec_val', 'rec_sum', 'rec_count', 'rec_max')


def _batch(broken=False):
    """y [N, 4] (normal values, some NaN, a row whose three columns cancel in one order only), node_ptr, lig_ptr."""
    rng = np.random.default_rng(78)
    lig_ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    node_ptr = (lig_ptr + np.arange(len(SIZES) + 1) * N_REC).astype(np.int32)
    n_nodes = int(node_ptr[-1]) + PAD_ROWS
    y = rng.standard_normal((n_nodes, 4)).astype(np.float32)
    y[rng.random(y.shape) < 0.02] = np.nan
    y[int(node_ptr[2]) + SIZES[2] + 7] = (7.0, 1e8, 1.0, -1e8)       # receptor atom 7 of the slot of five atoms
    y[int(node_ptr[3])] = (np.nan, 0.5, -0.0, 0.0)                   # a ligand row
    if broken:
        node_ptr[4] += 1                                             # spoils the slots of 64 and of 65 atoms
    return y, node_ptr, lig_ptr


def _run_slots(calls, column, n_mean, broken=False):
    from pointvs_amd import functional as PF
    y, node_ptr, lig_ptr = (torch.from_numpy(a).cuda() for a in _batch(broken))
    out = (torch.full((y.shape[0] - len(SIZES) * N_REC,), SENTINEL).cuda(),
           torch.full((len(SIZES), N_REC), SENTINEL).cuda()) + PF.new_contact_accumulators(N_REC, 'cuda')
    after = []
    for _ in range(calls):
        got = PF.slot_node_values(y, node_ptr, lig_ptr, N_REC, column, n_mean, out=out)
        assert all(g is o for g, o in zip(got, out))
        after.append(tuple(t.cpu().numpy() for t in got))
    return after


def _want_slots(calls, column, n_mean, broken=False):
    y, node_ptr, lig_ptr = _batch(broken)
    lig_val = np.full(y.shape[0] - len(SIZES) * N_REC, SENTINEL, dtype=np.float32)
    acc = ref.fresh_accumulators(N_REC)
    for _ in range(calls):
        lig_val, slot_rec, *acc = ref.slot_node_values(y, column, n_mean, node_ptr, lig_ptr, N_REC, *acc, lig_val)
    return (lig_val, slot_rec, *acc)


@pytest.mark.parametrize('column,n_mean,broken', [(0, 1, False), (3, 1, False), (1, 3, False), (0, 3, False), (1, 3, True)])
def test_slot_operator_is_exact_and_accumulates(column, n_mean, broken):
    once, twice = _run_slots(2, column, n_mean, broken)
    again = _run_slots(2, column, n_mean, broken)
    for calls, got in ((1, once), (2, twice)):
        want = _want_slots(calls, column, n_mean, broken)
        for name, g, w in zip(NAMES, got, want):
            assert g.dtype == w.dtype and g.shape == w.shape, name
            assert g.tobytes() == w.tobytes(), (name, calls, np.nonzero(~((g == w) | (np.isnan(g) & np.isnan(w)))))
    for a, b in zip((once, twice), again):                               # the same bits every time
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    lig_val, slot_rec, _, count, _ = once
    assert (lig_val[sum(SIZES):] == SENTINEL).all()
    assert np.isnan(slot_rec[0]).all() and np.isnan(slot_rec[-1]).all()                  # the empty slots
    assert np.isnan(slot_rec[1:-1]).any() and not np.isnan(slot_rec[1:-1]).all(axis=1).any() or broken
    if broken:
        assert np.isnan(slot_rec[3:5]).all() and not np.isnan(slot_rec[5]).all()
        assert (lig_val[6:6 + 64 + 65] == SENTINEL).all() and int(count.max()) == 3
    elif n_mean == 3 and column == 1:
        assert slot_rec[2, 7] == 0.0 and np.float32((1e8 - 1e8 + 1.0) / 3) != 0.0      # the stated order, no other
    assert np.array_equal(twice[3], 2 * once[3])


def test_slot_operator_allocates_and_refuses_wrong_arguments():
    from pointvs_amd import functional as PF
    y, node_ptr, lig_ptr = (torch.from_numpy(a).cuda() for a in _batch())
    n_lig, n_slots = y.shape[0] - len(SIZES) * N_REC, len(SIZES)
    got, want = PF.slot_node_values(y, node_ptr, lig_ptr, N_REC, column=2), _want_slots(1, 2, 1)
    assert got[0].shape == (n_lig,) and got[1].shape == (n_slots, N_REC)
    assert got[0][:sum(SIZES)].cpu().numpy().tobytes() == want[0][:sum(SIZES)].tobytes()
    for g, w in zip(got[1:], want[1:]):
        assert g.cpu().numpy().tobytes() == w.tobytes()
    empty = torch.zeros(1, dtype=torch.int32).cuda()
    none = PF.slot_node_values(y, empty, empty, N_REC)
    assert none[1].shape == (0, N_REC) and not none[3].any() and bool(torch.isnan(none[4]).all())

    def out(lig=n_lig, slots=n_slots, rec=N_REC, sum_dtype=torch.float64):
        return (torch.zeros(lig).cuda(), torch.zeros((slots, N_REC)).cuda(), torch.zeros(rec, dtype=sum_dtype).cuda(),
                torch.zeros(N_REC, dtype=torch.int32).cuda(), torch.zeros(N_REC).cuda())
    with pytest.raises(TypeError):
        PF.slot_node_values(y.double(), node_ptr, lig_ptr, N_REC)
    for column, n_mean in ((4, 1), (-1, 1), (2, 3), (0, 2), (0, 4)):
        with pytest.raises(ValueError, match='one column or the mean of three'):
            PF.slot_node_values(y, node_ptr, lig_ptr, N_REC, column, n_mean)
    with pytest.raises(ValueError):
        PF.slot_node_values(y, node_ptr.long(), lig_ptr, N_REC)
    with pytest.raises(ValueError):
        PF.slot_node_values(y, node_ptr, lig_ptr[:-1], N_REC)
    with pytest.raises(ValueError):
        PF.slot_node_values(y, node_ptr, lig_ptr, 2 * N_REC)
    for bad in (out(lig=n_lig - 1), out(slots=n_slots - 1), out(rec=N_REC - 1), out(sum_dtype=torch.float32)):
        with pytest.raises(ValueError, match='out ='):
            PF.slot_node_values(y, node_ptr, lig_ptr, N_REC, out=bad)
    with pytest.raises(RuntimeError):
        PF.slot_node_values(y.cpu(), node_ptr.cpu(), lig_ptr.cpu(), N_REC)
    with pytest.raises(RuntimeError):
        PF.slot_node_values(y, node_ptr, lig_ptr, N_REC, out=tuple(t.cpu() for t in out()))
    # the C entry refuses another n_mean itself
    from pointvs_amd import _lib
    o = out()
    rc = _lib.lib().pvs_slot_node_values(_lib.ptr(y), 4, 0, 2, y.shape[0], _lib.ptr(node_ptr), _lib.ptr(lig_ptr), n_slots,
                                         N_REC, *[_lib.ptr(t) for t in o], None)
    assert rc != 0 and b'n_mean' in _lib.lib().pvs_last_error()
    PF.slot_node_values(y, node_ptr, lig_ptr, N_REC, out=out())


# ---------------------------------------------------------------- the sweep against the fp64 oracle

def _sweep(model, rec, rec_feats, capture, batch_size=3, **kw):
    from pointvs_amd.screening import ScreeningSweep
    return ScreeningSweep(model.cuda(), rec.cuda(), rec_feats, RADIUS, batch_size=batch_size, capture=capture, **kw)


def _check_map(out, want, bound, what, n_hits):
    count = out['count'].cpu().numpy()
    assert out['count'].dtype == torch.int32 and (count == n_hits).all() and np.array_equal(count, want['count'])
    assert out['per_hit'].shape == (len(want['per_hit']), len(count)) and out['mean'].dtype == torch.float64
    assert list(out['ligand']) == list(want['ligand'])
    for name, values in out['ligand'].items():
        _close(values.cpu().numpy(), want['ligand'][name], bound, f'{what} ligand {name}')
    _close(out['per_hit'].cpu().numpy(), want['per_hit'], bound, f'{what} per_hit')
    _close(out['mean'].cpu().numpy(), want['mean'], bound, f'{what} mean')
    _close(out['max'].cpu().numpy(), want['max'], bound, f'{what} max')


@pytest.mark.parametrize('capture', [pytest.param(True, marks=needs_caching_allocator), False], ids=['captured', 'eager'])
def test_parity_with_the_fp64_oracle(capture):
    """Hits of 1, 12, 12 and 70 atoms at batch 3 (the last batch is partly empty): the map, the ligand atoms' values
    and every hit's row against the fp64 oracle; every hit's mean CAM over its complex against the screen's own score."""
    y = ref.sweep_yardstick()
    want, bound = y['y64'], y['bound']
    print(f"max|cam64| {y['scale']:.4f} noise32 {y['noise32']:.3e} bound {bound:.3e} score bound {y['score_bound']:.3e}")
    sweep = _sweep(y['model'], y['rec'], y['rec_feats'], capture)
    out = sweep.receptor_hotspots(y['items'], attribution='cam', per_hit=True, gnn_layer=17)      # (gnn_layer: ignored)
    screen = sweep.cam_screen
    assert screen.cam is not None and screen._captured == capture and sweep.hotspot is None
    assert sweep.batches_run == 1 + 2                      # the sizing batch, then ceil(4 / 3) steps
    _check_map(out, want, bound, f'cam capture={capture}', 4)
    # the screen's own scores of the same hits, one step each way
    names = [name for name, _, _ in y['items']]
    scores = {}
    for k in range(0, 4, 3):
        screen.load([(f, p) for _, f, p in y['items'][k:k + 3]])
        raw = (screen.replay().clone() if capture else screen()).reshape(3, -1)
        scores.update({name: float(raw[i, 0]) for i, name in enumerate(names[k:k + 3])})
    for i, name in enumerate(names):
        values = np.concatenate([out['ligand'][name].cpu().numpy(), out['per_hit'][i].cpu().numpy()]).astype(np.float64)
        err = abs(values.mean() - scores[name])
        print(f'{name}: mean CAM {values.mean():.8f} score {scores[name]:.8f} err {err:.3e}')
        assert err <= bound + y['score_bound']
        assert abs(scores[name] - float(want['score'][name][0])) <= y['score_bound']


def test_parity_with_the_per_complex_route():
    """pointvs_amd.attribution.cam, one complex per call on the oracle's edge list, within twice the bound."""
    from oracle.generate_edges_oracle import generate_edges
    from pointvs_amd import attribution
    y = ref.sweep_yardstick()
    out = _sweep(y['model'], y['rec'], y['rec_feats'], False).receptor_hotspots(y['items'], attribution='cam', per_hit=True)
    model = y['model'].cuda()
    for i, (name, feats, pose) in enumerate(y['items']):
        pos, x = torch.cat([pose, y['rec']], 0), torch.cat([feats, y['rec_feats']], 0)
        _, (rows, cols), attrs = generate_edges(pos.numpy(), x[:, -1].numpy(), RADIUS, RADIUS, prune=False)
        one = attribution.cam(model, pos[None], x[None], edge_indices=torch.from_numpy(np.vstack([rows, cols])).long(),
                              edge_attrs=torch.nn.functional.one_hot(torch.from_numpy(attrs).long(), 3))
        got = np.concatenate([out['ligand'][name].cpu().numpy(), out['per_hit'][i].cpu().numpy()])
        _close(got, one.reshape(-1), 2 * y['bound'], f'attribution.cam {name}')


@needs_caching_allocator
def test_nothing_leaks_into_the_accumulators():
    """A fresh sweep: the sizing batch, the capture (two warm-up steps and the captured one), then the run; a second
    call on the same sweep gives the same bytes, and an eager sweep the same counts."""
    y = ref.sweep_yardstick()
    sweep = _sweep(y['model'], y['rec'], y['rec_feats'], True)
    first = sweep.receptor_hotspots(y['items'], attribution='cam', per_hit=True)
    screen = sweep.cam_screen
    assert sweep.batches_run == 3 and screen._captured
    again = sweep.receptor_hotspots(y['items'], attribution='cam', per_hit=True)
    assert sweep.cam_screen is screen and sweep.batches_run == 5
    assert bool((first['count'] == 4).all())
    for key in ('mean', 'count', 'max', 'per_hit'):
        assert first[key].cpu().numpy().tobytes() == again[key].cpu().numpy().tobytes(), key
    for name in first['ligand']:
        assert first['ligand'][name].cpu().numpy().tobytes() == again['ligand'][name].cpu().numpy().tobytes()
    # a column instead of the rule: another screen (True is not column 1); an item without atoms does not count
    sweep.receptor_hotspots(y['items'], attribution='cam', column=0)
    assert sweep.cam_screen is not screen and sweep.cam_screen.cam_request == 0
    name, feats, pose = y['items'][1]
    some = sweep.receptor_hotspots(y['items'][:2] + [('nothing', feats[:0], pose[:0])], attribution='cam', column=0,
                                   per_hit=True)
    assert bool((some['count'] == 2).all()) and bool(torch.isnan(some['per_hit'][2]).all())
    assert some['ligand']['nothing'].numel() == 0
    _close(some['per_hit'][:2].cpu().numpy(), y['y64']['per_hit'][:2], y['bound'], 'beside an empty item')
    none = sweep.receptor_hotspots([], attribution='cam', per_hit=True)
    assert bool(torch.isnan(none['mean']).all()) and not none['count'].any() and none['per_hit'].shape == (0, N_REC_SCREEN)


def _parity_of(model, cfg, items, rec, rec_feats, what, sweep_kw=None, oracle_kw=None, **call):
    want, scale, noise, bound, _ = ref.oracle_pair(model, cfg, items, rec, rec_feats, RADIUS, **(oracle_kw or {}))
    print(f'{what}: max|cam64| {scale:.4f} noise32 {noise:.3e} bound {bound:.3e}')
    sweep = _sweep(model, rec, rec_feats, **(sweep_kw or dict(capture=False)))
    out = sweep.receptor_hotspots(items, attribution='cam', per_hit=True, **call)
    _check_map(out, want, bound, what, len(items))
    return sweep, want, bound


def test_three_outputs_are_averaged():
    items, rec, rec_feats = hits_and_receptor()
    model = attention_model(33, dim_output=3)
    cfg = dict(KW, edge_attention=True, num_layers=3, dim_output=3, _class='SartorrasEGNN')
    sweep, want, bound = _parity_of(model, cfg, items, rec, rec_feats, 'three outputs', oracle_kw=dict(n_mean=3))
    assert sweep.cam_screen._cam_plan[2:] == (0, 3)
    # a column of the three instead
    _parity_of(model, cfg, items, rec, rec_feats, 'column 2 of three', oracle_kw=dict(column=2), column=2)


def test_two_headed_model_takes_a_column():
    from tests.test_gpu_two_head_screen import KW as KW2, _model
    items, rec, rec_feats = hits_and_receptor()
    flags = dict(k=32, num_layers=2, dim_output=3, final_softplus=True)
    model = _model(3, **flags)
    cfg = dict(KW2, **flags, _class='MultitaskSatorrasEGNN')
    for column in (0, 1):
        sweep, _, _ = _parity_of(model, cfg, items, rec, rec_feats, f'two heads, column {column}',
                                 sweep_kw=dict(capture=False, tasks='both'), oracle_kw=dict(column=column, tasks='both'),
                                 column=column)
        assert sweep.cam_screen.cam['node_y'].shape[1] == 4
    with pytest.raises(ValueError, match='name a column'):
        _sweep(model, rec, rec_feats, False, tasks='both').receptor_hotspots(items, attribution='cam')
    # the affinity head alone: three outputs, the rule averages them
    _parity_of(model, cfg, items, rec, rec_feats, 'affinity head', sweep_kw=dict(capture=False, tasks='affinity'),
               oracle_kw=dict(n_mean=3, tasks='affinity'))


def test_graphnorm_model_runs_one_hit_per_step_eager():
    items, rec, rec_feats = hits_and_receptor()
    items = items[:3]
    model = attention_model(32, graphnorm=True)
    cfg = dict(KW, edge_attention=True, num_layers=3, graphnorm=True, _class='SartorrasEGNN')
    sweep, _, _ = _parity_of(model, cfg, items, rec, rec_feats, 'graphnorm', sweep_kw=dict(capture=True, batch_size=1))
    assert sweep.cam_screen.graphnorm and not sweep.cam_screen._captured and sweep.batches_run == 1 + 3


def test_other_hidden_sizes_and_heads_take_the_plain_route():
    """k = 16 has no first-layer reuse: the plain route, eager, offsets from the host-known sizes. A multi_fc head is
    none that the fused kernels take: each of its layers per node on the linear op, then the same slot operator."""
    items, rec, rec_feats = hits_and_receptor()
    model = attention_model(34, k=16, edge_attention=False)
    cfg = dict(KW, num_layers=3, k=16, _class='SartorrasEGNN')
    sweep, _, _ = _parity_of(model, cfg, items, rec, rec_feats, 'k = 16', sweep_kw=dict(capture=True))
    assert not sweep.cam_screen.reuse and not sweep.cam_screen._captured and sweep.batches_run == 2
    model = attention_model(35, multi_fc=True, edge_attention=False)
    cfg = dict(KW, num_layers=3, multi_fc=True, _class='SartorrasEGNN')
    sweep, _, _ = _parity_of(model, cfg, items, rec, rec_feats, 'multi_fc')
    assert sweep.cam_screen.reuse and sweep.cam_screen.model._fused_head(model.feats_linear_layers) is None


@needs_caching_allocator
def test_end_to_end_after_run_library(tmp_path):
    from pointvs_amd.screening import ScreeningSweep
    lig, rec, lig_feats, rec_feats = _set(8102, 70)
    work = _library(lig, lig_feats)
    sweep = ScreeningSweep(attention_model(5, edge_attention=False).cuda(), rec.cuda(), rec_feats, edge_radius=RADIUS,
                           batch_size=4)
    sweep.run_library(work, hits_file=tmp_path / 'hits.txt')
    before = sweep.batches_run
    out = sweep.receptor_hotspots(sweep.best_poses(work), attribution='cam', scores_file=tmp_path / 'hotspots.txt',
                                  ligand_scores_file=tmp_path / 'ligand.txt')
    sizes = {'ligA': 12, 'ligB': 9, 'ligC': 70, 'ligD': 12, 'ligE': 1}
    assert sweep.batches_run - before == 1 + -(-len(sizes) // 4) and 'per_hit' not in out
    assert {name: int(v.shape[0]) for name, v in out['ligand'].items()} == sizes
    assert sweep.cam_screen.max_lig_atoms == 70 and sweep.cam_screen._captured and sweep.library.cam is None
    mean, count = out['mean'].cpu().numpy(), out['count'].cpu().numpy()
    assert (count == len(sizes)).all() and not np.isnan(mean).any()
    lines = (tmp_path / 'hotspots.txt').read_text().splitlines()
    assert len(lines) == N_REC_SCREEN
    for j, line in enumerate(lines):
        assert re.fullmatch(r'-?\d+\.\d{6} \d+ \| receptor atom\d+', line), line
        assert line == f'{mean[j]:.6f} {count[j]} | receptor atom{j}'
    lines = (tmp_path / 'ligand.txt').read_text().splitlines()
    want = [(name, a, float(out['ligand'][name][a])) for name in out['ligand'] for a in range(sizes[name])]
    assert len(lines) == sum(sizes.values())
    for line, (name, a, v) in zip(lines, want):
        assert re.fullmatch(r'-?\d+\.\d{6} \| receptor \w+_atom\d+', line), line
        assert line == f'{v:.6f} | receptor {name}_atom{a}'
    # the two attributions side by side on one sweep need an attention layer only for one of them
    with pytest.raises(ValueError, match='no edge attention'):
        sweep.receptor_hotspots(sweep.best_poses(work))


def test_a_screen_without_cam_is_the_screen_it_was():
    """cam=None: no buffer, no launch of the two operators (their profile counters stay out of a step), the same bytes
    as a screen with cam on beside it."""
    from pointvs_amd.screening import LibraryScreen
    items, rec, rec_feats = hits_and_receptor()
    model = attention_model(31).cuda()
    slots = [(f, p) for _, f, p in items[:3]]
    plain = LibraryScreen(model, rec.cuda(), rec_feats, 3, 70, RADIUS)
    with_cam = LibraryScreen(model, rec.cuda(), rec_feats, 3, 70, RADIUS, cam=True, contact_attention=1)
    assert plain.cam is None and plain._cam_plan is None and plain._h_final is None
    a, b = plain(slots), with_cam(slots)
    assert plain._h_final is None and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()
    assert bool((with_cam.cam['rec_count'] == 3).all()) and int(with_cam.contact['rec_count'].sum()) > 0
    with pytest.raises(RuntimeError, match='without cam'):
        plain.reset_cam()
    with_cam.reset_cam()
    assert not with_cam.cam['rec_count'].any() and bool(torch.isnan(with_cam.cam['rec_max']).all())


def test_errors():
    from pointvs_amd.screening import ScreeningSweep
    items, rec, rec_feats = hits_and_receptor()
    item = items[1]
    sweep = _sweep(attention_model(6), rec, rec_feats, False)
    with pytest.raises(ValueError, match="attribution='nonsense'"):
        sweep.receptor_hotspots([item], attribution='nonsense')
    with pytest.raises(ValueError, match='column 1 of 1 outputs'):
        sweep.receptor_hotspots([item], attribution='cam', column=1)
    with pytest.raises(ValueError, match='column -1 of 1 outputs'):
        sweep.receptor_hotspots([item], attribution='cam', column=-1)
    with pytest.raises(ValueError, match="column selects a head output of attribution='cam'"):
        sweep.receptor_hotspots([item], column=0)
    with pytest.raises(NotImplementedError, match='fp32 only'):
        ScreeningSweep(attention_model(6).double().cuda(), rec.cuda().double(), rec_feats.double(), edge_radius=RADIUS,
                       batch_size=3).receptor_hotspots([item], attribution='cam')
    with pytest.raises(ValueError, match='receptor_hotspots: names must be unique'):
        sweep.receptor_hotspots([item, item], attribution='cam')
    assert list(sweep.receptor_hotspots([item], attribution='cam')['ligand']) == ['hitA']      # (still usable)
