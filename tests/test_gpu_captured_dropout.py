"""Edge dropout with a fixed-shape edge list, and captured training with it (train_model(capture=True), dropout > 0).

pvs_dropout_adj_mark_dev / pvs_dropout_adj_fill_padded (pointvs_amd/csrc/dropout_adj.hip) against the padded host
reference tests/_dropout_padded_ref.py, element for element (the draw is integer: every comparison of a list is exact;
the reference is pinned without a GPU in tests/test_dropout_padded_host.py). On top of the operator: the prepared graph
of the padded list against that of the eager draw, one training step with `static_dropout` against the fp64 oracle on
the list that was drawn over the batch's real nodes (tests/_golden.assert_strict - the padding is inert), the replayed
steps' masks against the eager schedule's, captured runs against the same runs taken eagerly (torch.equal), and the
limits (GraphNorm, fp64, the switch left off).
"""
import numpy as np
import pytest
import torch

from tests._dropout_padded_ref import dropout_adj_padded_ref, half_count
from tests._dropout_ref import SEED_STEPS, dropout_adj_ref
from tests._golden import CaseLog, assert_strict, grad_floor, needs_caching_allocator
from tests.test_gpu_edge_dropout import (FULL, RADIUS, _attr, _edge_list, _forty_candidates, _gpu,
                                         _iteration_that_keeps_nothing, _model, _one_small_graph, _references, _restart,
                                         _training_step, _two_graphs)

pytestmark = pytest.mark.gpu
POISON = -7


def _two_graph_lists():
    b = _two_graphs()
    return b.edge_index.numpy(), b.edge_attr.numpy(), int(b.x.size(0))


def _check_padded(ei, ea, p, seed, step, n_nodes, n_pad, cap=None, table=None, out=None, what=''):
    """One PF.dropout_adj_padded call against the reference: arrays and n_kept exact. Returns K."""
    from pointvs_amd import functional as PF
    cap = 2 * half_count(ei) if cap is None else cap
    if table is None:
        table = PF.dropout_key_table('cuda', seed, step)
    else:
        PF.write_dropout_key(table, seed, step)
    oi, oa, kept = PF.dropout_adj_padded(_gpu(ei), _gpu(ea), p, table, cap, n_nodes, n_pad, out=out)
    ref_i, ref_a, k = dropout_adj_padded_ref(ei, ea, p, seed, step, cap, n_nodes, n_pad)
    what = (what, seed, step, p)
    assert oi.dtype == torch.int64 and oi.is_cuda and tuple(oi.shape) == (2, cap), what
    assert kept.dtype == torch.int32 and kept.is_cuda and int(kept) == k, (what, int(kept), k)
    assert torch.equal(oi.cpu(), torch.from_numpy(ref_i)), what
    if ea is None:
        assert oa is None, what
    else:
        assert oa.dtype == torch.int64 and tuple(oa.shape) == ref_a.shape and torch.equal(oa.cpu(), torch.from_numpy(ref_a)), what
    if out is not None:
        assert oi is out[0] and oa is out[1]
    return k


# ---- 1. the fill, exactly --------------------------------------------------------------------------------------------
def test_padded_draw_of_the_two_graph_batch_equals_the_reference():
    """Every (seed, step) of SEED_STEPS (two differ in one 32-bit half only: the key is read from the device table) at
    p = 0.25, at 1e-9 (no dead slot) and at 0.999 (next to nothing survives; the third pair keeps nothing at all)."""
    from pointvs_amd.functional import static_dropout_plan
    ei, ea, n_nodes = _two_graph_lists()
    assert (n_nodes, ei.shape[1], half_count(ei)) == (207, 2470, 1235)
    kept = {}
    for p in (0.25, 1e-9, 0.999):
        cap, n_pad = static_dropout_plan(n_nodes, half_count(ei), p)
        kept[p] = [_check_padded(ei, ea, p, seed, step, n_nodes, n_pad, cap) for seed, step in SEED_STEPS]
    assert kept[0.25][:3] == [931, 919, 945] and kept[1e-9] == [1235] * 6 and kept[0.999][:3] == [1, 2, 0]
    assert len(set(kept[0.25])) > 3


def test_padded_draw_of_the_small_graph_equals_the_reference():
    ei = _forty_candidates()
    ea = np.eye(3, dtype=np.int64)[ei[0] % 3]
    for p, n_pad in ((0.25, 8), (0.999, 30)):
        for seed, step in SEED_STEPS:
            assert _check_padded(ei, ea, p, seed, step, 30, n_pad) <= 40


def _pairs_and_reverses(n_half):
    """n_half candidates (i, i + 1 + i % 3) with their reverses in between: E = cap = 2 n_half."""
    lo = np.arange(n_half, dtype=np.int64)
    hi = lo + 1 + lo % 3
    ei = np.empty((2, 2 * n_half), dtype=np.int64)
    ei[:, 0::2] = np.stack([lo, hi])
    ei[:, 1::2] = np.stack([hi, lo])
    return ei


@pytest.mark.parametrize('n_half', [255, 256, 257])
def test_launch_edges_of_the_fill(n_half):
    """cap = 512 +- 2 around two blocks of 256; both orders of max(E, cap): the list with its reverses (E = cap) and the
    candidates alone (cap = 2 E: the fill runs past E)."""
    ei = _pairs_and_reverses(n_half)
    ea5 = _edge_list(600)[1]
    n_nodes = n_half + 3
    for edges in (ei, ei[:, 0::2]):
        assert half_count(edges) == n_half
        for width in (None, 3):
            ea = _attr(ea5[:edges.shape[1]], width)
            for (seed, step), p in zip(SEED_STEPS[:4], (0.25, 0.999, 1e-9, 0.5)):
                _check_padded(edges, ea, p, seed, step, n_nodes, 6, what=(n_half, edges.shape[1], width))


def test_candidates_only_self_loops_and_no_attributes():
    ei, ea5 = _edge_list(513)
    up = np.sort(ei, axis=0)                       # every edge has row <= col: cap = 2 E
    loops = np.stack([ei[0], ei[0]])
    seed, step = SEED_STEPS[1]
    for edges, name in ((up, 'row <= col only'), (loops, 'self-loops'), (ei, 'mixed')):
        for ea in (None, _attr(ea5, 3), _attr(ea5, 1)):
            k = _check_padded(edges, ea, 0.5, seed, step, 1000, 4, what=name)
            assert 0 < 2 * k < 2 * half_count(edges)
    assert half_count(up) == 513 and half_count(loops) == 513 and half_count(ei) < 513


def test_rewriting_the_table_redraws_into_the_same_buffers():
    """The same call on the same output buffers after the table was rewritten gives the new key's list: nothing of the
    earlier draw is left behind (a longer draw, then one that keeps nothing - every slot padding - then a shorter)."""
    from pointvs_amd import functional as PF
    ei, ea, n_nodes = _two_graph_lists()
    cap, n_pad = PF.static_dropout_plan(n_nodes, half_count(ei), 0.25)
    table = PF.dropout_key_table('cuda')
    out = (torch.full((2, cap), POISON, dtype=torch.int64, device='cuda'),
           torch.full((cap, 3), POISON, dtype=torch.int64, device='cuda'))
    counts = [_check_padded(ei, ea, 0.25, seed, step, n_nodes, n_pad, cap, table=table, out=out) for seed, step in SEED_STEPS]
    assert len(set(counts)) > 3
    counts = [_check_padded(ei, ea, 0.999, seed, step, n_nodes, n_pad, cap, table=table, out=out) for seed, step in SEED_STEPS[:3]]
    assert counts == [1, 2, 0]
    assert int(out[0].min()) >= n_nodes, 'the draw that keeps nothing leaves padding edges only'
    _check_padded(ei, ea, 0.25, *SEED_STEPS[0], n_nodes, n_pad, cap, table=table, out=out)
    # the table is read when the kernels run: written on a stream, drawn on that stream, no host round trip in between
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _check_padded(ei, ea, 0.25, *SEED_STEPS[4], n_nodes, n_pad, cap, table=table, out=out)


def test_empty_lists_capacities_above_the_bound_and_what_is_refused():
    from pointvs_amd import functional as PF
    ei, ea5 = _edge_list(300)
    ea = _attr(ea5, 3)
    empty = np.zeros((2, 0), dtype=np.int64)
    for cap in (0, 4):
        assert _check_padded(empty, np.zeros((0, 3), dtype=np.int64), 0.3, 5, 1, 10, 2, cap) == 0
        assert _check_padded(empty, None, 0.3, 5, 1, 10, 2, cap) == 0
    down = np.stack([np.maximum(ei[0], ei[1]) + 1, np.minimum(ei[0], ei[1])])      # no candidate: cap = 0
    assert _check_padded(down, ea, 0.3, 5, 1, 1001, 2) == 0
    assert _check_padded(down, ea, 0.3, 5, 1, 1001, 4, cap=10) == 0
    _check_padded(ei, ea, 0.3, 5, 1, 1000, 4, cap=2 * half_count(ei) + 6)
    # a capacity below the draw: nothing is written, and n_kept tells
    table = PF.dropout_key_table('cuda', 5, 1)
    out = (torch.full((2, 4), POISON, dtype=torch.int64, device='cuda'), torch.full((4, 3), POISON, dtype=torch.int64, device='cuda'))
    _, _, kept = PF.dropout_adj_padded(_gpu(ei), _gpu(ea), 0.3, table, 4, 1000, 2, out=out)
    assert 2 * int(kept) > 4 and bool((out[0] == POISON).all()) and bool((out[1] == POISON).all())
    for bad in (dict(cap=3), dict(n_pad=3), dict(n_pad=0), dict(p=1.0), dict(cap=-2)):
        kw = dict(dict(p=0.3, cap=600, n_pad=2), **bad)
        with pytest.raises(ValueError):
            PF.dropout_adj_padded(_gpu(ei), _gpu(ea), kw['p'], table, kw['cap'], 1000, kw['n_pad'])
    with pytest.raises(ValueError):
        PF.dropout_adj_padded(_gpu(ei), _gpu(ea), 0.3, table, 600, 1000, 2, out=(out[0], out[1]))


# ---- 2. the prepared graph of the padded list ------------------------------------------------------------------------
@pytest.mark.parametrize('p', [0.25, 0.999])
def test_prepared_graph_of_the_padded_list_is_that_of_the_dropped_list_on_the_real_nodes(p):
    from pointvs_amd import functional as PF
    from pointvs_amd.graph import prepare_graph
    ei, ea, n_nodes = _two_graph_lists()
    cap, n_pad = PF.static_dropout_plan(n_nodes, half_count(ei), p)
    for seed, step in SEED_STEPS[:2]:
        oi, oa, kept = PF.dropout_adj_padded(_gpu(ei), _gpu(ea), p, PF.dropout_key_table('cuda', seed, step), cap, n_nodes, n_pad)
        padded = prepare_graph(oi, oa, n_nodes + n_pad, need_backward=True)
        di, da = PF.dropout_adj(_gpu(ei), _gpu(ea), p, training=True, seed=seed, step=step)
        plain = prepare_graph(di, da, n_nodes, need_backward=True)
        padded.check_status()
        plain.check_status()
        two_k = 2 * int(kept)
        assert two_k == plain.n_edges and padded.n_edges == cap and 0 < two_k < cap
        for name in ('rowptr', 'colptr'):
            assert torch.equal(padded.t[name][:n_nodes + 1], plain.t[name]), name
            assert int(padded.t[name][n_nodes]) == two_k and int(padded.t[name][-1]) == cap
        for name in ('row', 'col', 'etype', 'perm', 'cedge'):      # (real columns come first: their CSC entries too)
            assert torch.equal(padded.t[name][:two_k], plain.t[name][:two_k]), name
        assert torch.equal(padded.t['inv_deg'][:n_nodes], plain.t['inv_deg'])
        assert int(padded.t['row'][two_k:].min()) >= n_nodes and int(padded.t['col'][two_k:].min()) >= n_nodes
        # a padding row holds about the mean degree of the batch (static_dropout_plan's reason), never the lot
        pad_deg = (padded.t['rowptr'][n_nodes + 1:] - padded.t['rowptr'][n_nodes:-1]).cpu().numpy()
        assert pad_deg.sum() == cap - two_k and pad_deg.max() - pad_deg.min() <= 1


# ---- 3. one training step with the switch on, against the oracle on the drawn list -----------------------------------
def _check_last_dropout(model, edges, attr, p, n_nodes):
    """model.last_dropout against the padded reference for the key it names. Returns (seed, step, K)."""
    last = model.last_dropout
    ref_i, ref_a, k = dropout_adj_padded_ref(edges, attr, p, last['seed'], last['step'], last['cap'], n_nodes, last['n_pad'])
    assert int(last['n_kept']) == k
    assert torch.equal(last['out_index'].cpu(), torch.from_numpy(ref_i)) and torch.equal(last['out_attr'].cpu(), torch.from_numpy(ref_a))
    return last['seed'], last['step'], k


def _check_step_against_the_oracle(got, model_sd, cfg, host, drawn_i, drawn_a, case):
    ref64, ref32 = _references(model_sd, cfg, host, drawn_i, drawn_a)
    floor = grad_floor({k: v for k, v in ref64.items() if k.startswith('grad ')})
    log = CaseLog(case)
    for key, ref in ref64.items():
        if key == 'edge messages':
            continue
        if got[key] is None or ref is None:     # no gradient at all where the oracle has none, or exact zeros
            assert (got[key] is None or not bool(got[key].any())) and (ref is None or not ref.any()), key
            continue
        value = got[key].detach().cpu().numpy()
        assert value.dtype == np.float32 and value.size == ref.size, key
        assert_strict(value.reshape(ref.shape), ref, [r[key] for r in ref32], f'{log.case} {key}',
                      floor=floor if key.startswith('grad ') else 0.0, log=log)
    log.finish()


def _built(dev):
    from pointvs_amd.radius_graph import attach_radius_graph
    pg = attach_radius_graph(dev, RADIUS).prepared
    pg.check_status()
    e = pg.n_edges
    edges = np.stack([pg.t['row'][:e].cpu().numpy(), pg.t['col'][:e].cpu().numpy()]).astype(np.int64)
    return edges, np.eye(pg.n_edge_attr, dtype=np.int64)[pg.t['etype'][:e].cpu().numpy()]


@pytest.mark.parametrize('flags,way', [('defaults', 'coo'), ('full', 'coo'), ('full', 'built'), ('multitask', 'coo')])
def test_static_dropout_step_equals_the_oracle_on_the_drawn_list(flags, way, tmp_path):
    """Logits, loss and every parameter gradient of a training-mode forward + backward with static_dropout on, against
    the oracle on dropout_adj_ref's list for the recorded key over the N real nodes: the padding is inert."""
    if flags == 'multitask':
        from pointvs_amd.egnn_multitask import MultitaskSatorrasEGNN
        kw = dict(dim_input=12, k=32, dim_output=1, num_layers=2, dropout=0.25, graphnorm=False, edge_attention=True,
                  edge_attention_final_only=True)
        torch.manual_seed(3)
        model = MultitaskSatorrasEGNN(tmp_path, 2e-3, 1e-4, None, None, silent=True, **kw).cuda().train()
        cfg = dict(kw, _class='MultitaskSatorrasEGNN')
    else:
        model, cfg = _model(tmp_path, graphnorm=False, **(FULL if flags == 'full' else {}))
    host, dev = _two_graphs(), _two_graphs().to('cuda')
    if way == 'built':
        edges, attr = _built(dev)
        assert dev.prepared is not None
    else:
        edges, attr = dev.edge_index.cpu().numpy(), dev.edge_attr.cpu().numpy()
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    model.static_dropout = True
    _restart(model, seed=21, global_iter=5)
    got = _training_step(model, dev)
    seed, step, k = _check_last_dropout(model, edges, attr, 0.25, 207)
    from pointvs_amd.egnn_satorras import _mix64
    assert (seed, step) == (21, _mix64(_mix64(5) + 1)) and model.last_dropout['cap'] == 2 * half_count(edges)
    assert model.last_dropout['n_pad'] == 52 and 0 < 2 * k < model.last_dropout['cap']
    assert tuple(got['logits'].shape) == (2,)
    drawn_i, drawn_a = dropout_adj_ref(edges, attr, 0.25, seed, step)
    _check_step_against_the_oracle(got, sd, cfg, host, drawn_i, drawn_a, f'static-dropout-{flags}-{way}')
    # the next step draws at the next key; eval mode does not draw
    model.global_iter += 1
    _training_step(model, dev)
    assert _check_last_dropout(model, edges, attr, 0.25, 207)[1] == _mix64(_mix64(6) + 1) != step
    was = dict(model.last_dropout)
    model.eval()
    with torch.no_grad():
        model(dev)
    assert model.last_dropout['step'] == was['step']


def test_static_dropout_step_that_keeps_nothing_equals_the_oracle_on_the_empty_list(tmp_path):
    model, cfg = _model(tmp_path, dropout=0.999, graphnorm=False, **FULL)
    host, dev = _one_small_graph(), _one_small_graph().to('cuda')
    edges, attr = dev.edge_index.cpu().numpy(), dev.edge_attr.cpu().numpy()
    global_iter, steps = _iteration_that_keeps_nothing(edges, 21, 0.999)
    assert global_iter == 0
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    model.static_dropout = True
    _restart(model, seed=21, global_iter=global_iter)
    got = _training_step(model, dev)
    seed, step, k = _check_last_dropout(model, edges, attr, 0.999, 30)
    assert (seed, step, k) == (21, steps[0], 0) and (model.last_dropout['cap'], model.last_dropout['n_pad']) == (80, 30)
    assert int(model.last_dropout['out_index'].min()) >= 30
    _check_step_against_the_oracle(got, sd, cfg, host, np.zeros((2, 0), dtype=np.int64), np.zeros((0, 3), dtype=np.int64),
                                   'static-dropout-kept0')


# ---- 4. / 5. captured training ---------------------------------------------------------------------------------------
class _CheckingLoader(list):
    """Resident batches; before handing the next one out, checks the step just taken: model.last_dropout against the
    reference for the key the eager schedule gives at that step."""

    def __init__(self, batches, model, p, seed):
        super().__init__(batches)
        self.model, self.p, self.seed, self.drawn = model, p, seed, []

    def _check(self, batch, global_iter):
        from pointvs_amd.egnn_satorras import _mix64
        edges, attr = batch.edge_index.cpu().numpy(), batch.edge_attr.cpu().numpy()
        seed, step, k = _check_last_dropout(self.model, edges, attr, self.p, int(batch.x.size(0)))
        base = ((self.model.p_epoch + self.model.a_epoch) << 24) + global_iter
        assert (seed, step) == (self.seed, _mix64(_mix64(base) + 1)), (global_iter, seed, step)
        self.drawn.append((id(batch), dict(self.model.last_capture_stats), self.model.last_dropout['out_index'].cpu().numpy().tobytes()))

    def __iter__(self):
        for b in list.__iter__(self):
            at = self.model.global_iter
            yield b
            self._check(b, at)


def _batches():
    b0 = _two_graphs().to('cuda')
    b1 = _one_small_graph().to('cuda')
    b1.edge_attr = b1.edge_attr.long()
    return [b0, b1]


@needs_caching_allocator
def test_captured_training_with_edge_dropout_draws_the_eager_schedules_masks(tmp_path):
    model, _ = _model(tmp_path, graphnorm=False)
    loader = _CheckingLoader(_batches() * 4, model, 0.25, 77)
    _restart(model, seed=77)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    losses = [float(v) for v in model.train_model(loader, epochs=1, capture=True)]
    stats = model.last_capture_stats
    assert stats == {'eager': 2, 'captured': 2, 'replayed': 4} and len(losses) == 8 and np.isfinite(losses).all()
    assert len(loader.drawn) == 8 and model.global_iter == 8
    replayed = [d for d in loader.drawn if d[1]['replayed'] > 0]
    assert len(replayed) == 4
    for batch in loader[:2]:      # consecutive replays of the same batch draw different masks
        lists = [d[2] for d in loader.drawn if d[0] == id(batch)]
        assert len(lists) == 4 and len(set(lists)) == 4
    assert any(not torch.equal(p, before[n]) for n, p in model.named_parameters())
    assert model.__dict__.get('static_dropout') is None and not model.dropout_keys.is_external
    assert not torch.cuda.is_current_stream_capturing()


def _run(tmp_path, capture, static, optimiser='adam', use_1cycle=False, epochs=1, repeats=4):
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    kw = dict(dim_input=12, k=32, dim_output=1, num_layers=2, dropout=0.25, graphnorm=False, edge_attention=True)
    torch.manual_seed(3)
    model = SartorrasEGNN(tmp_path, 2e-3, 1e-4, None, None, silent=True, optimiser=optimiser, use_1cycle=use_1cycle,
                          **kw).cuda().train()
    if static is not None:
        model.static_dropout = static
    _restart(model, seed=77)
    losses = model.train_model(_batches() * repeats, epochs=epochs, capture=capture)
    return model, torch.tensor(losses), (dict(model.last_capture_stats) if capture else None)


@needs_caching_allocator
@pytest.mark.parametrize('optimiser,use_1cycle', [('adam', False), ('sgd', False), ('adam', True)])
def test_captured_run_equals_the_eager_static_run_bit_for_bit(optimiser, use_1cycle, tmp_path):
    eager, eager_losses, _ = _run(tmp_path / 'eager', False, True, optimiser, use_1cycle)
    captured, losses, stats = _run(tmp_path / 'captured', True, None, optimiser, use_1cycle)
    assert stats['captured'] == 2 and stats['replayed'] == 4, stats
    diff = (losses - eager_losses).abs().max()
    print(f'{optimiser} 1cycle={use_1cycle}: captured vs eager static losses, max |difference| {float(diff):.3e}')
    worst = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(captured.parameters(), eager.parameters()))
    print(f'{optimiser} 1cycle={use_1cycle}: captured vs eager static parameters, max |difference| {worst:.3e}')
    assert torch.equal(losses, eager_losses), (losses.tolist(), eager_losses.tolist())
    for (name, p), q in zip(captured.named_parameters(), eager.parameters()):
        assert torch.equal(p, q), name
    if optimiser == 'adam' and not use_1cycle:      # a second captured run repeats the first
        again, again_losses, again_stats = _run(tmp_path / 'again', True, None, optimiser, use_1cycle)
        assert again_stats == stats and torch.equal(again_losses, losses)
        assert all(torch.equal(p, q) for p, q in zip(again.parameters(), captured.parameters()))


@needs_caching_allocator
def test_captured_multitask_run_equals_its_eager_static_run(tmp_path):
    from pointvs_amd.egnn_multitask import MultitaskSatorrasEGNN
    runs = []
    for capture in (False, True):
        torch.manual_seed(3)
        model = MultitaskSatorrasEGNN(tmp_path / str(capture), 2e-3, 1e-4, None, None, silent=True, dim_input=12, k=32,
                                      dim_output=1, num_layers=2, dropout=0.25, graphnorm=False).cuda().train()
        model.static_dropout = None if capture else True
        _restart(model, seed=77)
        losses = torch.tensor(model.train_model(_batches() * 3, epochs=1, capture=capture))
        runs.append((model, losses))
    assert runs[1][0].last_capture_stats == {'eager': 2, 'captured': 2, 'replayed': 2}
    assert torch.equal(runs[0][1], runs[1][1]), (runs[0][1].tolist(), runs[1][1].tolist())
    assert all(torch.equal(p, q) for p, q in zip(runs[0][0].parameters(), runs[1][0].parameters()))


# ---- 6. limits -------------------------------------------------------------------------------------------------------
def test_graphnorm_models_with_dropout_are_refused_before_any_step(tmp_path):
    model, _ = _model(tmp_path, graphnorm=True)
    batch = _two_graphs().to('cuda')
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    with pytest.raises(NotImplementedError, match=r'dropout.*GraphNorm'):
        model.train_model([batch, batch, batch], epochs=1, capture=True)
    assert not torch.cuda.is_current_stream_capturing()
    assert not any((getattr(model, 'last_capture_stats', None) or {}).values())
    assert model.global_iter == 0 and all(torch.equal(p, before[n]) for n, p in model.named_parameters())
    assert model.__dict__.get('static_dropout') is None
    # without dropout the same GraphNorm model is captured as before
    plain, _ = _model(tmp_path, dropout=0.0, graphnorm=True)
    assert len(plain.train_model([batch, batch, batch], epochs=1, capture=True)) == 3
    assert plain.last_capture_stats == {'eager': 1, 'captured': 1, 'replayed': 1}


def test_fp64_models_keep_their_refusal(tmp_path):
    model, _ = _model(tmp_path, graphnorm=False)
    model = model.double()
    batch = _two_graphs().to('cuda')
    with pytest.raises(NotImplementedError, match='fp32 only'):
        model.train_model([batch, batch], epochs=1, capture=True)
    assert model.__dict__.get('static_dropout') is None and not torch.cuda.is_current_stream_capturing()


def test_multi_process_keeps_its_refusal(tmp_path, monkeypatch):
    model, _ = _model(tmp_path, graphnorm=False)
    monkeypatch.setattr(torch.distributed, 'is_initialized', lambda: True)
    monkeypatch.setattr(torch.distributed, 'get_world_size', lambda *a, **k: 2)
    with pytest.raises(NotImplementedError, match='single-process'):
        model.train_model([_two_graphs().to('cuda')] * 2, epochs=1, capture=True)


def test_with_the_switch_off_nothing_changes(tmp_path):
    """Two fresh models, the switch unset and set to False: one eager dropout step, losses and gradients torch.equal;
    neither touches the static path (no last_dropout, no plan on the batch)."""
    steps = []
    for switch in (None, False):
        model, _ = _model(tmp_path, graphnorm=False, **FULL)
        if switch is not None:
            model.static_dropout = switch
        dev = _two_graphs().to('cuda')
        _restart(model, seed=21, global_iter=5)
        steps.append(_training_step(model, dev))
        assert 'last_dropout' not in model.__dict__ and '_pvs_static_dropout' not in dev.__dict__
    for key, value in steps[0].items():
        other = steps[1][key]
        assert (value is None and other is None) or torch.equal(value, other), key


def test_the_switch_refuses_a_graphnorm_model_on_the_eager_path_too(tmp_path):
    """static_dropout = True on a GraphNorm model would normalise over the padding rows: the step raises, and the same
    model with the switch off takes the eager draw as before."""
    model, _ = _model(tmp_path, graphnorm=True)
    dev = _two_graphs().to('cuda')
    model.static_dropout = True
    _restart(model, seed=21, global_iter=5)
    with pytest.raises(NotImplementedError, match='GraphNorm'):
        _training_step(model, dev)
    assert 'last_dropout' not in model.__dict__
    model.static_dropout = None
    assert torch.isfinite(_training_step(model, dev)['loss'])


def test_one_key_serves_one_forward_when_a_replayer_writes_the_keys(tmp_path):
    model, _ = _model(tmp_path, graphnorm=False)
    dev = _two_graphs().to('cuda')
    _restart(model, seed=21, global_iter=5)
    with model.dropout_keys.external(model):
        assert model.static_dropout is True
        model.push_dropout_key(dev.x.device)
        _training_step(model, dev)
        with pytest.raises(RuntimeError, match='second training forward'):
            _training_step(model, dev)
        model.push_dropout_key(dev.x.device)
        _training_step(model, dev)
    from pointvs_amd.egnn_satorras import _mix64
    assert model.last_dropout['step'] == _mix64(_mix64(5) + 2)


@needs_caching_allocator
def test_the_plan_is_made_ahead_of_the_step_and_lives_with_the_captured_graph(tmp_path):
    """_make_capturable leaves the plan (the one host read) on the batch; a batch of one graph carries its own [0, N]
    offsets there, the pooling shortcut reads THAT tensor, and the replayer's entry keeps the plan alive - nothing a
    captured step reads belongs to a cache that could drop it."""
    from pointvs_amd.pnn_geometric_base import PNNGeometricBase
    from pointvs_amd.captured_step import StepReplayer
    model, _ = _model(tmp_path, graphnorm=False)
    two, one = _batches()
    model.static_dropout = True
    StepReplayer._make_capturable(two, model)
    StepReplayer._make_capturable(one, model)
    plan2, plan1 = two.__dict__['_pvs_static_dropout'], one.__dict__['_pvs_static_dropout']
    assert (plan2['n_half'], plan2['cap'], plan2['n_pad'], plan2['whole']) == (1235, 2470, 52, None)
    assert (plan1['n_half'], plan1['cap'], plan1['n_pad']) == (40, 80, 8) and plan1['whole'].tolist() == [0, 30]
    feats = torch.zeros(30, 4, device='cuda')
    assert PNNGeometricBase._whole_ptr(feats, plan1['whole']) is plan1['whole']
    for other in (plan1['node_ptr'], None, plan2['node_ptr']):
        fresh = PNNGeometricBase._whole_ptr(feats, other)
        assert fresh is not plan1['whole'] and fresh.tolist() == [0, 30] and fresh.dtype == torch.int32
    assert PNNGeometricBase._whole_ptr(feats[:20], plan1['whole']).tolist() == [0, 20]
    model.static_dropout = None
    _restart(model, seed=77)
    with StepReplayer(model) as replayer, torch.cuda.stream(replayer.stream):
        for _ in range(3):
            for batch in (two, one):
                replayer.step(batch)
            model.global_iter += 1
        assert replayer.stats == {'eager': 2, 'captured': 2, 'replayed': 2}
        entries = {id(e.batch): e for e in replayer.graphs.values()}
        assert entries[id(one)].plan is plan1 and entries[id(two)].plan is plan2
        assert one.__dict__['_pvs_static_dropout'] is plan1, 'the visits reuse the plan made ahead of them'


@needs_caching_allocator
def test_a_step_that_raises_leaves_model_and_optimiser_as_before_the_run(tmp_path):
    """The loader's fifth item is a batch without `y`: unpack_input_data_and_predict raises AttributeError on its first
    line, before any launch, in the eager visit of a run that has two captured graphs. The replayer's windows close on
    the way out, and the next captured run is an ordinary one."""
    import copy
    model, _ = _model(tmp_path, graphnorm=False)
    good = _batches()
    broken = copy.copy(good[0])
    del broken.y
    _restart(model, seed=77)
    flags = [g.get('capturable', False) for g in model.optimiser.param_groups]
    assert not any(flags) and model.optimiser_window is None
    with pytest.raises(AttributeError, match="'y'"):
        model.train_model(good * 2 + [broken], epochs=1, capture=True)
    assert model.last_capture_stats == {'eager': 3, 'captured': 2, 'replayed': 0} and model.global_iter == 4
    assert [g.get('capturable', False) for g in model.optimiser.param_groups] == flags
    counters = [st['step'] for st in model.optimiser.state.values()]
    assert counters and all(not c.is_cuda and c.dtype == torch.float32 and float(c) == 4.0 for c in counters)
    assert 'static_dropout' not in model.__dict__ and not model.dropout_keys.is_external
    assert model.optimiser_window is None
    assert not torch.cuda.is_current_stream_capturing()
    losses = model.train_model(good * 3, epochs=1, capture=True)
    assert model.last_capture_stats == {'eager': 2, 'captured': 2, 'replayed': 2}
    assert len(losses) == 6 and np.isfinite([float(v) for v in losses]).all()
