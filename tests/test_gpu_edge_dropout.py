"""Edge dropout (dropout > 0 in training mode): k_dropout_mark, the hipcub scan and k_dropout_fill of
pointvs_amd/csrc/dropout_adj.hip against the host reference tests/_dropout_ref.py, element for element.

The draw is counter-based and integer, so every comparison of an edge list is exact (torch.equal / np.array_equal).
The reference itself is pinned without a GPU in tests/test_dropout_ref_host.py. On top of the operator: the raw entry
points' refusals, the model's (seed, step) schedule, the dropped training step against the fp64 oracle on the list that
was drawn (tests/_golden.assert_strict; fp64 model: the bound of tests/test_gpu_fp64.py), and the refusal of captured
training with edge dropout.
"""
import functools
import types

import numpy as np
import pytest
import torch

from tests._dropout_ref import MAX_DRAW, SEED_STEPS, ZERO_DRAW, dropout_adj_ref, uniform24
from tests._golden import CaseLog, assert_strict, edge_permutations, grad_floor

pytestmark = pytest.mark.gpu

# (7, 7), (7, 7 + 2**32), (7 + 2**32, 7), (7 + 2**32, 7 + 2**32): equal low words, one or both high words set
SEED_STEPS_GPU = SEED_STEPS + [(0, 0), (7 + 2 ** 32, 7 + 2 ** 32)]
PROBS = [0.3, 0.5, 2.0 ** -24, 0.999]
SIZES = [1, 2, 255, 256, 257, 511, 512, 513, 4095, 4096, 4097, 100003]
BOUNDARY = (255, 256, 257)       # the sentinel thread E is the last of its block / alone in the next one
WIDTHS = [None, 1, 3, 5]


@functools.lru_cache(maxsize=None)
def _edge_list(n_edges, lo=0, hi=1000):
    """Random int64 list with both orientations, duplicate edges and self-loops; every attribute row names its edge in
    column 0 (magnitude above 2**33, alternating sign), the other columns are random 41-bit values of either sign."""
    rng = np.random.default_rng(1000 + n_edges)
    ei = rng.integers(lo, hi, size=(2, n_edges), dtype=np.int64)
    if n_edges >= 8:
        ei[:, 1::7] = ei[:, 0::7][:, :ei[:, 1::7].shape[1]]        # duplicates of the edge before
        ei[1, 3::11] = ei[0, 3::11]                                # self-loops
        ei[:, 5::13] = ei[::-1, 4::13][:, :ei[:, 5::13].shape[1]]  # the reverse of the edge before
    else:
        ei = np.sort(ei, axis=0)                                   # one or two edges: candidates (row <= col), ...
        ei[:, 1:] = ei[::-1, 1:]                                   # ... the second one the other way round
    ea = rng.integers(-2 ** 40, 2 ** 40, size=(n_edges, 5), dtype=np.int64)
    ea[:, 0] = (np.arange(n_edges) + 2 ** 33) * (1 - 2 * (np.arange(n_edges) % 2))
    ei.setflags(write=False)
    ea.setflags(write=False)
    return ei, ea


def _attr(ea, width):
    return None if width is None else np.ascontiguousarray(ea[:, :width])


def _gpu(a):
    return None if a is None else torch.from_numpy(np.array(a)).cuda()


def _assert_equals_reference(out, ei, ea, p, seed, step, what):
    ref_i, ref_a = dropout_adj_ref(ei, ea, p, seed, step)
    oi, oa = out
    assert oi.dtype == torch.int64 and oi.is_cuda and tuple(oi.shape) == ref_i.shape, (what, tuple(oi.shape), ref_i.shape)
    assert torch.equal(oi.cpu(), torch.from_numpy(ref_i)), what
    if ea is None:
        assert oa is None, what
    else:
        assert oa.dtype == torch.int64 and oa.is_cuda and tuple(oa.shape) == ref_a.shape, (what, tuple(oa.shape))
        assert torch.equal(oa.cpu(), torch.from_numpy(ref_a)), what
    return ref_i.shape[1] // 2


def _plan(n_edges):
    """(width, (seed, step), p) cells of one size: the whole product at the block-boundary sizes, elsewhere two widths
    times three (seed, step, p), rotated so that every width, pair and probability is used across the sizes."""
    if n_edges in BOUNDARY:
        return [(a, ss, p) for a in WIDTHS for ss in SEED_STEPS_GPU for p in PROBS]
    idx = SIZES.index(n_edges)
    widths = (None, 3) if idx % 2 == 0 else (1, 5)
    picks = [(SEED_STEPS_GPU[(idx + 2 * j) % len(SEED_STEPS_GPU)], PROBS[(idx + j) % len(PROBS)]) for j in range(3)]
    return [(a, ss, p) for a in widths for ss, p in picks]


# ---- a. PF.dropout_adj is the reference, element for element --------------------------------------------------------
@pytest.mark.parametrize('n_edges', SIZES)
def test_dropout_adj_equals_the_reference(n_edges):
    from pointvs_amd import functional as PF
    ei, ea5 = _edge_list(n_edges)
    ei_d = _gpu(ei)
    kept = set()
    for width, (seed, step), p in _plan(n_edges):
        ea = _attr(ea5, width)
        out = PF.dropout_adj(ei_d, _gpu(ea), p, training=True, seed=seed, step=step)
        kept.add(_assert_equals_reference(out, ei, ea, p, seed, step, (n_edges, width, seed, step, p)))
    assert n_edges < 255 or len(kept) > 1


def test_the_whole_plan_covers_every_width_pair_and_probability_at_every_size():
    for n_edges in SIZES:
        plan = _plan(n_edges)
        assert len({a for a, _, _ in plan}) >= 2 and len({(ss, p) for _, ss, p in plan}) >= 2
    for n_edges in BOUNDARY:
        plan = _plan(n_edges)
        assert {a for a, _, _ in plan} == set(WIDTHS) and {ss for _, ss, _ in plan} == set(SEED_STEPS_GPU)
        assert {p for _, _, p in plan} == set(PROBS)
    everything = [c for n in SIZES for c in _plan(n)]
    assert {a for a, _, _ in everything} == set(WIDTHS) and {ss for _, ss, _ in everything} == set(SEED_STEPS_GPU)


def test_node_ids_above_two_to_the_31_survive():
    from pointvs_amd import functional as PF
    ei, ea5 = _edge_list(513, lo=2 ** 31, hi=2 ** 40)
    assert int(ei.min()) >= 2 ** 31 and int(ei.max()) >= 2 ** 39
    ea = _attr(ea5, 3)
    for (seed, step), p in ((SEED_STEPS_GPU[1], 0.3), (SEED_STEPS_GPU[4], 0.5)):
        out = PF.dropout_adj(_gpu(ei), _gpu(ea), p, training=True, seed=seed, step=step)
        assert _assert_equals_reference(out, ei, ea, p, seed, step, 'wide ids') > 50


def test_the_draw_is_a_function_of_seed_and_step_on_any_stream():
    from pointvs_amd import functional as PF
    ei, ea5 = _edge_list(4097)
    ei_d, ea_d = _gpu(ei), _gpu(_attr(ea5, 3))
    seed, step = SEED_STEPS_GPU[1]
    first = PF.dropout_adj(ei_d, ea_d, 0.3, training=True, seed=seed, step=step)
    second = PF.dropout_adj(ei_d, ea_d, 0.3, training=True, seed=seed, step=step)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        third = PF.dropout_adj(ei_d, ea_d, 0.3, training=True, seed=seed, step=step)
    side.synchronize()
    for other in (second, third):
        assert torch.equal(first[0], other[0]) and torch.equal(first[1], other[1])
    _assert_equals_reference(third, ei, _attr(ea5, 3), 0.3, seed, step, 'side stream')


def test_draws_that_equal_the_probability_are_kept():
    """>= p, not > p: the smallest and the largest 24-bit value (searched draws of the host file), and a probability
    that is the value of one of the list's own counters."""
    from pointvs_amd import functional as PF
    ei, ea5 = _edge_list(257)
    ei = ei.copy()
    for e in (ZERO_DRAW[2], MAX_DRAW[2]):
        ei[:, e] = (4, 8)
    ea = _attr(ea5, 1)
    p_max = float(np.float32(1.0 - 2.0 ** -24))
    cand = int((ei[0] <= ei[1]).sum())
    for (seed, step, _), p, want in ((ZERO_DRAW, 2.0 ** -24, cand - 1), (MAX_DRAW, 2.0 ** -24, cand), (MAX_DRAW, p_max, 1),
                                     (ZERO_DRAW, p_max, 0)):
        out = PF.dropout_adj(_gpu(ei), _gpu(ea), p, training=True, seed=seed, step=step)
        assert _assert_equals_reference(out, ei, ea, p, seed, step, (seed, step, p)) == want
    seed, step = SEED_STEPS_GPU[2]
    u = uniform24(seed, step, np.arange(257))
    e0 = int(np.flatnonzero((ei[0] <= ei[1]) & (u > 0.2) & (u < 0.8))[0])
    p = float(u[e0])
    out = PF.dropout_adj(_gpu(ei), _gpu(ea), p, training=True, seed=seed, step=step)
    _assert_equals_reference(out, ei, ea, p, seed, step, 'p = a drawn value')
    assert int(ea[e0, 0]) in out[1][:, 0].tolist()


# ---- b. degenerate lists --------------------------------------------------------------------------------------------
def _forty_candidates():
    """40 row < col pairs with their reverses first: 80 edges, 40 of them candidates."""
    rng = np.random.default_rng(40)
    lo, hi = rng.integers(0, 15, 40), rng.integers(15, 30, 40)
    return np.stack([np.concatenate([hi, lo]), np.concatenate([lo, hi])]).astype(np.int64)


def _step_that_keeps_nothing(ei, seed, p=0.999):
    for step in range(2 ** 40, 2 ** 40 + 8):
        if dropout_adj_ref(ei, None, p, seed, step)[0].shape[1] == 0:
            return step
    raise AssertionError('no empty draw among 8 steps (each is empty with probability 0.96)')


@pytest.mark.parametrize('width', WIDTHS)
def test_lists_of_which_nothing_survives(width):
    from pointvs_amd import functional as PF
    ei, ea5 = _edge_list(300)
    down = np.stack([np.maximum(ei[0], ei[1]) + 1, np.minimum(ei[0], ei[1])])      # every edge has row > col
    forty = _forty_candidates()
    step = _step_that_keeps_nothing(forty, seed=7 + 2 ** 32)
    for edges, p, seed, stp in ((down, 0.3, 5, 1), (forty, 0.999, 7 + 2 ** 32, step)):
        ea = _attr(ea5[:edges.shape[1]], width)
        oi, oa = PF.dropout_adj(_gpu(edges), _gpu(ea), p, training=True, seed=seed, step=stp)
        assert _assert_equals_reference((oi, oa), edges, ea, p, seed, stp, 'empty') == 0
        assert tuple(oi.shape) == (2, 0) and (oa is None if width is None else tuple(oa.shape) == (0, width))


def test_a_list_of_self_loops():
    from pointvs_amd import functional as PF
    ei, ea5 = _edge_list(513)
    loops = np.stack([ei[0], ei[0]])
    ea = _attr(ea5, 3)
    seed, step = SEED_STEPS_GPU[1]
    out = PF.dropout_adj(_gpu(loops), _gpu(ea), 0.5, training=True, seed=seed, step=step)
    k = _assert_equals_reference(out, loops, ea, 0.5, seed, step, 'self-loops')
    assert 150 < k < 370 and torch.equal(out[0][:, :k], out[0][:, k:]), 'a surviving self-loop is listed twice'


def test_int32_and_strided_inputs_give_the_contiguous_int64_result():
    from pointvs_amd import functional as PF
    ei, ea5 = _edge_list(4097)
    ei_d, ea_d = _gpu(ei), _gpu(_attr(ea5, 3))
    seed, step = SEED_STEPS_GPU[2]
    want = PF.dropout_adj(ei_d, ea_d, 0.3, training=True, seed=seed, step=step)
    _assert_equals_reference(want, ei, _attr(ea5, 3), 0.3, seed, step, 'contiguous')
    transposed = ei_d.t().contiguous().t()
    sliced = torch.stack([ei_d, ei_d + 1], 2)[:, :, 0]
    ea_strided = _gpu(ea5)[:, :3]
    assert not transposed.is_contiguous() and not sliced.is_contiguous() and not ea_strided.is_contiguous()
    for edges, attrs in ((ei_d.int(), ea_d), (transposed, ea_d), (sliced, ea_strided)):
        got = PF.dropout_adj(edges, attrs, 0.3, training=True, seed=seed, step=step)
        assert got[0].dtype == torch.int64 and got[1].dtype == torch.int64
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- c. the raw entry points refuse what they document --------------------------------------------------------------
POISON = -7


def test_raw_mark_refuses_bad_arguments_and_leaves_pos_alone():
    """Every call here is refused by a check ahead of the launches: a status return, pos untouched."""
    from pointvs_amd import _lib
    lib = _lib.lib()
    n_edges = 300
    ei = _gpu(_edge_list(n_edges)[0])
    pos = torch.full((n_edges + 1,), POISON, dtype=torch.int32, device='cuda')
    ws_bytes = lib.pvs_dropout_adj_workspace_bytes(n_edges)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    stream = _lib.stream(ei.device)

    def mark(edges=ei, e=n_edges, p=0.5, out=pos, nbytes=ws_bytes):
        return lib.pvs_dropout_adj_mark(_lib.ptr(edges), e, p, 5, 1, _lib.ptr(out), _lib.ptr(ws), nbytes, stream)

    refused = dict(p_one=mark(p=1.0), p_above=mark(p=1.5), p_negative=mark(p=-0.25), p_nan=mark(p=float('nan')),
                   workspace_short=mark(nbytes=ws_bytes - 1), null_edges=mark(edges=None), null_pos=mark(out=None),
                   negative_e=mark(e=-1))
    torch.cuda.synchronize()
    assert all(rc != 0 for rc in refused.values()), refused
    assert lib.pvs_last_error()
    assert bool((pos == POISON).all())


def test_raw_fill_refuses_null_outputs():
    """n_kept = 0 with an all-zero pos (a consistent pair: nothing survived), so even an entry point that did not refuse
    would return before its launch."""
    from pointvs_amd import _lib
    lib = _lib.lib()
    n_edges = 300
    ei, ea5 = _edge_list(n_edges)
    ei_d, ea_d = _gpu(ei), _gpu(_attr(ea5, 3))
    pos = torch.zeros(n_edges + 1, dtype=torch.int32, device='cuda')
    out_i = torch.full((2, 2), POISON, dtype=torch.int64, device='cuda')
    out_a = torch.full((2, 3), POISON, dtype=torch.int64, device='cuda')
    stream = _lib.stream(ei_d.device)

    def fill(attr=ea_d, width=3, oi=out_i, oa=out_a):
        return lib.pvs_dropout_adj_fill(_lib.ptr(ei_d), _lib.ptr(attr), width, n_edges, _lib.ptr(pos), 0, _lib.ptr(oi),
                                        _lib.ptr(oa), stream)

    refused = dict(null_out_index=fill(oi=None), null_edge_attr=fill(attr=None), null_out_attr=fill(oa=None))
    assert all(rc != 0 for rc in refused.values()), refused
    assert fill() == 0 and fill(attr=None, width=0, oa=None) == 0
    torch.cuda.synchronize()
    assert bool((out_i == POISON).all()) and bool((out_a == POISON).all())


def test_workspace_bytes_grow_with_the_edge_count():
    from pointvs_amd import _lib
    lib = _lib.lib()
    sizes = [lib.pvs_dropout_adj_workspace_bytes(e) for e in SIZES]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert all(s >= 4 * (e + 1) for s, e in zip(sizes, SIZES))


# ---- the model ------------------------------------------------------------------------------------------------------
FULL = dict(edge_attention=True, edge_residual=True, node_attention=True, residual=True)
RADIUS = 4.0


def _model(save_path, dropout=0.25, **flags):
    """k = 32, two layers, build_net's defaults otherwise; the last coordinate weight (Xavier gain 0.001) a hundred times
    larger, so that the coordinate update is not lost beside the coordinates."""
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    kw = dict(dim_input=12, k=32, dim_output=1, num_layers=2, dropout=dropout, **flags)
    torch.manual_seed(3)
    model = SartorrasEGNN(save_path, 2e-3, 1e-4, None, None, silent=True, **kw)
    with torch.no_grad():
        for layer in list(model.layers)[1:]:
            layer.coord_mlp[2].weight.mul_(100.0)
    return model.cuda().train(), dict(kw, _class='SartorrasEGNN')


def _two_graphs():
    from pointvs_amd.graph import Batch
    from pointvs_amd.synthetic import synthetic_graph
    return Batch.from_data_list([synthetic_graph(90 + g, n_nodes=100 + 7 * g, n_lig=10, edge_radius=RADIUS)
                                 for g in range(2)])


def _one_small_graph():
    """30 nodes, the 80 edges of _forty_candidates."""
    from pointvs_amd.graph import Batch
    rng = np.random.default_rng(8)
    ei = _forty_candidates()
    x = np.zeros((30, 12), dtype=np.float32)
    x[np.arange(30), rng.integers(0, 11, 30)] = 1.0
    return Batch(x=torch.from_numpy(x), pos=torch.from_numpy(rng.normal(size=(30, 3)).astype(np.float32) * 2),
                 edge_index=torch.from_numpy(ei), edge_attr=torch.nn.functional.one_hot(torch.from_numpy(ei[0] % 3), 3),
                 batch=torch.zeros(30, dtype=torch.int64), ptr=torch.tensor([0, 30]), y=torch.ones(1),
                 lig_fname=['l'], rec_fname=['r'], num_graphs=1)


def _record_draws(monkeypatch):
    """PF.dropout_adj wrapped: every call's arguments and outputs are kept (as host arrays), and it still calls through."""
    from pointvs_amd import functional as PF
    real, calls = PF.dropout_adj, []

    def recording(edge_index, edge_attr=None, p=0.5, force_undirected=True, training=True, seed=0, step=0):
        out = real(edge_index, edge_attr, p, force_undirected=force_undirected, training=training, seed=seed, step=step)
        calls.append(types.SimpleNamespace(
            seed=seed, step=step, p=p, training=training, edges=edge_index.cpu().numpy(),
            attr=None if edge_attr is None else edge_attr.cpu().numpy(), out_edges=out[0].cpu().numpy(),
            out_attr=None if out[1] is None else out[1].cpu().numpy()))
        return out
    monkeypatch.setattr(PF, 'dropout_adj', recording)
    return calls


def _restart(model, seed, global_iter=0):
    torch.manual_seed(seed)
    model.global_iter, model.p_epoch, model.a_epoch = global_iter, 0, 0
    model.dropout_keys.base, model.dropout_keys.calls = None, 0


def _assert_call_equals_reference(call):
    ref_i, ref_a = dropout_adj_ref(call.edges, call.attr, call.p, call.seed, call.step)
    assert np.array_equal(call.out_edges, ref_i) and call.out_edges.shape == ref_i.shape
    assert np.array_equal(call.out_attr, ref_a) and call.out_attr.shape == ref_a.shape


# ---- d. the model's (seed, step) schedule ---------------------------------------------------------------------------
def test_the_models_schedule_of_seeds_and_steps(monkeypatch, tmp_path):
    calls = _record_draws(monkeypatch)
    model, _ = _model(tmp_path)
    batch = _two_graphs().to('cuda')

    def run_schedule():
        del calls[:]
        _restart(model, seed=77)
        with torch.no_grad():
            for bump in (None, None, None, 'global_iter', 'p_epoch', 'a_epoch', 'global_iter'):
                if bump:
                    setattr(model, bump, getattr(model, bump) + 1)
                model(batch)
        return list(calls)

    first = run_schedule()
    assert len(first) == 7 and all(c.training and c.p == 0.25 for c in first)
    steps = [c.step for c in first]
    assert len(set(steps)) == 7, 'every forward, and every bump of a counter, draws at a step not seen before'
    assert len({c.seed for c in first}) == 1 and first[0].seed == 77
    assert all(0 <= s < 2 ** 64 for s in steps) and any(s >> 32 for s in steps)
    assert len({c.out_edges.tobytes() for c in first}) == 7
    for c in first:
        assert np.array_equal(c.edges, batch.edge_index.cpu().numpy())
        _assert_call_equals_reference(c)
    second = run_schedule()
    assert [(c.seed, c.step) for c in second] == [(c.seed, c.step) for c in first]
    assert all(np.array_equal(a.out_edges, b.out_edges) and np.array_equal(a.out_attr, b.out_attr)
               for a, b in zip(first, second))
    # data-parallel rank 1: another seed (its high word set), another list at the same step
    monkeypatch.setattr(torch.distributed, 'is_initialized', lambda: True)
    monkeypatch.setattr(torch.distributed, 'get_rank', lambda *a, **k: 1)
    del calls[:]
    _restart(model, seed=77)
    with torch.no_grad():
        model(batch)
    rank1, = calls
    assert rank1.step == first[0].step and rank1.seed != first[0].seed and rank1.seed >> 32 and 0 <= rank1.seed < 2 ** 64
    assert rank1.seed == (77 + 0x9E3779B97F4A7C15) % 2 ** 64
    assert not np.array_equal(rank1.out_edges, first[0].out_edges)
    _assert_call_equals_reference(rank1)


# ---- e. the dropped training step equals the oracle on the drawn list -----------------------------------------------
def _oracle(sd, cfg, batch, edges, attr, dtype, perm=None):
    """Logits, loss, parameter gradients and last-layer edge messages (in the order of `edges`) of the oracle on the
    list `edges`; perm: the same list handed over in another edge order (one more sample of fp32 rounding noise)."""
    from oracle import egnn_oracle as orc
    ei, ea = torch.from_numpy(edges), torch.from_numpy(attr)
    if perm is not None:
        ei, ea = ei[:, perm], ea[perm]
    trace = {}
    y, loss, grads = orc.forward_backward(sd, cfg, batch.x, batch.pos, ei, ea, batch.batch, batch.y.float(), dtype=dtype,
                                          trace=trace)
    m = trace['m_last'].detach()
    if perm is not None:
        back = torch.empty_like(m)
        back[perm] = m
        m = back
    res = {'logits': y, 'loss': loss, 'edge messages': m}
    res.update({f'grad {k}': v for k, v in grads.items()})
    return {k: (None if v is None else v.numpy()) for k, v in res.items()}


def _references(sd, cfg, batch, edges, attr):
    ref64 = _oracle(sd, cfg, batch, edges, attr, torch.float64)
    perms = edge_permutations(edges.shape[1], count=2) if edges.shape[1] else []
    ref32 = [_oracle(sd, cfg, batch, edges, attr, torch.float32)] + [_oracle(sd, cfg, batch, edges, attr, torch.float32, p)
                                                                    for p in perms]
    return ref64, ref32


def _training_step(model, batch_dev):
    model.zero_grad(set_to_none=True)
    y_pred, y_true, _, _ = model.unpack_input_data_and_predict(batch_dev)
    loss = model.get_loss(y_true.to(y_pred.device), y_pred)
    loss.backward()
    got = {'logits': y_pred, 'loss': loss}
    got.update({f'grad {n}': p.grad for n, p in model.named_parameters()})
    return got


def _edge_messages(model, batch_dev, edges, attr):
    feats, _, coords, _, bvec = model.unpack_graph(batch_dev)
    with torch.no_grad():
        return model.get_embeddings(feats, _gpu(edges), coords, _gpu(attr), bvec)[1]


def _graph_as_handed_over(way, batch):
    """(device batch, COO list the draw numbers): the batch's own list, or - graph built on the GPU - the builder's
    sorted list."""
    from pointvs_amd.radius_graph import attach_radius_graph
    dev = _two_graphs().to('cuda') if batch is None else batch
    if way == 'coo':
        return dev, dev.edge_index.cpu().numpy(), dev.edge_attr.cpu().numpy()
    pg = attach_radius_graph(dev, RADIUS).prepared
    pg.check_status()
    e = pg.n_edges
    edges = np.stack([pg.t['row'][:e].cpu().numpy(), pg.t['col'][:e].cpu().numpy()]).astype(np.int64)
    attr = np.eye(pg.n_edge_attr, dtype=np.int64)[pg.t['etype'][:e].cpu().numpy()]
    return dev, edges, attr


@pytest.mark.parametrize('way', ['coo', 'built'])
@pytest.mark.parametrize('flags', ['defaults', 'full'])
def test_dropped_training_step_equals_the_oracle_on_the_drawn_list(flags, way, monkeypatch, tmp_path):
    """Logits, loss and every parameter gradient of a training-mode forward + backward, and the edge messages of
    get_embeddings row for row in the order of the dropped list, each against the oracle on dropout_adj_ref's list for
    the recorded (seed, step)."""
    calls = _record_draws(monkeypatch)
    model, cfg = _model(tmp_path, **(FULL if flags == 'full' else {}))
    host = _two_graphs()
    dev, edges, attr = _graph_as_handed_over(way, None)
    assert edges.shape[1] > 1000 and (way == 'built') == (getattr(dev, 'prepared', None) is not None)
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    _restart(model, seed=21, global_iter=5)
    got = _training_step(model, dev)
    got['edge messages'] = _edge_messages(model, dev, edges, attr)
    assert len(calls) == 2 and calls[0].step != calls[1].step
    log = CaseLog(f'dropout-{flags}-{way}')
    for call, keys in ((calls[0], [k for k in got if k != 'edge messages']), (calls[1], ['edge messages'])):
        assert np.array_equal(call.edges, edges) and np.array_equal(call.attr, attr)
        drawn_i, drawn_a = dropout_adj_ref(edges, attr, 0.25, call.seed, call.step)
        assert 0 < drawn_i.shape[1] < edges.shape[1]
        ref64, ref32 = _references(sd, cfg, host, drawn_i, drawn_a)
        floor = grad_floor({k: v for k, v in ref64.items() if k.startswith('grad ')})
        for key in keys:
            if got[key] is None or ref64[key] is None:      # (the last layer's coordinate branch: nothing reads x_L)
                assert got[key] is None and ref64[key] is None and 'coord_mlp' in key, key
                continue
            value = got[key].detach().cpu().numpy()
            assert value.dtype == np.float32 and value.size == ref64[key].size, key
            assert_strict(value.reshape(ref64[key].shape), ref64[key], [r[key] for r in ref32], f'{log.case} {key}',
                          floor=floor if key.startswith('grad ') else 0.0, log=log)
    assert tuple(got['edge messages'].shape) == (calls[1].out_edges.shape[1], 32)
    log.finish()


def _iteration_that_keeps_nothing(edges, seed, p):
    """global_iter at which the model's first two draws (the training step, then get_embeddings) both keep nothing."""
    from pointvs_amd.egnn_satorras import _mix64
    for global_iter in range(16):
        steps = [_mix64(_mix64(global_iter) + calls) for calls in (1, 2)]
        if all(dropout_adj_ref(edges, None, p, seed, s)[0].shape[1] == 0 for s in steps):
            return global_iter, steps
    raise AssertionError('no pair of empty draws in 16 iterations (each is empty with probability 0.92)')


def test_a_draw_that_keeps_nothing_trains_on_the_empty_list(monkeypatch, tmp_path):
    calls = _record_draws(monkeypatch)
    model, cfg = _model(tmp_path, dropout=0.999, **FULL)
    host = _one_small_graph()
    dev, edges, attr = _graph_as_handed_over('coo', _one_small_graph().to('cuda'))
    global_iter, steps = _iteration_that_keeps_nothing(edges, 21, 0.999)
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    _restart(model, seed=21, global_iter=global_iter)
    got = _training_step(model, dev)
    got['edge messages'] = _edge_messages(model, dev, edges, attr)
    assert [c.step for c in calls] == steps and all(c.out_edges.shape == (2, 0) and c.out_attr.shape == (0, 3) for c in calls)
    assert tuple(got['edge messages'].shape) == (0, 32)
    ref64, ref32 = _references(sd, cfg, host, np.zeros((2, 0), dtype=np.int64), np.zeros((0, 3), dtype=np.int64))
    floor = grad_floor({k: v for k, v in ref64.items() if k.startswith('grad ')})
    log = CaseLog('dropout-kept0')
    for key, ref in ref64.items():
        if key == 'edge messages':
            continue
        if got[key] is None:          # a parameter only the edges reach: no gradient at all, where the oracle has zeros
            assert ref is None or not ref.any(), key
            continue
        assert ref is not None, key
        value = got[key].detach().cpu().numpy()
        assert_strict(value.reshape(ref.shape), ref, [r[key] for r in ref32], f'{log.case} {key}',
                      floor=floor if key.startswith('grad ') else 0.0, log=log)
    log.finish()


def test_dropped_training_step_of_the_fp64_model(monkeypatch, tmp_path):
    from tests.test_gpu_fp64 import _check
    calls = _record_draws(monkeypatch)
    model, cfg = _model(tmp_path, **FULL)
    model = model.double()
    host = _two_graphs()
    dev, edges, attr = _graph_as_handed_over('coo', None)
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    _restart(model, seed=21, global_iter=5)
    got = _training_step(model, dev)
    got['edge messages'] = _edge_messages(model, dev, edges, attr)
    assert len(calls) == 2
    for call, keys in ((calls[0], [k for k in got if k != 'edge messages']), (calls[1], ['edge messages'])):
        drawn_i, drawn_a = dropout_adj_ref(edges, attr, 0.25, call.seed, call.step)
        ref64 = _oracle(sd, cfg, host, drawn_i, drawn_a, torch.float64)
        g_max = max(float(np.abs(v).max()) for k, v in ref64.items() if k.startswith('grad ') and v is not None)
        for key in keys:
            if got[key] is None or ref64[key] is None:
                assert got[key] is None and ref64[key] is None and 'coord_mlp' in key, key
                continue
            assert got[key].dtype == torch.float64, key
            _check(got[key], ref64[key], f'fp64 dropout {key}', g_max if key.startswith('grad ') else 0.0)


def test_eval_mode_never_reaches_the_draw(monkeypatch, tmp_path):
    calls = _record_draws(monkeypatch)
    model, _ = _model(tmp_path)
    dev, edges, attr = _graph_as_handed_over('built', None)
    model.eval()
    with torch.no_grad():
        model(dev)
        _edge_messages(model, dev, edges, attr)
        dev.prepared = None
        model(dev)
    assert calls == []


# ---- captured training ----------------------------------------------------------------------------------------------
def test_captured_training_refuses_edge_dropout(tmp_path):
    """The refusal comes before any step: parameters unchanged, no capture statistics, no stream left capturing; the
    same model trains eagerly."""
    model, _ = _model(tmp_path)
    batch = _two_graphs().to('cuda')
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    with pytest.raises(NotImplementedError, match='dropout'):
        model.train_model([batch, batch, batch], epochs=1, capture=True)
    assert not torch.cuda.is_current_stream_capturing()
    assert not any((getattr(model, 'last_capture_stats', None) or {}).values())
    assert model.global_iter == 0 and all(torch.equal(p, before[n]) for n, p in model.named_parameters())
    losses = [float(v) for v in model.train_model([batch, batch, batch], epochs=1, capture=False)]
    assert len(losses) == 3 and np.isfinite(losses).all() and len(set(losses)) == 3
    assert any(not torch.equal(p, before[n]) for n, p in model.named_parameters())
