"""fp64 path (--double): the model in float64 on the fp64 HIP kernels, against the oracle's fp64 run.

The bound is deterministic (no fp32 noise draws): per tensor
    max|got - ref64| <= 1e-9 * max|ref64| + 1e-14 * G
with G the case's largest gradient magnitude (a floor for gradients that are mathematically zero). fp32 arithmetic
cannot meet it (its errors are >= 1e-7 relative); the first test also shows that the fp32 path breaks it.
"""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from tests._golden import CASES, GoldenCase
from tests.test_gpu_parity import build_model, make_batch

pytestmark = pytest.mark.gpu
REL64, FLOOR64 = 1e-9, 1e-14
ROOT = Path(__file__).resolve().parent.parent


def _np(t):
    return (t.detach().cpu() if isinstance(t, torch.Tensor) else torch.as_tensor(t)).double().numpy()


def _check(got, ref, what, g_max=0.0):
    got, ref = _np(got), _np(ref)
    assert got.size == ref.size, (what, got.shape, ref.shape)
    ref = ref.reshape(got.shape)
    if got.size == 0:
        return
    err = float(np.abs(got - ref).max())
    bound = REL64 * float(np.abs(ref).max()) + FLOOR64 * g_max
    assert err <= bound, f'{what}: |got - ref64| = {err:.3e} > bound {bound:.3e}'


def _bound_broken(got, ref):
    got, ref = _np(got), _np(ref)
    ref = ref.reshape(got.shape)
    return float(np.abs(got - ref).max()) > REL64 * float(np.abs(ref).max())


def _oracle64(sd, cfg, x, pos, edge_index, edge_attr, batch, y):
    from oracle import egnn_oracle as orc
    t64 = {}
    y64, loss64, g64 = orc.forward_backward(sd, cfg, x, pos, edge_index, edge_attr, batch, y,
                                            dtype=torch.float64, trace=t64)
    g_max = max(float(g.abs().max()) for g in g64.values() if g is not None and g.numel())
    return y64, loss64, g64, t64, g_max


def _check_model(model, batch_fn, sd, cfg, x, pos, edge_index, edge_attr, batch, y, tag, layers=True):
    """Every traced h / x, attention values, edge messages, logits, loss and parameter gradient of an fp64 model."""
    from oracle import egnn_oracle as orc
    from pointvs_amd.graph import prepared_for
    y64, loss64, g64, t64, g_max = _oracle64(sd, cfg, x, pos, edge_index, edge_attr, batch, y)
    if layers:
        feats, edges, coords, eattr, bvec = model.unpack_graph(batch_fn())
        assert feats.dtype == torch.float64 and coords.dtype == torch.float64
        pg = prepared_for(edges, eattr, feats.size(0))
        trace = {}
        with torch.no_grad():
            model.embed_prepared(pg, feats, coords, need_messages=True, trace=trace)
        n_layers = orc.layer_flags(cfg, 0)['num_layers']
        for li in range(n_layers + 1):
            assert trace[f'h{li}'].dtype == torch.float64
            _check(trace[f'h{li}'], t64[f'h{li}'], f'{tag} h{li}')
            _check(trace[f'x{li}'], t64[f'x{li}'], f'{tag} x{li}')
        for li, layer in enumerate(list(model.layers)[1:], start=1):
            if t64.get(f'att{li}') is not None:
                assert layer.att_val.dtype == np.float64
                _check(layer.att_val, t64[f'att{li}'], f'{tag} att{li}')
            if t64.get(f'natt{li}') is not None:
                assert layer.node_att_val.dtype == np.float64
                _check(layer.node_att_val, t64[f'natt{li}'], f'{tag} natt{li}')
        with torch.no_grad():
            _, m_in = model.get_embeddings(feats, edges, coords, eattr, bvec)
        assert m_in.dtype == torch.float64
        _check(m_in, t64['m_last'], f'{tag} edge messages')
    model.zero_grad()
    y_pred, _, _, _ = model.unpack_input_data_and_predict(batch_fn())
    assert y_pred.dtype == torch.float64
    _check(y_pred, y64, f'{tag} logits')
    loss = model.get_loss(y.cuda(), y_pred)
    _check(loss, loss64, f'{tag} loss')
    loss.backward()
    for name, p in model.named_parameters():
        if p.grad is None:
            assert g64[name] is None, (tag, name)
            continue
        assert p.grad.dtype == torch.float64
        _check(p.grad, g64[name], f'{tag} grad {name}', g_max)
    return y64


@pytest.mark.parametrize('name', CASES)
def test_golden_cases_in_fp64_match_the_fp64_oracle(name):
    c = GoldenCase(name)
    model = build_model(c).double()
    _check_model(model, lambda: make_batch(c), c.sd, c.cfg, c.x, c.pos, c.edge_index, c.edge_attr, c.batch,
                 c.y_true, name)
    if name == 'c0_clidefault_g5batch':     # the bound discriminates: the fp32 path does not meet it
        y64 = _oracle64(c.sd, c.cfg, c.x, c.pos, c.edge_index, c.edge_attr, c.batch, c.y_true)[0]
        y32, _, _, _ = build_model(c).unpack_input_data_and_predict(make_batch(c))
        assert _bound_broken(y32, y64)


# ---- synthetic models and graphs ----
ALL_ON = dict(dim_input=12, dim_output=1, num_layers=2, residual=True, edge_residual=True, edge_attention=True,
              normalize=True, tanh=True, graphnorm=True, update_coords=True, node_attention=True,
              gated_residual=True, model_task='classification')


def _model(kwargs, seed=7, save_path=Path('/tmp/pvs_fp64')):
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    torch.manual_seed(seed)
    m = SartorrasEGNN(save_path, 2e-3, 1e-4, None, None, silent=True, **kwargs)
    return m.double().cuda().eval()


def _graphs(parts, seed=3, n_feat=12):
    """parts: list of (n_nodes, edge list [(i, j), ...] local ids). Returns the batch tensors (int64 one-hot attrs)."""
    gen = torch.Generator().manual_seed(seed)
    xs, ps, es, bs, off = [], [], [], [], 0
    for g, (n, edges) in enumerate(parts):
        xs.append(torch.randn(n, n_feat, generator=gen))
        ps.append(torch.randn(n, 3, generator=gen) * 3.0)
        if edges:
            es.append(torch.tensor(edges, dtype=torch.int64).t() + off)
        bs.append(torch.full((n,), g, dtype=torch.int64))
        off += n
    ei = torch.cat(es, 1) if es else torch.zeros((2, 0), dtype=torch.int64)
    attr = torch.nn.functional.one_hot(torch.randint(0, 3, (ei.shape[1],), generator=gen), 3)
    y = torch.randint(0, 2, (len(parts),), generator=gen).float()
    return torch.cat(xs), torch.cat(ps), ei, attr, torch.cat(bs), y


def _batch_fn(x, pos, ei, attr, b, y):
    from pointvs_amd.graph import Batch
    n_graphs = int(b.max()) + 1
    return lambda: Batch(x=x.clone(), edge_index=ei.clone(), edge_attr=attr.clone(), pos=pos.clone(), batch=b.clone(),
                         y=y.clone(), lig_fname=['l'] * n_graphs, rec_fname=['r'] * n_graphs).to('cuda')


def _run(kwargs, data, tag, layers=True):
    model = _model(kwargs)
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    cfg = dict(kwargs, _class='SartorrasEGNN')
    return _check_model(model, _batch_fn(*data), sd, cfg, *data, tag, layers=layers)


def _random_graph(n, p, seed):
    rng = np.random.default_rng(seed)
    return [(int(i), int(j)) for i in range(n) for j in range(n) if i != j and rng.random() < p]


@pytest.mark.parametrize('k', [16, 24, 48, 96])
def test_widths_padded_and_decomposed_match_the_fp64_oracle(k):
    data = _graphs([(30, _random_graph(30, 0.3, 1)), (20, _random_graph(20, 0.4, 2))])
    _run(dict(ALL_ON, k=k), data, f'k{k}')


def test_ragged_and_degenerate_graphs_match_the_fp64_oracle():
    dup = _random_graph(12, 0.3, 5)
    dup += dup[:7] + [(0, 0), (3, 3), (4, 4)]          # duplicate edges and self-loops
    iso = [(i, j) for i, j in _random_graph(25, 0.2, 6) if i < 15 and j < 15]     # nodes 15..24 isolated
    parts = [(12, dup), (6, []), (1, []), (25, iso)]
    for k, extra in ((32, {}), (64, dict(softmax_attention=True, gated_residual=False, rezero=True)),
                     (16, dict(permutation_invariance=True, edge_residual=False))):
        _run(dict(ALL_ON, k=k, **extra), _graphs(parts), f'ragged k{k}')
    # high-degree rows: one hub row and one hub column among several thousand edges
    n = 300
    edges = _random_graph(n, 0.03, 8) + [(0, j) for j in range(1, n)] + [(i, 1) for i in range(2, n)]
    _run(dict(ALL_ON, k=32, softmax_attention=True), _graphs([(n, edges)]), 'hub rows', layers=False)


def test_cfg2_size_graph_matches_the_fp64_oracle():
    """One whole 2000-atom graph with a radius-10 A edge set (the reference's default-shape density)."""
    gen = torch.Generator().manual_seed(11)
    n = 2000
    pos = torch.rand(n, 3, generator=gen, dtype=torch.float64) * 37.0
    d = torch.cdist(pos, pos)
    ei = torch.nonzero((d < 10.0) & (d > 1e-7)).t().contiguous()
    attr = torch.nn.functional.one_hot(torch.randint(0, 3, (ei.shape[1],), generator=gen), 3)
    x = torch.randn(n, 12, generator=gen)
    data = (x, pos, ei, attr, torch.zeros(n, dtype=torch.int64), torch.ones(1))
    kw = dict(dim_input=12, dim_output=1, k=32, num_layers=3, update_coords=True, model_task='classification')
    _run(kw, data, 'cfg2 graph', layers=False)


FAMILIES = [dict(ALL_ON), dict(ALL_ON, softmax_attention=True, gated_residual=False, rezero=True),
            dict(ALL_ON, edge_residual=False, attention_activation_fn='relu', permutation_invariance=True),
            dict(ALL_ON, attention_activation_fn='silu', graphnorm=False, normalize=False, tanh=False),
            dict(ALL_ON, attention_activation_fn='tanh', gated_residual=False, update_coords=False),
            dict(dim_input=12, dim_output=1, num_layers=3, update_coords=True, model_task='classification')]


@pytest.mark.parametrize('k', [32, 64])
@pytest.mark.parametrize('fam', range(len(FAMILIES)))
def test_fp64_forward_backward_is_bitwise_reproducible(k, fam):
    data = _graphs([(40, _random_graph(40, 0.25, 21)), (35, _random_graph(35, 0.3, 22))])
    model = _model(dict(FAMILIES[fam], k=k))
    batch_fn = _batch_fn(*data)
    runs = []
    for _ in range(2):
        model.zero_grad()
        y, _, _, _ = model.unpack_input_data_and_predict(batch_fn())
        feats, edges, coords, eattr, b = model.unpack_graph(batch_fn())
        with torch.no_grad():
            h, m = model.get_embeddings(feats, edges, coords, eattr, b)
        model.get_loss(data[5].cuda(), y).backward()
        runs.append([y.detach().clone(), h.clone(), m.clone()] +
                    [p.grad.clone() for p in model.parameters() if p.grad is not None])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_five_training_steps_match_oracle_and_torch_adam(tmp_path):
    """train_model in fp64 (clip 1.0 + Adam, as the reference's backprop) against the oracle's fp64 forward /
    backward with torch's fp64 Adam in the same loop."""
    from oracle import egnn_oracle as orc
    data = _graphs([(30, _random_graph(30, 0.3, 31)), (25, _random_graph(25, 0.3, 32))])
    kwargs = dict(ALL_ON, k=32)
    model = _model(kwargs, save_path=tmp_path)
    names = [n for n, _ in model.named_parameters()]
    ref = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in model.named_parameters()}
    opt = torch.optim.Adam([ref[n] for n in names], lr=2e-3, weight_decay=1e-4)
    batch = _batch_fn(*data)()
    losses = model.train_model([batch] * 5, epochs=1)
    cfg = dict(kwargs, _class='SartorrasEGNN')
    x, pos, ei, attr, b, y = data
    ref_losses = []
    for _ in range(5):
        y_pred = orc.model_forward(ref, cfg, x, pos, ei, attr, b).reshape(-1)
        loss = orc.loss_fn(cfg, y_pred, y.double())
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_value_([ref[n] for n in names], 1.0)
        opt.step()
        ref_losses.append(float(loss.detach()))
    got_losses = [float(v) for v in losses]
    assert len(got_losses) == 5
    _check(np.array(got_losses), np.array(ref_losses), 'losses')
    for n, p in model.named_parameters():
        assert p.dtype == torch.float64
        _check(p, ref[n], f'param {n} after 5 steps')


def test_mixed_dtypes_and_unbuilt_fp64_paths_raise(tmp_path):
    from pointvs_amd import functional as PF
    from pointvs_amd.screening import ReceptorScreen
    data = _graphs([(20, _random_graph(20, 0.3, 41))])
    model = _model(dict(ALL_ON, k=32), save_path=tmp_path)
    feats, edges, coords, eattr, b = model.unpack_graph(_batch_fn(*data)())
    layer = model.layers[1]
    h = model.layers[0].embed(feats, coords)
    with pytest.raises(TypeError, match='mixed dtypes'):
        layer(h.float(), edges, coords, edge_attr=eattr)
    with pytest.raises(TypeError, match='mixed dtypes'):
        layer(h, edges, coords.float(), edge_attr=eattr)
    with pytest.raises(TypeError, match='mixed dtypes'):
        PF.linear(feats, layer.node_mlp[3].weight.float())
    with pytest.raises(NotImplementedError):
        ReceptorScreen(model, coords[5:].float(), torch.ones(20, 12, device='cuda'), 5, 4, 6.0)
    with pytest.raises(NotImplementedError, match='capture'):
        model.train_model([_batch_fn(*data)()], epochs=1, capture=True)


def test_point_vs_entry_trains_and_predicts_in_fp64(tmp_path):
    spec = importlib.util.spec_from_file_location('pvs_entry', ROOT / 'point_vs.py')
    entry = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(entry)
    try:
        model = entry.main(['egnn', str(tmp_path / 'run'), '--synthetic_graphs', '12', '--synthetic_atoms', '150',
                            '-ep', '1', '--layers', '2', '-b', '4', '--edge_radius', '6', '--double'])
    finally:
        torch.set_default_dtype(torch.float32)
    assert all(p.dtype == torch.float64 for p in model.parameters())
    ckpt = tmp_path / 'run' / 'checkpoints' / 'pose_ckpt_epoch_1.pt'
    state = torch.load(ckpt, map_location='cpu', weights_only=False)
    floats = [v for v in state['model_state_dict'].values() if v.is_floating_point()]
    assert floats and all(v.dtype == torch.float64 for v in floats)
    assert (tmp_path / 'run' / 'pose_predictions.txt').read_text().count('\n') == 12


@pytest.mark.parametrize('call, other', [(torch.float32, torch.float64), (torch.float64, torch.float32)],
                         ids=['f64_into_f32', 'f32_into_f64'])
def test_each_operator_refuses_the_other_dtype_forward_and_backward(call, other, tmp_path):
    """One wrapper per operator over functional.KINDS: a tensor of the `other` dtype in a `call`-dtype call is a TypeError
    from the one contiguity-and-dtype helper, in the forward and - called directly, as autograd itself would cast the
    gradient first - in every backward: never a launch on memory of the wrong width."""
    from pointvs_amd import functional as PF
    from pointvs_amd.graph import prepared_for
    data = _graphs([(20, _random_graph(20, 0.3, 41))])
    model = _model(dict(ALL_ON, k=16), save_path=tmp_path).to(call)
    feats, edges, coords, eattr, _ = model.unpack_graph(_batch_fn(*data)())
    first, second = model.layers[1], model.layers[2]
    h = model.layers[0].embed(feats, coords)
    assert h.dtype == call and coords.dtype == call
    h1, x1, _, m1 = first(h, edges, coords, edge_attr=eattr)
    assert (h1.dtype, x1.dtype, m1.dtype) == (call, call, call)

    def refused():
        return pytest.raises(TypeError, match='mixed dtypes')

    # forward: the layer's coordinates and previous messages, linear's weight and bias
    with refused():
        first(h, edges, coords.to(other), edge_attr=eattr)
    with refused():
        second(h1, edges, x1, edge_attr=eattr, edge_messages=m1.to(other))
    gen = torch.Generator().manual_seed(5)
    x = torch.randn(20, 8, generator=gen).to('cuda', call).requires_grad_()
    w = torch.randn(8, 8, generator=gen).to('cuda', call).requires_grad_()
    bias = torch.randn(8, generator=gen).to('cuda', call).requires_grad_()
    with refused():
        PF.linear(x, w.to(other))
    with refused():
        PF.linear(x, w, bias.to(other))
    # either dtype is taken and returned
    graph_ptr = torch.tensor([0, 7, 20], dtype=torch.int32, device='cuda')
    ids = torch.randint(0, 5, (20,), generator=gen).cuda()
    pg = prepared_for(edges, eattr, feats.size(0))
    rows = torch.randn(edges.shape[1], 8, generator=gen).to('cuda', call).requires_grad_()
    outs = {'linear': PF.linear(x, w, bias), 'mean_pool': PF.mean_pool(x, graph_ptr),
            'segment_sum': PF.segment_reduce(x, ids, 5), 'segment_mean': PF.segment_reduce(x, ids, 5, mean=True),
            'rows_to_sorted_order': PF.rows_to_sorted_order(rows, pg), 'rows_to_input_order': PF.rows_to_input_order(rows, pg)}
    for name, y in outs.items():
        assert y.dtype == call, name
    assert torch.equal(PF.rows_to_input_order(outs['rows_to_sorted_order'], pg), rows)
    # fp32 only
    if call == torch.float64:
        with pytest.raises(TypeError, match='fp32 only'):
            PF.pool_head(x, graph_ptr, w, bias)
        with pytest.raises(TypeError, match='fp32 only'):
            PF.bce_with_logits_mean(x[:, 0], torch.ones(20, device='cuda', dtype=call))
    else:
        assert PF.pool_head(x, graph_ptr, w, bias).dtype == call
        assert PF.bce_with_logits_mean(x[:, 0], torch.ones(20, device='cuda')).dtype == call
        with pytest.raises(TypeError, match='fp32 only'):
            PF.pool_head(x.to(other), graph_ptr, w, bias)
        with pytest.raises(TypeError, match='fp32 only'):
            PF.bce_with_logits_mean(x[:, 0].to(other), torch.ones(20, device='cuda', dtype=other))
    # backward: a correct forward in `call`, its backward handed a gradient of `other`
    for name, y in outs.items():
        with refused():
            y.grad_fn.apply(torch.ones_like(y, dtype=other))
    node = h1.grad_fn                   # the layer's own node: (h_out, x_out, m_out, att, node_att)
    assert type(node).__name__ == '_EGNNLayerFnBackward'
    with refused():
        node.apply(torch.ones_like(h1, dtype=other), None, None, None, None)
    with refused():
        node.apply(torch.ones_like(h1), torch.ones_like(x1, dtype=other), None, None, None)
    # ... and the right dtype still runs, after all the refusals
    g_in = node.apply(torch.ones_like(h1), None, None, None, None)
    assert g_in[0] is None and g_in[1].dtype == call and g_in[1].shape == h.shape
    g_x, g_w, g_b = outs['linear'].grad_fn.apply(torch.ones_like(outs['linear']))
    assert (g_x.dtype, g_w.dtype, g_b.dtype) == (call, call, call)
