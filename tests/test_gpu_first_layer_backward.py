"""The first-layer backward pair (k_edge_bwd_f16_nogx + k_node_gather_rho, edge_dispatch.h pvs_first_layer_bwd) against
the general pair it replaces when nobody asks for the gradient of a layer's input coordinates.

The pair runs the general kernels' operations in the general kernels' order and only leaves out the per-edge
coordinate gradient, so g_h and every parameter gradient must come out BIT FOR BIT as the general pair gives them
(coord.requires_grad = True on identical inputs): no tolerance. What the first-layer run returns also passes the strict
fp64-oracle bound of tests/test_gpu_edge_classes.py (Problem.check). Which pair ran is read from the library
(pvs_edge_bwd_last_variant): with PVS_EGNN_FIRST_LAYER_BWD=0 the same call gives the same bits through the general pair.

Inputs: the 3,200-edge graphs of tests/_edge_partition_cases.py (hub rows, isolated nodes, empty chunks), H = 32, 0 and 3
edge classes, the plain flag set (coordinates updated), under the default plan and the three PARTITIONS: at this size every
tile-end, graph-end, row-less-node and empty-chunk case of the kernels occurs.
"""
import copy
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _edge_partition_cases as epc
from tests.test_gpu_edge_classes import _new_layer
from tests.test_gpu_edge_partitions import _problem

pytestmark = pytest.mark.gpu

GENERAL, FIRST_LAYER = 0, 1
PLANS = {'default': {}, **epc.PARTITIONS}
SWITCH = 'PVS_EGNN_FIRST_LAYER_BWD'
FALLBACKS = {
    'edge_attention': (32, dict(edge_attention=True, node_attention=True, attention_activation_fn='tanh')),
    'edge_residual_sum': (32, dict(edge_residual=True)),
    'edge_residual_gated': (32, dict(edge_residual=True, gated_residual=True, residual=True)),
    'h64': (64, dict()),
}


def _last_variant():
    from pointvs_amd import _lib
    return _lib.lib().pvs_edge_bwd_last_variant()


def _plan(monkeypatch, plan, switch=None):
    for name in ('PVS_CHUNK_EDGES', 'PVS_EDGES_PER_WAVE', SWITCH):
        monkeypatch.delenv(name, raising=False)
    for k, v in PLANS[plan].items():
        monkeypatch.setenv(k, v)
    if switch is not None:
        monkeypatch.setenv(SWITCH, switch)


def _run(p, coord_grad):
    """One EGNNLayer forward + backward with a live g_x_out, as Problem.gpu runs it, with the coordinates a leaf that
    does (the general pair) or does not (the first-layer pair) require a gradient. Returns (results, variant)."""
    layer = _new_layer(p.A, p.hid, p.flags, 11)
    layer.load_state_dict(p.sds[0])
    layer = layer.cuda()
    ei = p.g.edge_index.cuda()
    ea = None if p.g.edge_attr is None else p.g.edge_attr.cuda()
    h0 = p.h0.detach().cuda().requires_grad_(True)
    x0 = p.g.pos.detach().cuda().requires_grad_(coord_grad)
    mp = p.m0.detach().cuda().requires_grad_(True)
    h, x, _, m = layer(h0, ei, x0, ea, mp)
    res = dict(h_out=h, x_out=x, m=m)
    if layer.att_val is not None:
        res['att'] = torch.as_tensor(layer.att_val)
    if layer.node_att_val is not None:
        res['natt'] = torch.as_tensor(layer.node_att_val)
    ((h * p.wh.cuda()).sum() + (x * p.wx.cuda()).sum() + (m * p.wm.cuda()).sum()).backward()
    variant = _last_variant()
    res['g_h'] = h0.grad
    if coord_grad:
        res['g_x'] = x0.grad
    else:
        assert x0.grad is None
    if p.flags.get('edge_residual'):
        res['g_m_prev'] = mp.grad
    for name, q in layer.named_parameters():
        assert q.grad is not None, name
        res[f'grad {name}'] = q.grad
    torch.cuda.synchronize()
    return {k: v.detach().cpu().numpy() for k, v in res.items()}, variant


def _assert_same_bits(a, b, what):
    keys = [k for k in a if k != 'g_x']
    assert set(keys) == set(k for k in b if k != 'g_x'), what
    differing = [k for k in keys if a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes()]
    assert not differing, (what, differing)


@pytest.mark.parametrize('plan', list(PLANS))
@pytest.mark.parametrize('A', [0, 3])
@pytest.mark.parametrize('graph', list(epc.GRAPHS))
def test_first_layer_pair_gives_the_general_pairs_bits_and_passes_the_oracle_bound(graph, A, plan, monkeypatch):
    p = _problem(graph, A, 32, 'plain')
    _plan(monkeypatch, plan)
    general, v_general = _run(p, coord_grad=True)
    first, v_first = _run(p, coord_grad=False)
    assert (v_general, v_first) == (GENERAL, FIRST_LAYER), 'the calls did not take the pairs this test compares'
    assert 'g_x' in general and 'g_x' not in first
    _assert_same_bits(general, first, f'{graph} A{A} {plan}')
    # the witness: the same call through the general pair (the switch is read at every call) gives those bits too
    _plan(monkeypatch, plan, switch='0')
    off, v_off = _run(p, coord_grad=False)
    assert v_off == GENERAL
    _assert_same_bits(first, off, f'{graph} A{A} {plan} switched off')
    # everything the first-layer run returns, under the strict bound of the edge-class tests (the shared problem and
    # its references stay as they are: the copy only leaves out the one tensor this run does not return)
    q = copy.copy(p)
    q.ref64 = {k: v for k, v in p.ref64.items() if k != 'g_x'}
    q.ref32 = [{k: v for k, v in r.items() if k != 'g_x'} for r in p.ref32]
    q.check(first, f'first-layer {graph}-A{A}-{plan}')


@functools.lru_cache(maxsize=None)
def _fallback_inputs(name):
    """Inputs as Problem draws them (no oracle: these cells compare two runs of the library)."""
    hid, flags = FALLBACKS[name]
    g = epc.graph('mixed', 3)
    n, e = g.n_nodes, int(g.edge_index.shape[1])
    sd = {k: v.detach().clone() for k, v in _new_layer(3, hid, flags, 11).state_dict().items()}
    gen = torch.Generator().manual_seed(8)
    h0, m0, wh, wx, wm = (torch.randn(s, generator=gen) for s in ((n, hid), (e, hid), (n, hid), (n, 3), (e, hid)))
    return SimpleNamespace(A=3, hid=hid, flags=flags, g=g, sds=[sd], h0=h0, m0=m0, wh=wh, wx=wx, wm=wm)


@pytest.mark.parametrize('name', list(FALLBACKS))
def test_layers_outside_the_pair_keep_the_general_kernels(name, monkeypatch):
    """Edge attention, every edge-residual kind the flags alone select and H = 64: coord.requires_grad = False changes
    nothing but the missing g_x - the general pair runs, and gives the bits of its requires_grad = True run."""
    p = _fallback_inputs(name)
    _plan(monkeypatch, 'default')
    with_gx, v1 = _run(p, coord_grad=True)
    without, v2 = _run(p, coord_grad=False)
    assert (v1, v2) == (GENERAL, GENERAL)
    _assert_same_bits(with_gx, without, name)


def _batch_of(names, A=3):
    """Two of the test graphs as one batch of a SartorrasEGNN (12 input features, as tests/test_gpu_properties.py)."""
    from pointvs_amd.graph import Batch
    graphs = [epc.graph(n, A) for n in names]
    rng = np.random.default_rng(17)
    n_total = sum(g.n_nodes for g in graphs)
    x = np.zeros((n_total, 12), dtype=np.float32)
    x[np.arange(n_total), rng.integers(0, 11, n_total)] = 1.0
    x[:, 11] = rng.integers(0, 2, n_total)
    offsets = np.cumsum([0] + [g.n_nodes for g in graphs[:-1]])
    return Batch(
        x=torch.from_numpy(x), pos=torch.cat([g.pos for g in graphs]),
        edge_index=torch.cat([g.edge_index + int(o) for g, o in zip(graphs, offsets)], dim=1),
        edge_attr=torch.cat([g.edge_attr for g in graphs]),
        batch=torch.cat([torch.full((g.n_nodes,), k, dtype=torch.int64) for k, g in enumerate(graphs)]),
        y=torch.ones(len(graphs)), lig_fname=['l'] * len(graphs), rec_fname=['r'] * len(graphs), num_graphs=len(graphs))


def _model_grads(model, g, monkeypatch, stack):
    monkeypatch.setenv('PVS_EGNN_STACK', '1' if stack else '0')
    model.train()
    model.optimiser.zero_grad()
    y = model(g).reshape(-1)
    model.get_loss(torch.ones_like(y), y).backward()
    variant = _last_variant()        # the last layer call of a backward is the model's FIRST layer
    return y.detach().clone(), {n: (None if q.grad is None else q.grad.detach().clone())
                                for n, q in model.named_parameters()}, variant


def test_stack_backward_takes_the_pair_like_the_per_layer_calls(monkeypatch):
    """pvs_egnn_stack_bwd and the per-layer calls reach the selection through the same call: a 3-layer H = 32 model on
    two of the graphs batched gives the same logits and parameter gradients bit for bit both ways, through the first-layer
    pair in its first layer - and the stack gives those bits through the general pair too (the switch)."""
    from tests.test_gpu_properties import make_model
    model, _ = make_model(seed=5, num_layers=3)
    g = _batch_of(('hub_first', 'hub_last')).to('cuda')
    _plan(monkeypatch, 'default')
    runs = {'per layer': _model_grads(copy.deepcopy(model), g, monkeypatch, stack=False)}
    twin = copy.deepcopy(model)
    runs['stack'] = _model_grads(twin, g, monkeypatch, stack=True)
    assert twin.__dict__.get('_stack_cache') is not None, 'the one-call stack did not run'
    _plan(monkeypatch, 'default', switch='0')
    runs['stack, switched off'] = _model_grads(copy.deepcopy(model), g, monkeypatch, stack=True)
    assert [r[2] for r in runs.values()] == [FIRST_LAYER, FIRST_LAYER, GENERAL]
    y0, g0, _ = runs['per layer']
    assert any(v is not None for k, v in g0.items() if k.startswith('layers.1.coord_mlp'))
    for what, (y, grads, _) in runs.items():
        assert torch.equal(y0, y), what
        assert grads.keys() == g0.keys()
        for name in g0:
            if g0[name] is None or grads[name] is None:
                assert g0[name] is None and grads[name] is None, (what, name)
            else:
                assert torch.equal(g0[name], grads[name]), (what, name)
