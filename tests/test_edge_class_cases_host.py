"""Host-side pins of the edge-class inputs (tests/_edge_class_cases.py): a GPU result on these graphs is a finding only
while the graphs have the shape the GPU tests rely on, and while the oracle depends on the class columns the way the
layer definition says. No GPU."""
import numpy as np
import pytest
import torch

from tests import _edge_class_cases as ecc


@pytest.mark.parametrize('odd', [False, True])
@pytest.mark.parametrize('A', ecc.CLASS_COUNTS)
def test_class_graph_has_the_promised_shape(A, odd):
    g = ecc.class_graph(A, seed=100 + A, odd_edges=odd)
    ei = g.edge_index.numpy()
    e = ei.shape[1]
    assert g.edge_index.dtype == torch.int64 and g.pos.shape == (ecc.N_NODES, 3) and g.pos.dtype == torch.float32
    assert e == ecc.N_RANDOM + ecc.HUB_EDGES + (1 if odd else 0) and e % 2 == (1 if odd else 0)
    assert ei.min() >= 0 and ei.max() < ecc.N_NODES
    assert not (ei[0] == ei[1]).any(), 'self loops make normalize=True ill-conditioned'
    assert not np.isin(ei, ecc.ISOLATED).any() and len(ecc.ISOLATED) == 5
    # the 512-thread forward (8 waves of 64 edges per workgroup) gets several workgroups
    assert e > 4 * 8 * 64
    # the hub: one row whose sorted range spans > 6 tiles of 32 edges, a dozen of 16 and an end of a 64-edge chunk
    d = ecc.prepared_definition(g.edge_index, g.etype, g.n_nodes)
    lo, hi = int(d['rowptr'][ecc.HUB]), int(d['rowptr'][ecc.HUB + 1])
    assert hi - lo >= ecc.HUB_EDGES
    assert (hi - 1) // 32 - lo // 32 >= 6 and (hi - 1) // 16 - lo // 16 >= 12 and (hi - 1) // 64 > lo // 64
    hub_in_input = np.flatnonzero(ei[0] == ecc.HUB)
    assert np.diff(hub_in_input).max() > 1, 'the hub edges are scattered over the input list'
    if A == 0:
        assert g.edge_attr is None and g.etype is None
        return
    et = g.etype.numpy()
    assert g.edge_attr.dtype == torch.int64 and tuple(g.edge_attr.shape) == (e, A)
    assert np.array_equal(g.edge_attr.numpy().argmax(1), et) and (g.edge_attr.sum(1) == 1).all()
    counts = np.bincount(et, minlength=A)
    K = ecc.n_live_classes(A)
    assert (counts[:K] > 0).all() and (counts[K:] == 0).all()
    if A == 8:
        assert counts[7] == 0, 'A = 8 keeps its last class empty'
    if K >= 2:
        assert counts[K - 1] == 1, 'one class has exactly one edge'
    for c in range(1, K - 1):                            # shares fall roughly as 2^-c
        assert 0.25 * counts[c - 1] < counts[c] < 0.8 * counts[c - 1], counts
    assert set(et[hub_in_input]) == set(range(K)), 'the hub row holds every class that has edges'


@pytest.mark.parametrize('odd', [False, True])
@pytest.mark.parametrize('A', [0, 1, 2, 5, 8])
def test_class_runs_keep_the_loader_layout(A, odd):
    from pointvs_amd.graph import runs_layout
    batch, et = ecc.class_runs(A, seed=300, odd_edges=odd)
    e = int(batch.edge_index.shape[1])
    assert batch.edge_layout == 'generate_edges' and e % 2 == (1 if odd else 0)
    assert sum(batch.graph_edge_counts) == e and len(batch.graph_edge_counts) == 3
    assert runs_layout(batch, device='cpu') is not None, 'the host tables match the edge list'
    rows = batch.edge_index[0].numpy()
    start = 0
    for count in batch.graph_edge_counts:                # per graph: at most one descent of the row ids
        r = rows[start:start + count]
        assert int((np.diff(r) < 0).sum()) <= 1
        start += count
    if A == 0:
        assert batch.edge_attr is None and et is None
        return
    counts = np.bincount(et.numpy(), minlength=A)
    K = ecc.n_live_classes(A)
    assert tuple(batch.edge_attr.shape) == (e, A) and (counts[:K] > 0).all() and (counts[K:] == 0).all()
    assert K < 2 or counts[K - 1] == 1


def _oracle(A, hid, flags, g, w1_extra=None):
    """fp64 oracle layer on `g` with A classes (w1_extra: one more weight column and a class that is never hot)."""
    from oracle import egnn_oracle as orc
    gen = torch.Generator().manual_seed(5)
    ld1 = (hid if flags.get('permutation_invariance') else 2 * hid) + 1 + A
    shapes = {'edge_mlp.0.weight': (hid, ld1), 'edge_mlp.0.bias': (hid,), 'edge_mlp.2.weight': (hid, hid),
              'edge_mlp.2.bias': (hid,), 'coord_mlp.0.weight': (hid, hid), 'coord_mlp.0.bias': (hid,),
              'coord_mlp.2.weight': (1, hid), 'node_mlp.0.weight': (hid, 2 * hid), 'node_mlp.0.bias': (hid,),
              'node_mlp.3.weight': (hid, hid), 'node_mlp.3.bias': (hid,), 'att_mlp.0.weight': (1, hid),
              'att_mlp.0.bias': (1,)}
    sd = {'L.' + k: (0.3 * torch.randn(s, generator=gen, dtype=torch.float64)) for k, s in shapes.items()}
    attr = None if g.edge_attr is None else g.edge_attr
    if w1_extra is not None:
        sd['L.edge_mlp.0.weight'] = torch.cat([sd['L.edge_mlp.0.weight'], w1_extra], dim=1)
        zero = torch.zeros((g.edge_index.shape[1], 1), dtype=torch.int64)
        attr = zero if attr is None else torch.cat([attr, zero], dim=1)
    sd = {k: v.requires_grad_(True) for k, v in sd.items()}
    kw = dict(orc.BUILD_NET_DEFAULTS, residual=True, normalize=False, tanh=False, graphnorm=False)
    kw.update(flags)
    kw['edge_attention_here'], kw['node_attention_here'] = kw['edge_attention'], kw['node_attention']
    n, e = g.n_nodes, g.edge_index.shape[1]
    h = torch.randn((n, hid), generator=gen, dtype=torch.float64).requires_grad_(True)
    x = g.pos.double().requires_grad_(True)
    wh, wx, wm = (torch.randn(s, generator=gen, dtype=torch.float64) for s in ((n, hid), (n, 3), (e, hid)))
    h1, x1, m1, att, _ = orc.egnn_layer(sd, 'L.', kw, h, g.edge_index, x, attr, None)
    ((h1 * wh).sum() + (x1 * wx).sum() + (m1 * wm).sum()).backward()
    out = {'h_out': h1, 'x_out': x1, 'm': m1, 'att': att, 'g_h': h.grad, 'g_x': x.grad}
    out.update({'grad ' + k[2:]: v.grad for k, v in sd.items()})
    return {k: v.detach().numpy() for k, v in out.items() if v is not None}


@pytest.mark.parametrize('flags', [dict(), dict(edge_attention=True, permutation_invariance=True)], ids=['plain', 'att_perm'])
@pytest.mark.parametrize('A', ecc.CLASS_COUNTS)
def test_oracle_with_a_never_hot_class_equals_the_oracle_without_it(A, flags):
    """The arbiter depends on the class columns as the layer definition says: class c adds column ld1 - A + c of
    edge_mlp.0.weight to the first layer of the edges of class c and to nothing else. So a further class that no edge
    has changes nothing, whatever its weight column holds, and that column's gradient is zero."""
    hid = 16
    g = ecc.class_graph(A, seed=100 + A)
    extra = 3.0 * torch.randn((hid, 1), generator=torch.Generator().manual_seed(9), dtype=torch.float64)
    a, b = _oracle(A, hid, flags, g), _oracle(A, hid, flags, g, w1_extra=extra)
    assert set(a) == set(b)
    for key in a:
        got, ref = b[key], a[key]
        if key == 'grad edge_mlp.0.weight':
            assert got.shape[1] == ref.shape[1] + 1 and not got[:, -1].any()
            got = got[:, :-1]
        scale = float(np.abs(ref).max())
        assert scale > 0 and float(np.abs(got - ref).max()) <= 1e-12 * scale, key
    # and the columns are live: the gradient of every class that has edges is non-zero, an empty class's is zero
    w1g = a['grad edge_mlp.0.weight']
    for c in range(A):
        assert bool(np.abs(w1g[:, w1g.shape[1] - A + c]).max() > 0) == (c < ecc.n_live_classes(A)), c
