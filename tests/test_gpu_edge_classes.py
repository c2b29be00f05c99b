"""EGNNLayer, graph preparation and edge dropout with 0 ... 8 edge classes (the rest of the suite runs 3 only).

The class count A changes which code runs: the 512-thread H = 64 forward (A > 3), an MFMA forward with a generic
backward over one `saved` buffer (A > 3), the row stride ld1 = (H or 2H) + 1 + A of edge_mlp.0.weight (a multiple of 4
only at A = 3), the class columns of its gradient (fixed slots in the MFMA backward, eight accumulators in the generic
one, three scalars in fp64), a null etype pointer (A = 0), the one-hot decoders of the graph preparation.

Arbiter: autograd on the fp64 oracle layer (oracle/egnn_oracle.py). Bound: tests/_golden.py assert_strict with at
least three fp32 oracle draws (two under edge permutations); fp64 layers: the bound of tests/test_gpu_fp64.py.
Inputs: tests/_edge_class_cases.py, pinned by tests/test_edge_class_cases_host.py.
"""
import contextlib
import functools
import os

import numpy as np
import pytest
import torch

from tests import _edge_class_cases as ecc
from tests._golden import CaseLog, assert_strict, edge_permutations, grad_floor

pytestmark = pytest.mark.gpu

FLAGS = {
    'plain': dict(),
    'full': dict(edge_residual=True, gated_residual=True, residual=True, edge_attention=True, node_attention=True,
                 normalize=True, tanh=True, graphnorm=True),
    'soft': dict(edge_attention=True, softmax_attention=True, residual=True),
    'perm': dict(permutation_invariance=True),            # ld1 = H + 1 + A
    # the node-side kinds of tests/test_gpu_node_side.py (`node_gate`: the value _new_layer gives node_gate_parameter)
    'nores': dict(residual=False),
    'gn': dict(graphnorm=True),
    'natt-sigmoid': dict(node_attention=True, attention_activation_fn='sigmoid'),
    'natt-tanh': dict(node_attention=True, attention_activation_fn='tanh'),
    'natt-relu': dict(node_attention=True, attention_activation_fn='relu'),
    'natt-silu': dict(node_attention=True, attention_activation_fn='silu'),
    'rezero0': dict(residual=True, rezero=True, node_attention=True, node_gate=0.0),     # what every rezero model starts from
    'rezero': dict(residual=True, rezero=True, node_attention=True, node_gate=0.35),
    'gated+': dict(residual=True, gated_residual=True, node_gate=0.6),
    'gated0': dict(residual=True, gated_residual=True, node_gate=0.0),
    'gated-': dict(residual=True, gated_residual=True, node_gate=-0.3),
    'eatt-tanh': dict(edge_attention=True, node_attention=True, attention_activation_fn='tanh'),
    'eatt-relu': dict(edge_attention=True, node_attention=True, attention_activation_fn='relu'),
    'eatt-silu': dict(edge_attention=True, node_attention=True, attention_activation_fn='silu'),
}
FAMILY_ENV = {'default': {}, 'exact': {'PVS_EGNN_BF16X3': '0'}, 'generic': {'PVS_EGNN_KERNELS': 'generic'}}


def _cell(group, A, hid, family='default', flags='plain', grad=True, env=None, route='fused'):
    tag = f'{group}-A{A}-H{hid}-{family}-{flags}-{"grad" if grad else "nograd"}'
    if env:
        tag += '-' + '-'.join(f'{k}={v}' for k, v in env.items())
    return pytest.param(dict(group=group, A=A, hid=hid, family=family, flags=flags, grad=grad, env=env or {}, route=route,
                             tag=tag), id=tag)


def _cells():
    out = []
    # (a) the 512-thread H = 64 forward (A > 3, default family), with and without softmax, no_grad and with gradients
    for A in (4, 5, 8):
        for flags in ('plain', 'soft'):
            for grad in (False, True):
                out.append(_cell('a', A, 64, 'default', flags, grad))
    # (b) MFMA forward + generic backward: A in {4, 8} x H in {32, 64} x {default, exact}; all four flag sets at H = 32
    for flags in ('plain', 'full', 'soft', 'perm'):
        out += [_cell('b', 4, 32, 'default', flags), _cell('b', 4, 32, 'exact', flags)]
    out += [_cell('b', 8, 32, 'default', 'full'), _cell('b', 8, 32, 'exact', 'plain'), _cell('b', 4, 64, 'default', 'full'), _cell('b', 4, 64, 'exact', 'full'), _cell('b', 8, 64, 'default', 'perm'),
            _cell('b', 8, 64, 'exact', 'perm')]
    # (c) fewer than 3 classes: all four flag sets in the default family, the plain set in the other two
    for A in (0, 1, 2):
        for hid in (32, 64):
            for flags in ('plain', 'full', 'soft', 'perm'):
                out.append(_cell('c', A, hid, 'default', flags))
            out += [_cell('c', A, hid, 'exact', 'plain'), _cell('c', A, hid, 'generic', 'plain')]
    # (d) the 64-bit-offset instantiation of the 512-thread forward
    out.append(_cell('d', 5, 64, 'default', 'soft', env={'PVS_FWD_SADDR': '0'}))
    # (e) hidden 48, zero-padded to 64
    out += [_cell('e', 0, 48, 'default', 'full'), _cell('e', 5, 48, 'default', 'full')]
    # (f) hidden 100 on the fused wide kernels (up to 3 classes), (g) hidden 100 with 5 classes: the decomposed layer
    out.append(_cell('f', 2, 100, 'default', 'full'))
    out.append(_cell('g', 5, 100, 'default', 'full', route='decomposed'))
    # hidden 128 with 5 classes does not raise: it takes the decomposed route as well
    out.append(_cell('wide128', 5, 128, 'default', 'plain', route='decomposed'))
    # control: three classes
    out.append(_cell('control', 3, 64, 'default', 'full'))
    # H = 16 runs the generic kernels whatever the family; the generic family at H = 32 / 64 with more than 3 classes
    for A, flags in ((0, 'full'), (1, 'perm'), (2, 'soft'), (4, 'plain'), (5, 'full'), (8, 'soft')):
        out.append(_cell('h16', A, 16, 'default', flags))
    out += [_cell('generic', 5, 64, 'generic', 'full'), _cell('generic', 8, 32, 'generic', 'perm'),
            _cell('perm', 5, 64, 'default', 'perm')]
    return out


CELLS = _cells()
REQUIRED_ABC = [c for c in CELLS if c.values[0]['group'] in ('a', 'b', 'c')]


@contextlib.contextmanager
def _environment(cell):
    """The family switches are read by the library at every call (edge_dispatch.h)."""
    env = dict(FAMILY_ENV[cell['family']], **cell['env'])
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _new_layer(A, hid, flags, seed, node_gate=None):
    """A layer with every parameter away from its symmetric initial value: gates 0.7 / 0.6 instead of 0.5 (a swap of
    gate and 1 - gate would not show), GraphNorm's (1, 0, 1) perturbed, the last coordinate weight (Xavier gain 0.001)
    a hundred times larger so that the coordinate update is not lost beside the coordinates.
    node_gate: another value for node_gate_parameter (default: the flag set's `node_gate` entry, else 0.6)."""
    from pointvs_amd.egnn_satorras import EGNNLayer
    flags = dict(flags)
    gate = flags.pop('node_gate', 0.6)
    node_gate = gate if node_gate is None else node_gate
    torch.manual_seed(seed)
    layer = EGNNLayer(hid, hid, hid, edges_in_d=A, **flags)
    gen = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        layer.coord_mlp[2].weight.mul_(100.0)
        if flags.get('graphnorm'):
            for p in layer.node_mlp[1].parameters():
                p.add_(0.2 * torch.randn(p.shape, generator=gen))
        if hasattr(layer, 'edge_gate_parameter'):
            layer.edge_gate_parameter.fill_(0.7)
        if hasattr(layer, 'node_gate_parameter'):
            layer.node_gate_parameter.fill_(node_gate)
    return layer


class Problem:
    """Inputs and oracle references of a chain of `depth` layers on the A-class graph: built once per (A, hid, flags,
    depth) and shared, unchanged, by every test that needs it. `graph`: another graph with A classes in its place
    (tests/test_gpu_edge_partitions.py)."""

    def __init__(self, A, hid, flags_name, depth=1, graph=None):
        self.A, self.hid, self.flags, self.depth = A, hid, FLAGS[flags_name], depth
        self.g = ecc.class_graph(A, seed=100 + A) if graph is None else graph
        n, e = self.g.n_nodes, int(self.g.edge_index.shape[1])
        self.sds = [{k: v.detach().clone() for k, v in _new_layer(A, hid, self.flags, 11 + 7 * d).state_dict().items()}
                    for d in range(depth)]
        gen = torch.Generator().manual_seed(5 + A)
        self.h0, self.m0, self.wh, self.wx, self.wm = (
            torch.randn(s, generator=gen) for s in ((n, hid), (e, hid), (n, hid), (n, 3), (e, hid)))
        self.ref64 = self.oracle(torch.float64)
        self.ref32 = [self.oracle(torch.float32)] + [self.oracle(torch.float32, perm)
                                                     for perm in edge_permutations(e, count=2)]
        self.floor = grad_floor({k: v for k, v in self.ref64.items() if k.startswith('grad ')})

    @staticmethod
    def param_key(depth_index, name):
        return f'grad {name}' if depth_index == 0 else f'grad layer{depth_index + 1}.{name}'

    def oracle(self, dtype, perm=None):
        """Every compared tensor as numpy, edge tensors in the caller's edge order (a permuted draw is put back)."""
        from oracle import egnn_oracle as orc
        kw = dict(orc.BUILD_NET_DEFAULTS, residual=True, normalize=False, tanh=False, graphnorm=False)  # EGNNLayer's defaults
        kw.update(self.flags)
        kw['edge_attention_here'], kw['node_attention_here'] = kw['edge_attention'], kw['node_attention']
        ei, ea, m0, wm = self.g.edge_index, self.g.edge_attr, self.m0, self.wm
        if perm is not None:
            ei, m0, wm = ei[:, perm], m0[perm], wm[perm]
            ea = None if ea is None else ea[perm]

        def back(t):
            if perm is None:
                return t
            out = torch.empty_like(t)
            out[perm] = t
            return out

        def leaf(t):       # (a copy: .to() of the same dtype would hand the shared tensor itself to autograd)
            return t.detach().to(dtype).clone().requires_grad_(True)

        sd = {f'L{d}.{k}': leaf(v) for d, s in enumerate(self.sds) for k, v in s.items()}
        h0, x0, mp = leaf(self.h0), leaf(self.g.pos), leaf(m0)
        h, x, m = h0, x0, mp
        res = {}
        for d in range(self.depth):
            h, x, m, att, natt = orc.egnn_layer(sd, f'L{d}.', kw, h, ei, x, ea, m)
            if d == self.depth - 1:
                if att is not None:
                    res['att'] = back(att)
                if natt is not None:
                    res['natt'] = natt
        ((h * self.wh.to(dtype)).sum() + (x * self.wx.to(dtype)).sum() + (m * wm.to(dtype)).sum()).backward()
        res.update(h_out=h, x_out=x, m=back(m), g_h=h0.grad, g_x=x0.grad)
        if self.flags.get('edge_residual'):
            res['g_m_prev'] = back(mp.grad)
        for d, s in enumerate(self.sds):
            for k in s:
                assert sd[f'L{d}.{k}'].grad is not None, k
                res[self.param_key(d, k)] = sd[f'L{d}.{k}'].grad
        return {k: v.detach().numpy() for k, v in res.items()}

    def gpu(self, grad=True, dtype=torch.float32):
        """The same through EGNNLayer.forward (reference signature) on the device; a fresh layer per call."""
        layers = []
        for d, s in enumerate(self.sds):
            layer = _new_layer(self.A, self.hid, self.flags, 11 + 7 * d)
            layer.load_state_dict(s)
            layers.append(layer.to(dtype).cuda())
        ei = self.g.edge_index.cuda()
        ea = None if self.g.edge_attr is None else self.g.edge_attr.cuda()
        h0, x0, mp = (t.detach().to(dtype).cuda().requires_grad_(grad) for t in (self.h0, self.g.pos, self.m0))
        res = {}
        with torch.enable_grad() if grad else torch.no_grad():
            h, x, m = h0, x0, mp
            for layer in layers:
                h, x, ea_out, m = layer(h, ei, x, ea, m)
                assert ea_out is ea and m.shape == self.m0.shape
            res.update(h_out=h, x_out=x, m=m)
            if layers[-1].att_val is not None:
                res['att'] = torch.as_tensor(layers[-1].att_val)
            if layers[-1].node_att_val is not None:
                res['natt'] = torch.as_tensor(layers[-1].node_att_val)
            if grad:
                ((h * self.wh.to(dtype).cuda()).sum() + (x * self.wx.to(dtype).cuda()).sum()
                 + (m * self.wm.to(dtype).cuda()).sum()).backward()
                res.update(g_h=h0.grad, g_x=x0.grad)
                if self.flags.get('edge_residual'):
                    res['g_m_prev'] = mp.grad
                for d, layer in enumerate(layers):
                    for name, p in layer.named_parameters():
                        assert p.grad is not None, name
                        res[self.param_key(d, name)] = p.grad
        torch.cuda.synchronize()
        return {k: v.detach().cpu().numpy() for k, v in res.items()}

    def class_columns(self, key):
        """(label, column) of the 1 + A trailing columns of an edge_mlp.0.weight gradient: rho, then one per class."""
        width = self.ref64[key].shape[1]
        return [('rho', width - self.A - 1)] + [(f'class {c}', width - self.A + c) for c in range(self.A)]

    def check(self, got, tag, grad=True):
        log = CaseLog(tag)
        outputs = [k for k in self.ref64 if not k.startswith('g')]
        grads = [k for k in self.ref64 if k.startswith('g')] if grad else []
        assert set(got) == set(outputs + grads), sorted(set(got) ^ set(outputs + grads))
        for key in outputs + grads:
            floor = self.floor if key in grads else 0.0
            ref64, ref32 = self.ref64[key], [r[key] for r in self.ref32]
            assert got[key].dtype == np.float32
            value = got[key].reshape(ref64.shape)
            assert_strict(value, ref64, ref32, f'{tag} {key}', floor=floor, log=log)
            if key.endswith('edge_mlp.0.weight'):
                # each trailing column as a tensor of its own: the column of a rare class is orders of magnitude below
                # the matrix maximum and would hide behind it
                for label, c in self.class_columns(key):
                    assert_strict(value[:, c], ref64[:, c], [r[:, c] for r in ref32], f'{tag} {key}[:, {label}]',
                                  floor=floor, log=log)
                    if label.startswith('class') and int(label.split()[1]) >= ecc.n_live_classes(self.A):
                        assert not ref64[:, c].any()
                        if value[:, c].any():
                            log.failures.append(f'{tag} {key}[:, {label}]: the column of a class without edges is not 0.0')
        log.finish()


@functools.lru_cache(maxsize=None)
def problem(A, hid, flags_name, depth=1):
    return Problem(A, hid, flags_name, depth)


@contextlib.contextmanager
def _route_counter():
    """Counts the calls of EGNNLayer._decomposed_call (the layer as the composition of its public sub-methods)."""
    from pointvs_amd.egnn_satorras import EGNNLayer
    calls = []
    real = EGNNLayer._decomposed_call

    def counted(self, *args, **kwargs):
        calls.append(self.hidden_nf)
        return real(self, *args, **kwargs)
    EGNNLayer._decomposed_call = counted
    try:
        yield calls
    finally:
        EGNNLayer._decomposed_call = real


@pytest.mark.parametrize('cell', CELLS)
def test_layer_with_a_classes_matches_the_fp64_oracle(cell):
    """Outputs (h, coord, messages in the caller's edge order, att_val / node_att_val), input gradients and every
    parameter gradient of one EGNNLayer.forward, under the strict bound; the rho column and every class column of
    edge_mlp.0.weight.grad on their own as well, the column of a class without edges exactly 0."""
    p = problem(cell['A'], cell['hid'], cell['flags'])
    with _environment(cell), _route_counter() as decomposed:
        got = p.gpu(grad=cell['grad'])
    assert bool(decomposed) == (cell['route'] == 'decomposed'), (cell['route'], decomposed)
    p.check(got, cell['tag'], grad=cell['grad'])


@pytest.mark.parametrize('cell', REQUIRED_ABC)
def test_layer_with_a_classes_is_bitwise_reproducible(cell):
    p = problem(cell['A'], cell['hid'], cell['flags'])
    with _environment(cell):
        first, second = p.gpu(grad=cell['grad']), p.gpu(grad=cell['grad'])
    assert set(first) == set(second)
    differing = [k for k in first if first[k].tobytes() != second[k].tobytes()]
    assert not differing, differing


@pytest.mark.parametrize('A', [0, 5])
def test_two_chained_layers_with_edge_residual(A):
    """layer2(h1, ei, x1, ea, m1) with gradients through both (H = 32, gated edge residual, attention): the messages
    and g_m_prev pass between the layers - at A = 5 between a generic backward and an MFMA forward."""
    p = problem(A, 32, 'full', 2)
    p.check(p.gpu(), f'chain-A{A}-H32-default-full-grad')


# ---- fp64 ---------------------------------------------------------------------------------------------------------------
def _check64(p, got, tag):
    from tests.test_gpu_fp64 import _check
    g_max = max(float(np.abs(v).max()) for k, v in p.ref64.items() if k.startswith('grad '))
    assert set(got) == set(p.ref64)
    for key, ref in p.ref64.items():
        assert got[key].dtype == np.float64, key
        _check(got[key], ref, f'{tag} {key}', g_max if key.startswith('g') else 0.0)
        if key.endswith('edge_mlp.0.weight'):
            for label, c in p.class_columns(key):
                _check(got[key][:, c], ref[:, c], f'{tag} {key}[:, {label}]', g_max)


@pytest.mark.parametrize('hid,flags', [(32, 'full'), (16, 'soft')])
@pytest.mark.parametrize('A', [0, 1, 2])
def test_fp64_layer_with_fewer_than_three_classes(A, hid, flags):
    p = problem(A, hid, flags)
    _check64(p, p.gpu(dtype=torch.float64), f'fp64-A{A}-H{hid}-{flags}')


def test_fp64_layer_refuses_more_than_three_classes_and_stays_usable():
    """layer_f64.hip holds three class scalars behind a REQUIRE(n_edge_attr <= 3): four classes raise from the forward's
    check, before any kernel runs, and the A = 3 call right after it is correct."""
    p4 = problem(4, 32, 'full')
    for grad in (False, True):
        with pytest.raises(RuntimeError, match=r'n_edge_attr=4 \(0\.\.3 built\)'):
            p4.gpu(grad=grad, dtype=torch.float64)
    p3 = problem(3, 32, 'full')
    _check64(p3, p3.gpu(dtype=torch.float64), 'fp64-A3-H32-full')


# ---- refusals -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grad', [False, True])
def test_nine_classes_raise_from_the_layer_call(grad):
    from pointvs_amd.egnn_satorras import EGNNLayer
    g = ecc.class_graph(8, seed=108)
    layer = EGNNLayer(32, 32, 32, edges_in_d=9).cuda()
    ea = torch.nn.functional.one_hot(g.etype, 9).cuda()
    h = torch.randn(g.n_nodes, 32).cuda().requires_grad_(grad)
    with torch.enable_grad() if grad else torch.no_grad():
        with pytest.raises(RuntimeError, match=r'n_edge_attr 9 unsupported \(0\.\.8\)'):
            layer(h, g.edge_index.cuda(), g.pos.cuda(), ea)


def test_edge_attr_of_another_width_raises():
    from pointvs_amd.egnn_satorras import EGNNLayer
    g = ecc.class_graph(5, seed=105)
    h, ei, x, ea = torch.randn(g.n_nodes, 32).cuda(), g.edge_index.cuda(), g.pos.cuda(), g.edge_attr.cuda()
    with pytest.raises(ValueError, match='layer built with edges_in_d=3 but edge_attr has 5 columns'):
        EGNNLayer(32, 32, 32, edges_in_d=3).cuda()(h, ei, x, ea)
    with pytest.raises(ValueError, match='layer built with edges_in_d=0, edge_attr given'):
        EGNNLayer(32, 32, 32).cuda()(h, ei, x, ea)
    with pytest.raises(ValueError, match='layer built with edges_in_d=5, edge_attr missing'):
        EGNNLayer(32, 32, 32, edges_in_d=5).cuda()(h, ei, x, None)


@pytest.mark.parametrize('path', ['sort', 'runs'])
@pytest.mark.parametrize('ones', [0, 2])
def test_rows_that_are_not_one_hot_raise_through_the_status_word(path, ones):
    from pointvs_amd.graph import prepare_graph, runs_layout
    batch, _ = ecc.class_runs(5, seed=300)
    e, n = int(batch.edge_index.shape[1]), int(batch.x.shape[0])
    assert e % 2 == 0
    for victim in (0, 2 * (e // 4) + 1, e - 1):           # the first edge of a pair, the second of one, the last edge
        ea = batch.edge_attr.clone()
        ea[victim] = 0
        if ones == 2:
            ea[victim, 1] = ea[victim, 4] = 1
        layout = runs_layout(batch, device='cuda') if path == 'runs' else None
        assert (layout is not None) == (path == 'runs')
        pg = prepare_graph(batch.edge_index.cuda(), ea.cuda(), n, need_backward=True, layout=layout)
        with pytest.raises(ValueError, match='one-hot'):
            pg.check_status()
    good = prepare_graph(batch.edge_index.cuda(), batch.edge_attr.cuda(), n, need_backward=True, layout=layout)
    good.check_status()


# ---- graph preparation and edge dropout ---------------------------------------------------------------------------------
def _assert_prepared(pg, want, A):
    pg.check_status()
    e = pg.n_edges
    for name in ('rowptr', 'row', 'col', 'perm', 'colptr', 'cedge', 'inv_deg'):
        got = pg.t[name].cpu().numpy()
        got = got[:e] if name in ('row', 'col', 'perm', 'cedge') else got
        assert np.array_equal(got, want[name]), name
    if A == 0:
        assert 'etype' not in pg.t and not pg.c.etype
    else:
        assert pg.t['etype'].dtype == torch.uint8
        assert np.array_equal(pg.t['etype'].cpu().numpy()[:e], want['etype']), 'etype'


@pytest.mark.parametrize('odd', [False, True], ids=['even', 'odd'])
@pytest.mark.parametrize('path', ['sort', 'runs'])
@pytest.mark.parametrize('A', [0, 1, 2, 5, 8])
def test_prepared_graph_with_a_classes_equals_its_definition(A, path, odd):
    """rowptr, row, col, etype, perm, inv_deg, colptr, cedge of pvs_graph_prepare (sort) and pvs_graph_prepare_runs
    (merge: 16-byte loads of the one-hot rows at even E, scalar loads at odd E), each against numpy's stable sorts."""
    from pointvs_amd.graph import prepare_graph, runs_layout
    if path == 'sort':
        g = ecc.class_graph(A, seed=100 + A, odd_edges=odd)
        ei, ea, et, n, layout = g.edge_index, g.edge_attr, g.etype, g.n_nodes, None
    else:
        batch, et = ecc.class_runs(A, seed=300, odd_edges=odd)
        ei, ea, n = batch.edge_index, batch.edge_attr, int(batch.x.shape[0])
        layout = runs_layout(batch, device='cuda')
        assert layout is not None
    assert int(ei.shape[1]) % 2 == int(odd)
    pg = prepare_graph(ei.cuda(), None if ea is None else ea.cuda(), n, need_backward=True, layout=layout)
    _assert_prepared(pg, ecc.prepared_definition(ei, et, n), A)


@pytest.mark.parametrize('A', [0, 1, 5])
def test_edge_dropout_with_a_classes(A):
    """PF.dropout_adj on a duplicate-free list: the survivors are row <= col input edges, the second half holds their
    reverses, every survivor carries the class of its own (row, col), and the drawn subset is the one drawn with three
    classes on the same list, seed and step (the draw does not look at the attributes)."""
    from pointvs_amd import functional as PF
    g = ecc.class_graph(max(A, 1), seed=100 + A)
    n = g.n_nodes
    keys = (g.edge_index[0] * n + g.edge_index[1]).numpy()
    _, first = np.unique(keys, return_index=True)
    first = np.sort(first)
    ei = g.edge_index[:, first].contiguous()
    et = g.etype[first]
    ea = None if A == 0 else torch.nn.functional.one_hot(et, A)
    ea3 = torch.nn.functional.one_hot(torch.arange(ei.shape[1]) % 3, 3)
    class_of = dict(zip(keys[first].tolist(), et.tolist()))
    oi, oa = PF.dropout_adj(ei.cuda(), None if ea is None else ea.cuda(), 0.3, training=True, seed=5, step=1)
    oi3, oa3 = PF.dropout_adj(ei.cuda(), ea3.cuda(), 0.3, training=True, seed=5, step=1)
    assert torch.equal(oi, oi3)
    k = oi.shape[1] // 2
    cand = int((ei[0] <= ei[1]).sum())
    assert 0 < k < cand and oi.shape[1] == 2 * k and abs(k / cand - 0.7) < 4 * np.sqrt(0.21 / cand) + 1e-3
    assert torch.equal(oi[0, :k], oi[1, k:]) and torch.equal(oi[1, :k], oi[0, k:]), 'kept pairs stay together'
    assert bool((oi[0, :k] <= oi[1, :k]).all())
    out_keys = (oi[0, :k] * n + oi[1, :k]).cpu().tolist()
    assert all(key in class_of for key in out_keys) and len(set(out_keys)) == k
    kept = set(out_keys)
    assert out_keys == [key for key in keys[first].tolist() if key in kept], 'survivors keep the input order'
    if A == 0:
        assert oa is None
        return
    assert oa.dtype == torch.int64 and tuple(oa.shape) == (2 * k, A) and bool((oa.sum(1) == 1).all())
    assert torch.equal(oa[:k], oa[k:])
    assert oa[:k].argmax(1).cpu().tolist() == [class_of[key] for key in out_keys], 'attributes travel with their edges'
