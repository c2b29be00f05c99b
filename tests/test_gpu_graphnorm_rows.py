"""GraphNorm over a row count that lives on the device (PvsGraph.n_norm_rows_dev), on the GPU.

Operator level (PF.graphnorm_stats -> pvs_graphnorm_stats_rows): at every edge of the row partition - one workgroup, the
steps of rows-per-workgroup, the 512-workgroup cap at 65,536 rows - the statistics of the first n rows of a padded
[N_cap, H] input do not move by a bit when the padding is NaN or 1e30, equal the host-count route on those n rows bit for
bit, and lie within the column-sum bound of tests/_dense_ref.py of the fp64 restatement tests/_graphnorm_rows_ref.py
(pinned without a GPU in tests/test_graphnorm_rows_host.py).

Layer level (EGNNLayer on a PreparedGraph with set_norm_rows, forward and backward through the C ABI): the 207-node
two-graph batch followed by padding rows without edges, against the fp64 oracle on the unpadded graph at the strict
parity bound (tests/_golden.assert_strict), and - with a gradient arriving on the padding rows - against the oracle
with its GraphNorm replaced by the restatement. Then what is refused.
"""
import contextlib
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests import _dense_ref as dref
from tests import _graphnorm_rows_ref as gref
from tests._golden import edge_permutations, grad_floor
from tests.test_gpu_edge_classes import Problem, _new_layer
from tests.test_gpu_edge_dropout import _two_graphs

pytestmark = pytest.mark.gpu

WIDTHS = (16, 32, 64, 128)
N_ROWS = (0, 1, 2, 127, 128, 129, 255, 256, 257, 65535, 65536, 65537, 70000)
BIG_CAP = 70001                  # for the small n: nearly every workgroup of the launch has nothing to do
SMALL_N = 257                    # n up to here also run at BIG_CAP
BASE_ROWS = 70000 + 257
U32 = dref.unit(np.float32)


def _caps(n):
    return [n, n + 1, n + 257] + ([BIG_CAP] if n <= SMALL_N else [])


@functools.lru_cache(maxsize=None)
def _base(hidden):
    """(values [BASE_ROWS, H] on the device, the same on the host, mean_scale on the device and on the host): standard
    normal columns around per-column offsets, mean_scale in [0.5, 1.5]; built once per width, never written."""
    gen = torch.Generator().manual_seed(77 + hidden)
    y = torch.randn(BASE_ROWS, hidden, generator=gen) + 0.5 * torch.randn(hidden, generator=gen)
    ms = 0.5 + torch.rand(hidden, generator=gen)
    return y.cuda(), y.numpy(), ms.cuda(), ms.numpy()


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _word(n):
    return torch.tensor([n], dtype=torch.int32, device='cuda')


@functools.lru_cache(maxsize=None)
def _reference(hidden, n):
    """fp64 statistics of the first n base rows and what the bound needs: the sums of |terms| per column."""
    _, y, _, ms = _base(hidden)
    mean, var = gref.stats(torch.from_numpy(y[:n].astype(np.float64)), torch.from_numpy(ms.astype(np.float64)), n)
    s_mean = np.abs(y[:n]).astype(np.float64).sum(axis=0) / max(n, 1)
    return mean.numpy(), var.numpy(), s_mean


def _assert_within_the_column_sum_bound(stats, hidden, n, what):
    """tests/_dense_ref.py's rule for a column sum of k addends: |got - ref| <= gamma(k + 3) S, S = sum |terms| (here
    divided by n; the + 3 covers the rounding of 1 / n and the scale). The mean is such a sum. The variance is one of
    (y - shift)^2 around the kernel's OWN fp32 shift = fl(mean_gpu * mean_scale): each addend is the square of a rounded
    difference, two more roundings per addend (gamma(k + 5)); and moving the shift by delta moves the variance of the
    reference by -2 delta (mean - shift) + delta^2, delta <= the mean's bound * |mean_scale| + u |shift| (the product's
    rounding)."""
    _, y, _, ms = _base(hidden)
    mean64, var64, s_mean = _reference(hidden, n)
    got = stats.detach().cpu().numpy().astype(np.float64)
    assert np.all(np.isfinite(got)), what
    b_mean = dref.gamma(n + 3, U32) * s_mean
    err = np.abs(got[:hidden] - mean64)
    assert np.all(err <= b_mean), (what, 'mean', float(err.max()), float(b_mean.max()))
    ms64 = ms.astype(np.float64)
    shift64 = mean64 * ms64
    delta = b_mean * np.abs(ms64) + U32 * np.abs(shift64)
    s_var = ((y[:n].astype(np.float64) - shift64) ** 2).sum(axis=0) / max(n, 1) if n else np.zeros(hidden)
    # (S around a shift within delta of shift64: (|d| + delta)^2 summed)
    s_var = s_var + 2 * delta * np.sqrt(s_var) + delta ** 2
    b_var = dref.gamma(n + 5, U32) * s_var + 2 * delta * np.abs(mean64 - shift64) + delta ** 2
    err = np.abs(got[hidden:] - var64)
    assert np.all(err <= b_var), (what, 'var', float(err.max()), float(b_var.max()))


# ---- B. the operator -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', N_ROWS)
@pytest.mark.parametrize('hidden', WIDTHS)
def test_statistics_of_the_leading_rows(hidden, n):
    from pointvs_amd import functional as PF
    y_dev, _, ms, _ = _base(hidden)
    count = _word(n)
    host = PF.graphnorm_stats(y_dev[:n], ms) if n >= 1 else None        # today's route: host N = n, no count
    for cap in _caps(n):
        what = (hidden, n, cap)
        clean = y_dev[:cap].clone()
        stats = PF.graphnorm_stats(clean, ms, n_rows=count)
        assert stats.shape == (2 * hidden,) and stats.dtype == torch.float32
        for poison in (float('nan'), 1e30):
            padded = clean.clone()
            padded[n:] = poison
            assert np.array_equal(_bits(PF.graphnorm_stats(padded, ms, n_rows=count)), _bits(stats)), (what, poison)
        if n >= 1:
            assert np.array_equal(_bits(stats), _bits(host)), what
            _assert_within_the_column_sum_bound(stats, hidden, n, what)
        else:
            assert not _bits(stats).any(), what           # +0.0 everywhere
            normed = (clean - ms * stats[:hidden]) / (stats[hidden:] + gref.EPS).sqrt()      # rstd = 1 / sqrt(eps)
            assert torch.isfinite(normed).all(), what
    # ten calls in a row, into poisoned outputs: the same bits
    y = y_dev[:_caps(n)[2]]
    first = PF.graphnorm_stats(y, ms, n_rows=count)
    for _ in range(10):
        out = torch.full((2 * hidden,), float('nan'), device='cuda')
        assert PF.graphnorm_stats(y, ms, n_rows=count, out=out) is out
        assert np.array_equal(_bits(out), _bits(first))


def test_the_count_is_read_when_the_kernels_run_and_clamped():
    """One captured-style use: the same call on the same word after the word was rewritten on the stream; a count
    above the capacity or below zero is clamped to it."""
    from pointvs_amd import functional as PF
    y_dev, _, ms, _ = _base(32)
    y = y_dev[:300]
    count = _word(5)
    first = PF.graphnorm_stats(y, ms, n_rows=count)
    count.fill_(129)
    second = PF.graphnorm_stats(y, ms, n_rows=count)
    assert np.array_equal(_bits(first), _bits(PF.graphnorm_stats(y_dev[:5], ms)))
    assert np.array_equal(_bits(second), _bits(PF.graphnorm_stats(y_dev[:129], ms)))
    count.fill_(100000)
    assert np.array_equal(_bits(PF.graphnorm_stats(y, ms, n_rows=count)), _bits(PF.graphnorm_stats(y, ms)))
    count.fill_(-3)
    assert not _bits(PF.graphnorm_stats(y, ms, n_rows=count)).any()
    with pytest.raises(ValueError):
        PF.graphnorm_stats(y, ms, n_rows=torch.zeros(1, dtype=torch.int64, device='cuda'))
    with pytest.raises(RuntimeError, match='host-count route needs at least one row'):
        PF.graphnorm_stats(y[:0], ms)


# ---- C. the layer ----------------------------------------------------------------------------------------------------
N_REAL = 207
LAYER_FLAGS = {False: dict(graphnorm=True), True: dict(graphnorm=True, node_attention=True)}


@functools.lru_cache(maxsize=None)
def _graph207():
    b = _two_graphs()
    assert int(b.x.size(0)) == N_REAL
    return SimpleNamespace(pos=b.pos.float(), edge_index=b.edge_index, edge_attr=b.edge_attr.long(), n_nodes=N_REAL)


def _padded_graph(n_cap):
    """The 207 nodes, then rows without edges."""
    g = _graph207()
    pos = torch.cat([g.pos, torch.randn(n_cap - N_REAL, 3, generator=torch.Generator().manual_seed(n_cap))])
    return SimpleNamespace(pos=pos, edge_index=g.edge_index, edge_attr=g.edge_attr, n_nodes=n_cap)


@contextlib.contextmanager
def _oracle_graphnorm_over(n):
    """The oracle's GraphNorm replaced by the restatement over the first n rows (None: the oracle's own)."""
    from oracle import egnn_oracle as orc
    if n is None:
        yield
        return
    own = orc.graph_norm
    orc.graph_norm = lambda x, weight, bias, mean_scale, eps=1e-5: gref.forward(x, weight, bias, mean_scale, n, eps)
    try:
        yield
    finally:
        orc.graph_norm = own


class _GnProblem(Problem):
    """tests/test_gpu_edge_classes.Problem (inputs, fp64 / fp32 oracle references, gradient floor) on `graph` with a
    flag set of this module; norm_rows: the oracle normalises every row by the statistics of that many leading ones."""

    def __init__(self, hid, flags, graph, norm_rows=None):
        self.A, self.hid, self.flags, self.depth, self.g, self.norm_rows = 3, hid, flags, 1, graph, norm_rows
        n, e = graph.n_nodes, int(graph.edge_index.shape[1])
        self.sds = [{k: v.detach().clone() for k, v in _new_layer(3, hid, flags, 11).state_dict().items()}]
        gen = torch.Generator().manual_seed(5 + hid)
        self.h0, self.m0, self.wh, self.wx, self.wm = (
            torch.randn(s, generator=gen) for s in ((n, hid), (e, hid), (n, hid), (n, 3), (e, hid)))
        self.ref64 = self.oracle(torch.float64)
        self.ref32 = [self.oracle(torch.float32)] + [self.oracle(torch.float32, perm)
                                                     for perm in edge_permutations(e, count=2)]
        self.floor = grad_floor({k: v for k, v in self.ref64.items() if k.startswith('grad ')})

    def oracle(self, dtype, perm=None):
        with _oracle_graphnorm_over(self.norm_rows):
            return super().oracle(dtype, perm)


@functools.lru_cache(maxsize=None)
def _unpadded(hid, natt):
    return _GnProblem(hid, LAYER_FLAGS[natt], _graph207())


def _run_padded(p, n_cap, count, dtype=torch.float32):
    """p's layer on p's graph followed by n_cap - n_nodes padding rows (random features and coordinates, no edges, zero
    upstream gradient), the statistics over `count` rows read from a device word. Everything of p.ref64's keys, the
    node tensors cut to p's rows; 'pad g_h' / 'pad h_out': the padding rows'."""
    from pointvs_amd import functional as PF
    from pointvs_amd.graph import prepare_graph
    n = p.g.n_nodes
    layer = _new_layer(3, p.hid, p.flags, 11)
    layer.load_state_dict(p.sds[0])
    layer = layer.to(dtype).cuda()
    gen = torch.Generator().manual_seed(n_cap)
    pad = lambda t: torch.cat([t, torch.randn(n_cap - n, t.shape[1], generator=gen)]).to(dtype).cuda()
    h0, x0 = pad(p.h0).requires_grad_(True), pad(p.g.pos).requires_grad_(True)
    pg = prepare_graph(p.g.edge_index.cuda(), p.g.edge_attr.cuda(), n_cap, need_backward=True)
    word = _word(count)
    pg.set_norm_rows(word)
    assert pg.t['norm_rows'] is word and pg.c.n_norm_rows_dev == word.data_ptr()
    h, x, m_sorted = layer.forward_prepared(pg, h0, x0, None, need_m=True)
    m = PF.rows_to_input_order(m_sorted, pg)
    ((h[:n] * p.wh.to(dtype).cuda()).sum() + (x[:n] * p.wx.to(dtype).cuda()).sum() + (m * p.wm.to(dtype).cuda()).sum()).backward()
    res = dict(h_out=h[:n], x_out=x[:n], m=m, g_h=h0.grad[:n], g_x=x0.grad[:n])
    if p.flags.get('node_attention'):
        res['natt'] = torch.as_tensor(layer.node_att_val)[:n]
    for name, param in layer.named_parameters():
        assert param.grad is not None, name
        res[p.param_key(0, name)] = param.grad
    torch.cuda.synchronize()
    res = {k: v.detach().cpu().numpy() for k, v in res.items()}
    return res, h.detach()[n:].cpu(), h0.grad[n:].cpu()


@pytest.mark.parametrize('n_cap', [207, 208, 256, 640])
@pytest.mark.parametrize('natt', [False, True], ids=['gn', 'gn-natt'])
@pytest.mark.parametrize('hid', [32, 64])
def test_padded_layer_matches_the_fp64_oracle_on_the_unpadded_graph(hid, natt, n_cap):
    p = _unpadded(hid, natt)
    got, pad_h, pad_g_h = _run_padded(p, n_cap, N_REAL)
    for name in ('node_mlp.1.weight', 'node_mlp.1.bias', 'node_mlp.1.mean_scale', 'node_mlp.0.bias'):
        assert f'grad {name}' in got and got[f'grad {name}'].any(), name
    p.check(got, f'graphnorm-rows-H{hid}-{"natt" if natt else "plain"}-cap{n_cap}')
    # the padding rows are normalised too (finite), and with no gradient arriving on them none leaves them
    assert torch.isfinite(pad_h).all() and not pad_g_h.any()


def test_a_gradient_on_the_padding_rows_follows_the_row_bound():
    """N_cap = 256, statistics over 207 rows, the loss reads all 256: the oracle with the restatement as its GraphNorm
    (autograd: the exact gradient of 'all rows normalised by the statistics of the first 207')."""
    p = _GnProblem(32, LAYER_FLAGS[True], _padded_graph(256), norm_rows=N_REAL)
    got, _, _ = _run_padded(p, 256, N_REAL)
    p.check(got, 'graphnorm-rows-H32-natt-cap256-padding-gradient')
    # and it is not the gradient of statistics over all 256 rows
    everywhere = _GnProblem(32, LAYER_FLAGS[True], _padded_graph(256), norm_rows=256)
    assert np.abs(everywhere.ref64['g_h'] - p.ref64['g_h']).max() > 1e-3 * np.abs(p.ref64['g_h']).max()


def test_a_count_of_zero_gives_finite_outputs_and_gradients():
    p = _unpadded(32, False)
    got, pad_h, _ = _run_padded(p, 256, 0)
    for key, value in got.items():
        assert np.all(np.isfinite(value)), key
    assert torch.isfinite(pad_h).all()
    assert not got['grad node_mlp.1.mean_scale'].any()        # the mean is the constant 0


def test_fp64_and_the_decomposed_route_refuse_the_count():
    from pointvs_amd.graph import prepare_graph
    g = _graph207()
    pg = prepare_graph(g.edge_index.cuda(), g.edge_attr.cuda(), 256, need_backward=False)
    pg.set_norm_rows(_word(N_REAL))
    x = torch.randn(256, 3, device='cuda')
    with torch.no_grad():
        layer64 = _new_layer(3, 32, LAYER_FLAGS[False], 11).double().cuda()
        with pytest.raises(RuntimeError, match='n_norm_rows_dev'):
            layer64.forward_prepared(pg, torch.randn(256, 32, device='cuda', dtype=torch.float64), x.double())
        wide = _new_layer(3, 160, LAYER_FLAGS[False], 11).cuda()
        with pytest.raises(NotImplementedError, match='hidden sizes up to 128'):
            wide.forward_prepared(pg, torch.randn(256, 160, device='cuda'), x)
        # cleared, both run
        pg.set_norm_rows(None)
        assert 'norm_rows' not in pg.t and not pg.c.n_norm_rows_dev
        assert torch.isfinite(wide.forward_prepared(pg, torch.randn(256, 160, device='cuda'), x)[0]).all()
        assert torch.isfinite(layer64.forward_prepared(pg, torch.randn(256, 32, device='cuda', dtype=torch.float64),
                                                       x.double())[0]).all()
    with pytest.raises(ValueError):
        pg.set_norm_rows(torch.zeros(2, dtype=torch.int32, device='cuda'))
