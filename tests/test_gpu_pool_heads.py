"""PF.pool_heads (pvs_pool_heads_fwd): one pooling and several heads in one launch. Exact against the single-head op
(PF.pool_head) and PF.mean_pool on the same inputs, exact on integer-valued inputs, Softplus against the fp64 value
within what torch's own fp32 softplus shows on the same logits, and the refusals."""
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
NODES = (0, 1, 127, 128, 129, 300)      # width 32: 32 rows a trip - the 4-way unrolled loop, its tail, the empty graph
PADDING = 40                            # rows behind graph_ptr[-1]: no graph's
HEAD_SETS = {'none+relu': [(1, None), (1, 'relu')], 'none+softplus3': [(1, None), (3, 'softplus')],
             'single': [(2, None)], 'no-bias': [(1, None, False), (3, 'relu', False), (2, None, True)]}


def _graphs(nodes):
    ptr = np.concatenate([[0], np.cumsum(nodes)]).astype(np.int32)
    return torch.from_numpy(ptr).cuda(), int(ptr[-1])


def _heads(spec, width, gen, integer=False):
    heads = []
    for n_out, act, *bias in spec:
        if integer:
            w = torch.randint(-3, 4, (n_out, width), generator=gen).float()
            b = torch.randint(-5, 6, (n_out,), generator=gen).float()
        else:
            w, b = torch.randn(n_out, width, generator=gen) / width ** 0.5, torch.randn(n_out, generator=gen)
        heads.append((w.cuda(), b.cuda() if (not bias or bias[0]) else None, act))
    return heads


def _columns(y, heads):
    at = 0
    for w, b, act in heads:
        yield y[:, at:at + w.shape[0]], w, b, act
        at += w.shape[0]
    assert at == y.shape[1]


def _ulps(got, want):
    """Distance in units of the last place between fp32 tensors of one sign pattern (softplus: positive)."""
    return (got.contiguous().view(torch.int32).long() - want.contiguous().view(torch.int32).long()).abs()


def _softplus64(x):
    return torch.log1p(torch.exp(x.double())).float()


def _softplus_distances(got, logits):
    """(the kernel's, torch's own fp32 softplus's) largest ulp distance from the fp64 value on `logits`."""
    want = _softplus64(logits)
    return int(_ulps(got, want).max()), int(_ulps(torch.nn.functional.softplus(logits), want).max())


@pytest.mark.parametrize('nodes', [NODES, (77,)], ids=['six-graphs', 'B=1'])
@pytest.mark.parametrize('width', [16, 32, 64, 128])
@pytest.mark.parametrize('spec', list(HEAD_SETS))
def test_columns_equal_the_single_head_op_bit_for_bit(spec, width, nodes):
    from pointvs_amd import functional as PF
    gen = torch.Generator().manual_seed(1000 + width + len(nodes))
    graph_ptr, n = _graphs(nodes)
    h = torch.randn(n + PADDING, width, generator=gen).cuda()
    heads = _heads(HEAD_SETS[spec], width, gen)
    with torch.no_grad():
        y, pooled = PF.pool_heads(h, graph_ptr, heads, return_pooled=True)
        assert torch.equal(PF.pool_heads(h, graph_ptr, heads), y)
        assert y.shape == (len(nodes), sum(w.shape[0] for w, _, _ in heads))
        assert torch.equal(pooled, PF.mean_pool(h, graph_ptr))
        for cols, w, b, act in _columns(y, heads):
            single = PF.pool_head(h, graph_ptr, w, b)
            if act is None:
                assert torch.equal(cols, single)
            elif act == 'relu':
                assert torch.equal(cols, torch.relu(single))
            else:       # (the bound of test_softplus_..., on this head's own logits)
                got, own = _softplus_distances(cols, single)
                assert got <= max(1, 2 * own), (got, own)
            if nodes[0] == 0:                      # the empty graph: act(b), exactly
                bias = torch.zeros(w.shape[0], device='cuda') if b is None else b
                want = {None: bias, 'relu': torch.relu(bias)}.get(act)
                if want is not None:
                    assert torch.equal(cols[0], want)
                else:
                    got, own = _softplus_distances(cols[0], bias)
                    assert got <= max(1, 2 * own), (got, own)


@pytest.mark.parametrize('width', [16, 32, 64, 128])
def test_integer_valued_inputs_give_exact_results(width):
    """Rows that are the graph's node count times small integers: the sums, the mean (an integer) and the products
    are all exact in fp32 (every intermediate below 2^24), so the result is THE value, whatever the order."""
    from pointvs_amd import functional as PF
    gen = torch.Generator().manual_seed(2000 + width)
    graph_ptr, n = _graphs(NODES)
    ints = torch.randint(-4, 5, (n + PADDING, width), generator=gen)
    count = torch.repeat_interleave(torch.tensor(NODES + (1,)), torch.tensor(NODES + (PADDING,)))
    h = (ints * count[:, None]).float().cuda()
    heads = _heads([(1, None), (3, 'relu'), (2, None, False)], width, gen, integer=True)
    with torch.no_grad():
        y, pooled = PF.pool_heads(h, graph_ptr, heads, return_pooled=True)
    ptr = graph_ptr.cpu().tolist()
    mean = torch.stack([ints[ptr[g]:ptr[g + 1]].sum(0) for g in range(len(NODES))])          # int64
    assert torch.equal(pooled.cpu(), mean.float())
    for cols, w, b, act in _columns(y.cpu(), heads):
        want = mean @ w.cpu().long().T + (0 if b is None else b.cpu().long())
        assert int(want.abs().max()) < 2 ** 24
        assert torch.equal(cols, (want.clamp_min(0) if act == 'relu' else want).float())


def test_softplus_is_within_twice_what_torch_softplus_shows_on_the_same_logits():
    """One node per graph with the logit in channel 0 and unit weights: the head's pre-activations are x, -x and x / 2
    exactly. Reference: log1p(exp(x)) in fp64, rounded to fp32. Allowed: twice the largest ulp distance torch's own
    fp32 softplus shows on the device on the same logits, at least 1 ulp (the kernel takes another, equally valid
    expf / log1pf route: the margin of one more rounding each). Above the threshold (20) the result is the input."""
    from pointvs_amd import functional as PF
    width = 16
    above = float(np.nextafter(np.float32(20.0), np.float32(30.0)))
    below = float(np.nextafter(np.float32(20.0), np.float32(0.0)))
    x = torch.cat([torch.linspace(-30.0, 30.0, 1537), torch.tensor([20.0, above, below, 20.5, 25.0, 30.0, 0.0, -20.0])])
    h = torch.zeros(x.numel(), width)
    h[:, 0] = x
    w = torch.zeros(3, width)
    w[:, 0] = torch.tensor([1.0, -1.0, 0.5])
    graph_ptr, _ = _graphs([1] * x.numel())
    with torch.no_grad():
        y = PF.pool_heads(h.cuda(), graph_ptr, [(w[:1].cuda(), None, None), (w.cuda(), None, 'softplus')])
        logits = (x[:, None] * w[:, 0]).cuda()
        assert torch.equal(y[:, :1], logits[:, :1]) and logits.min() == -30 and logits.max() == 30
        got, own = _softplus_distances(y[:, 1:], logits)
    text = (f'softplus on {logits.numel()} logits in [-30, 30] against log1p(exp(x)) in fp64 rounded to fp32, largest '
            f'distance in ulps\ntorch.nn.functional.softplus (fp32, device): {own}\npvs_pool_heads_fwd: {got}\n'
            f'allowed for the kernel: max(1, 2 x torch) = {max(1, 2 * own)}\n')
    print(text)
    (ROOT / 'profiles' / 'two_head_pool_heads_ulps.txt').write_text(text)
    assert got <= max(1, 2 * own), (got, own)
    over = logits > 20
    assert int(over.sum()) >= 6 and torch.equal(y[:, 1:][over], logits[over])


def test_refusals():
    from pointvs_amd import _lib
    from pointvs_amd import functional as PF
    width = 32
    graph_ptr, n = _graphs((3, 5))
    h = torch.randn(n, width).cuda()
    w, b = torch.randn(2, width).cuda(), torch.randn(2).cuda()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='heads'):
            PF.pool_heads(h, graph_ptr, [(w, b, None)] * 5)
        assert PF.pool_heads(h, graph_ptr, [(w, b, None)] * 4).shape == (2, 8)
        with pytest.raises(TypeError, match='fp32 only'):
            PF.pool_heads(h.double(), graph_ptr, [(w, b, None)])
        with pytest.raises(TypeError, match='fp32 only'):
            PF.pool_heads(h, graph_ptr, [(w.double(), b, None)])
        with pytest.raises(ValueError, match='activation'):
            PF.pool_heads(h, graph_ptr, [(w, b, 'silu')])
    for name in ('h', 'w', 'b'):
        grads = {k: v.clone().requires_grad_(k == name) for k, v in (('h', h), ('w', w), ('b', b))}
        with pytest.raises(RuntimeError, match='forward only'):
            PF.pool_heads(grads['h'], graph_ptr, [(grads['w'], grads['b'], None)])
        with torch.no_grad():
            PF.pool_heads(grads['h'], graph_ptr, [(grads['w'], grads['b'], None)])
    # the C entry itself: overlapping and out-of-range column ranges (the Python op lays the columns out itself)
    y = torch.full((2, 4), 7.0).cuda()

    def call(cols, ld_y=4):
        table = (_lib.PvsHead * len(cols))(*[_lib.PvsHead(_lib.ptr(w), _lib.ptr(b), 2, _lib.HEAD_NONE, c) for c in cols])
        return _lib.lib().pvs_pool_heads_fwd(_lib.ptr(h), _lib.ptr(graph_ptr), table, len(cols), None, _lib.ptr(y), 2,
                                             width, ld_y, _lib.stream(h.device))
    for cols, what in (((0, 1), 'overlapping'), ((1, 0), 'overlapping'), ((2, 2), 'overlapping'), ((0, 3), 'outside'),
                       ((-1, 2), 'outside')):
        assert call(cols) == -1, cols
        assert what in _lib.lib().pvs_last_error().decode(), cols
    torch.cuda.synchronize()
    assert bool((y == 7.0).all())                     # a refused call launches nothing
    assert call((2, 0)) == 0
    torch.cuda.synchronize()
    with torch.no_grad():
        assert torch.equal(y[:, :2], PF.pool_head(h, graph_ptr, w, b)) and torch.equal(y[:, 2:], y[:, :2])
