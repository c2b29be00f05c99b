"""The fused optimisers at operator level (pointvs_amd/optim.py over pvs_sgd_clip_step, pvs_*_clip_step_hyper and
pvs_hyper_write): FusedClipSGD against clip_grad_value_ + torch.optim.SGD, and the capturable forms - lr, betas /
momentum read from device memory - against their host-scalar twins, bit for bit, through a hipGraph replay whose
hyper-parameters change every step as a OneCycleLR changes them.

Shapes: those of tests/test_gpu_properties.py's Adam test plus a single element, 257 (one block and one thread) and 5000
(more than the 8 x 256 threads a tensor gets: the grid-stride loop and its tail)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from tests._golden import needs_caching_allocator, rel_err

pytestmark = pytest.mark.gpu
SHAPES = [(32, 68), (32,), (1, 32), (64, 64), (3,), (1,), (257,), (5000,)]
NEVER, LATE = 4, 2          # indices into SHAPES: a parameter that never has a gradient, one whose first comes at step 3


def _np(t):
    return t.detach().cpu().numpy()


def _grad(shape, step, k):
    return torch.randn(shape, generator=torch.Generator().manual_seed(10 * step + k)).cuda() * 2


@pytest.mark.parametrize('momentum,nesterov', [(0.9, True), (0.0, False), (0.9, False)])
def test_fused_clip_sgd_matches_torch_sgd(momentum, nesterov):
    """pvs_sgd_clip_step (one launch, two while some parameters have no momentum buffer yet) vs clip_grad_value_ +
    torch.optim.SGD over five steps, with a parameter that never receives a gradient and one that starts at step 3.
    1e-6 relative (torch's foreach ops may or may not contract to FMAs; the kernel never does); the clipped gradients
    and the state_dict layout are torch's exactly, and torch's SGD continues from the fused optimiser's state."""
    from pointvs_amd.optim import FusedClipSGD
    kw = dict(lr=2e-3, momentum=momentum, nesterov=nesterov, weight_decay=1e-4)
    torch.manual_seed(0)
    a = [torch.nn.Parameter(torch.randn(s, device='cuda')) for s in SHAPES]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    oa, ob = FusedClipSGD(a, **kw), torch.optim.SGD(b, **kw)

    def set_grads(param_lists, step):
        for k in range(len(SHAPES)):
            g = None if k == NEVER or (k == LATE and step < 2) else _grad(SHAPES[k], step, k)
            for ps in param_lists:
                ps[k].grad = None if g is None else g.clone()

    for step in range(5):
        set_grads((a, b), step)
        oa.step(clip_value=1.0)
        torch.nn.utils.clip_grad_value_(b, 1.0)
        ob.step()
    assert oa._fast is not None and oa._fast['fusable']          # the kernel ran, not the fallback
    for k, (pa, pb) in enumerate(zip(a, b)):
        assert rel_err(_np(pa), _np(pb)) < 1e-6, k
        assert (pa.grad is None) == (pb.grad is None)
        if pa.grad is not None:
            assert torch.equal(pa.grad, pb.grad), k          # clipped in place, like clip_grad_value_
    assert torch.equal(a[NEVER].detach(), b[NEVER].detach())
    sda, sdb = oa.state_dict(), ob.state_dict()
    assert set(sda['state']) == set(sdb['state'])
    assert [set(g) for g in sda['param_groups']] == [set(g) for g in sdb['param_groups']]
    for k in sda['state']:
        assert set(sda['state'][k]) == set(sdb['state'][k])
        if momentum:
            assert rel_err(_np(sda['state'][k]['momentum_buffer']), _np(sdb['state'][k]['momentum_buffer'])) < 1e-6, k
    assert (len(sda['state']) == len(SHAPES) - 1) if momentum else (sda['state'] == {})

    # torch's SGD takes the fused optimiser's checkpoint and goes on exactly as a torch SGD does that holds the same
    # buffers as its own state (and, to 1e-6, as the torch SGD that ran beside it all along)
    c = [torch.nn.Parameter(p.detach().clone()) for p in a]
    d = [torch.nn.Parameter(p.detach().clone()) for p in a]
    oc, od = torch.optim.SGD(c, **kw), torch.optim.SGD(d, **kw)
    oc.load_state_dict(copy.deepcopy(sda))
    if momentum:
        for k, p in enumerate(d):
            if k in sda['state']:
                od.state[p]['momentum_buffer'] = sda['state'][k]['momentum_buffer'].clone()
    for step in range(5, 7):
        set_grads((b, c, d), step)
        for params, opt in ((b, ob), (c, oc), (d, od)):
            torch.nn.utils.clip_grad_value_(params, 1.0)
            opt.step()
    for k, (pb, pc, pd) in enumerate(zip(b, c, d)):
        assert torch.equal(pc.detach(), pd.detach()), k
        assert rel_err(_np(pc), _np(pb)) < 1e-6, k


def _one_cycle_values(make_optimiser, steps=6):
    """(lr, momentum or beta1) of each step of a `steps`-step OneCycleLR at the harness's max_lr."""
    p = torch.nn.Parameter(torch.zeros(1))
    opt = make_optimiser([p])
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr=2e-3, total_steps=steps)
    out = []
    for t in range(steps):
        group = opt.param_groups[0]
        out.append((float(group['lr']), float(group['momentum'] if 'momentum' in group else group['betas'][0])))
        opt.step()
        if t + 1 < steps:
            sched.step()
    assert all(u[0] != v[0] and u[1] != v[1] for u, v in zip(out, out[1:]))       # both change every step
    return out


def _set(opt, lr, m):
    for group in opt.param_groups:
        group['lr'] = lr
        if 'momentum' in group:
            group['momentum'] = m
        else:
            group['betas'] = (m, group['betas'][1])


@needs_caching_allocator
@pytest.mark.parametrize('kind', ['sgd', 'adam'])
def test_device_hyperparameters_match_the_host_scalar_form_bit_for_bit_eagerly_and_replayed(kind):
    """FusedClipSGD / FusedClipAdam with capturable=True read lr and momentum / the betas from device memory
    (pvs_*_clip_step_hyper). Six steps at the (lr, momentum | beta1) pairs of a six-step OneCycleLR - both change every
    step: three eager, the fourth captured on a side stream, the last two replayed after push_hyperparameters() - must
    leave the parameters and every state tensor of the non-capturable twin that was given the same values as host
    scalars, bit for bit, and torch's own optimiser's to 1e-6. A replay that ran at the rate or momentum of the capture
    would differ from both."""
    from pointvs_amd.optim import FusedClipAdam, FusedClipSGD
    if kind == 'sgd':
        kw = dict(lr=2e-3, momentum=0.9, nesterov=True, weight_decay=1e-4)
        fused, ref_cls, ref_kw, state_names = FusedClipSGD, torch.optim.SGD, kw, ('momentum_buffer',)
    else:
        kw = dict(lr=2e-3, weight_decay=1e-4)
        fused, ref_cls, ref_kw, state_names = FusedClipAdam, torch.optim.Adam, dict(kw, capturable=True), \
            ('exp_avg', 'exp_avg_sq')
    values = _one_cycle_values(lambda ps: ref_cls(ps, **kw))
    assert all(values[3][j] != values[t][j] for t in (4, 5) for j in (0, 1))      # the replays differ from the capture
    shapes = [s for k, s in enumerate(SHAPES) if k != NEVER]
    torch.manual_seed(0)
    a = [torch.nn.Parameter(torch.randn(s, device='cuda')) for s in shapes]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    c = [torch.nn.Parameter(p.detach().clone()) for p in a]
    oa, ob, oc = fused(a, capturable=True, **kw), fused(b, **kw), ref_cls(c, **ref_kw)
    grads = [[_grad(s, t, k) for k, s in enumerate(shapes)] for t in range(6)]
    for p in a + b + c:
        p.grad = torch.zeros_like(p)
    stream = torch.cuda.Stream()
    hip_graph = None
    with torch.cuda.stream(stream):
        for t in range(6):
            for k in range(len(shapes)):
                for ps in (a, b, c):
                    ps[k].grad.copy_(grads[t][k])
            for opt in (oa, ob, oc):
                _set(opt, *values[t])
            if t < 3:
                oa.step(clip_value=1.0)
            elif hip_graph is None:
                oa.push_hyperparameters()        # (outside the capture: what the first replay runs at)
                stream.synchronize()
                hip_graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(hip_graph, stream=stream):
                    oa.step(clip_value=1.0)
                hip_graph.replay()               # (capturing does not execute)
            else:
                oa.push_hyperparameters()
                hip_graph.replay()
            ob.step(clip_value=1.0)
            torch.nn.utils.clip_grad_value_(c, 1.0)
            oc.step()
    torch.cuda.synchronize()
    assert oa._fast['fusable'] and ob._fast['fusable']
    assert all(w['hyper'] is not None for w in oa._fast['groups'][0]) and len(oa._fast['groups'][0]) == 1
    sa, sb, sc = oa.state_dict()['state'], ob.state_dict()['state'], oc.state_dict()['state']
    assert set(sa) == set(sb) == set(sc) == set(range(len(shapes)))
    for k, (pa, pb, pc) in enumerate(zip(a, b, c)):
        assert torch.equal(pa.detach(), pb.detach()), k
        assert torch.equal(pa.grad, pb.grad) and torch.equal(pa.grad, pc.grad), k
        assert rel_err(_np(pa), _np(pc)) < 1e-6, k
        assert set(sa[k]) == set(sb[k]) == set(sc[k])
        for name in state_names:
            assert torch.equal(sa[k][name], sb[k][name]), (k, name)
            assert rel_err(_np(sa[k][name]), _np(sc[k][name])) < 1e-6, (k, name)
        if kind == 'adam':
            assert float(sa[k]['step']) == float(sb[k]['step']) == float(sc[k]['step']) == 6.0


@pytest.mark.parametrize('n', [1, 2, 3, 4])
def test_hyper_write_stores_the_doubles_it_was_given(n):
    """pvs_hyper_write: n doubles by value into device memory, exactly, and nothing behind them."""
    from pointvs_amd import _lib
    values = [2e-3 * 0.7, 1.0 / 3.0, 0.999, 1e-300][:n]
    block = torch.full((6,), -1.0, dtype=torch.float64, device='cuda')
    args = values + [7.0] * (4 - n)                              # (arguments past n must not be stored)
    _lib.check(_lib.lib().pvs_hyper_write(block.data_ptr(), n, *args, _lib.stream(block.device)), 'pvs_hyper_write')
    got = block.cpu().numpy()
    assert np.array_equal(got[:n], np.asarray(values, dtype=np.float64)), (got, values)
    assert np.array_equal(got[n:], np.full(6 - n, -1.0))
    for bad in (0, 5):
        assert _lib.lib().pvs_hyper_write(block.data_ptr(), bad, 0.0, 0.0, 0.0, 0.0, _lib.stream(block.device)) != 0
    assert ctypes.sizeof(ctypes.c_double) == block.element_size()
