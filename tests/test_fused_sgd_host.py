"""CPU-side checks of the fused SGD (pointvs_amd/optim.py FusedClipSGD) and of the exports it and the device
hyper-parameter blocks need: without a GPU the optimiser IS clip_grad_value_ + torch.optim.SGD, its state and
`state_dict` are torch's, and the harness builds it for `optimiser='sgd'`."""
import copy
import re
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
SGD_KW = dict(lr=2e-3, momentum=0.9, nesterov=True, weight_decay=1e-4)
NEW_EXPORTS = ('pvs_hyper_write', 'pvs_adam_clip_step_hyper', 'pvs_sgd_clip_step', 'pvs_sgd_clip_step_hyper')


def _grads(params_a, params_b, step):
    for k, (pa, pb) in enumerate(zip(params_a, params_b)):
        g = torch.randn(pa.shape, generator=torch.Generator().manual_seed(10 * step + k)) * 3
        pa.grad, pb.grad = g.clone(), g.clone()


def test_fused_clip_sgd_falls_back_to_torch_on_cpu_tensors():
    """No GPU here: FusedClipSGD must behave exactly like clip_grad_value_ + torch.optim.SGD (five steps), survive
    copy.deepcopy, and exchange its state_dict with torch.optim.SGD in both directions."""
    from pointvs_amd.optim import FusedClipSGD
    torch.manual_seed(0)
    a = [torch.nn.Parameter(torch.randn(7, 3)), torch.nn.Parameter(torch.randn(5))]
    b = [torch.nn.Parameter(p.detach().clone()) for p in a]
    oa, ob = FusedClipSGD(a, **SGD_KW), torch.optim.SGD(b, **SGD_KW)
    assert isinstance(oa, torch.optim.SGD)
    for step in range(5):
        _grads(a, b, step)
        oa.step(clip_value=1.0)
        torch.nn.utils.clip_grad_value_(b, 1.0)
        ob.step()
    for pa, pb in zip(a, b):
        assert torch.equal(pa, pb) and torch.equal(pa.grad, pb.grad)
    sa, sb = oa.state_dict(), ob.state_dict()
    assert set(sa['state']) == set(sb['state']) and set(sa['state'][0]) == set(sb['state'][0]) == {'momentum_buffer'}
    assert [set(g) for g in sa['param_groups']] == [set(g) for g in sb['param_groups']]
    for k in sa['state']:
        assert torch.equal(sa['state'][k]['momentum_buffer'], sb['state'][k]['momentum_buffer'])

    # a copy (EMA / snapshot of a whole model) keeps the state and the switch, and starts with its own transients
    oa.capturable = True
    twin = copy.deepcopy(oa)
    assert isinstance(twin, FusedClipSGD) and twin.capturable
    assert twin._ring == [] and twin._fast is None and twin._recent == {} and twin._hyper == {}
    oa.capturable = twin.capturable = False
    assert torch.equal(twin.state_dict()['state'][1]['momentum_buffer'], sa['state'][1]['momentum_buffer'])

    # round trip: torch's SGD continues from the fused optimiser's state_dict, and the other way round
    c = [torch.nn.Parameter(p.detach().clone()) for p in a]
    d = [torch.nn.Parameter(p.detach().clone()) for p in a]
    oc, od = torch.optim.SGD(c, **SGD_KW), FusedClipSGD(d, **SGD_KW)
    oc.load_state_dict(copy.deepcopy(oa.state_dict()))        # (load_state_dict keeps tensors that need no cast: no aliases)
    od.load_state_dict(copy.deepcopy(ob.state_dict()))
    for step in range(5, 7):
        _grads(a, b, step)
        _grads(c, d, step)
        oa.step(clip_value=1.0)
        od.step(clip_value=1.0)
        for params, opt in ((b, ob), (c, oc)):
            torch.nn.utils.clip_grad_value_(params, 1.0)
            opt.step()
    for pa, pb, pc, pd in zip(a, b, c, d):
        assert torch.equal(pa, pb) and torch.equal(pa, pc) and torch.equal(pa, pd)


def test_fused_clip_sgd_without_momentum_keeps_no_state_on_cpu():
    from pointvs_amd.optim import FusedClipSGD
    torch.manual_seed(1)
    a = [torch.nn.Parameter(torch.randn(4, 2))]
    b = [torch.nn.Parameter(a[0].detach().clone())]
    oa, ob = FusedClipSGD(a, lr=1e-2, weight_decay=1e-3), torch.optim.SGD(b, lr=1e-2, weight_decay=1e-3)
    for step in range(3):
        _grads(a, b, step)
        oa.step(clip_value=1.0)
        torch.nn.utils.clip_grad_value_(b, 1.0)
        ob.step()
    assert torch.equal(a[0], b[0])
    assert oa.state_dict()['state'] == ob.state_dict()['state'] == {}


def test_the_harness_builds_the_fused_sgd_for_optimiser_sgd(tmp_path):
    """`optimiser='sgd'`: the reference's arguments (momentum 0.9, Nesterov, the weight decay) on a FusedClipSGD, which
    is a torch.optim.SGD; backprop() steps it with the clip at 1.0."""
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.optim import FusedClipAdam, FusedClipSGD
    kw = dict(dim_input=12, k=8, dim_output=1, num_layers=1, model_task='classification')
    model = SartorrasEGNN(tmp_path, 2e-3, 1e-4, None, None, silent=True, optimiser='sgd', **kw)
    assert isinstance(model.optimiser, FusedClipSGD) and isinstance(model.optimiser, torch.optim.SGD)
    group = model.optimiser.param_groups[0]
    assert (group['lr'], group['momentum'], group['nesterov'], group['weight_decay'], group['dampening']) == \
        (2e-3, 0.9, True, 1e-4, 0)
    assert not model.optimiser.capturable
    assert isinstance(SartorrasEGNN(tmp_path, 2e-3, 1e-4, None, None, silent=True, **kw).optimiser, FusedClipAdam)


def test_new_exports_are_declared_bound_and_versioned():
    from pointvs_amd import _lib
    header = (ROOT / 'include' / 'pvs_egnn.h').read_text()
    declared = set(re.findall(r'\b(pvs_[a-z0-9_]+)\s*\(', header))
    for name in NEW_EXPORTS:
        assert name in declared, name
        assert name in _lib.EXPORTED_SYMBOLS and name in _lib._PROTOTYPES, name
    assert 'PvsSgdEntry' in header
    assert _lib.MIN_VERSION >= 104
    handle = _lib.lib()
    assert handle.pvs_version() >= 104
    for name in NEW_EXPORTS:
        assert hasattr(handle, name), name
