"""Captured training, host side: the optimiser's capturable window (optim.capturable_window) and the model's dropout key
schedule (egnn_satorras.DropoutKeys) on CPU models. The replayer itself needs a GPU: tests/test_gpu_captured_*.py."""
import copy
import hashlib
import types

import pytest
import torch

from pointvs_amd.egnn_satorras import DropoutKeys, SartorrasEGNN, _mix64
from pointvs_amd.optim import FusedClipAdam, FusedClipSGD, capturable_window

KW = dict(dim_input=12, k=16, dim_output=1, num_layers=2, dropout=0.25, graphnorm=False)


def _stepped_model(tmp_path, optimiser):
    torch.manual_seed(5)
    model = SartorrasEGNN(tmp_path, 2e-3, 1e-4, silent=True, optimiser=optimiser, **KW)
    for _ in range(2):
        for p in model.parameters():
            p.grad = torch.full_like(p, 0.5)
        model.optimiser.step(clip_value=1.0)
    return model


def _form(opt):
    """What the window flips: SGD's attribute, the groups' flags, where and as what the step counters are held."""
    return (getattr(opt, 'capturable', None), [g.get('capturable') for g in opt.param_groups],
            [(st['step'].device, st['step'].dtype, float(st['step'])) for st in opt.state.values() if 'step' in st])


def _assert_same_state_dict(got, want):
    assert got['param_groups'] == want['param_groups']
    assert got['state'].keys() == want['state'].keys() and len(want['state']) > 0
    for idx, st in want['state'].items():
        assert got['state'][idx].keys() == st.keys()
        for name, value in st.items():
            other = got['state'][idx][name]
            assert other.device.type == 'cpu' and other.dtype == value.dtype and torch.equal(other, value), (idx, name)


@pytest.mark.parametrize('optimiser', ['adam', 'sgd'])
@pytest.mark.parametrize('raises', [False, True])
def test_the_capturable_window_flips_and_restores(optimiser, raises, tmp_path, monkeypatch):
    model = _stepped_model(tmp_path, optimiser)
    opt = model.optimiser
    assert isinstance(opt, FusedClipAdam if optimiser == 'adam' else FusedClipSGD)
    reserved = []       # (pinned memory needs a GPU: the call is recorded here)
    monkeypatch.setattr(type(opt), 'reserve_capture_tables', lambda self, k: reserved.append(k))
    before, plain = _form(opt), copy.deepcopy(opt.state_dict())
    opt._fast = 'a work list'
    try:
        with capturable_window(opt, 7) as window:
            assert reserved == [7] and opt._fast is None
            flag, flags, counters = _form(opt)
            if optimiser == 'sgd':
                assert flag is True and flags == before[1] and counters == []
            else:
                assert flags == [True] * len(opt.param_groups) and len(counters) == len(list(model.parameters()))
                assert all((dev, dtype, n) == (p.device, torch.float32, 2.0)
                           for (dev, dtype, n), p in zip(counters, model.parameters()))
            _assert_same_state_dict(window.checkpoint_state_dict(), plain)
            opt._fast = 'the window\'s work list'
            if raises:
                raise KeyError('from the body')
    except KeyError:
        assert raises
    assert _form(opt) == before and opt._fast is None
    _assert_same_state_dict(opt.state_dict(), plain)


def test_the_window_on_plain_torch_adam_and_groups_that_were_capturable():
    params = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2))]
    opt = torch.optim.Adam([dict(params=params[:1]), dict(params=params[1:], capturable=False)], lr=1e-3)
    for p in params:
        p.grad = torch.ones_like(p)
    opt.step()
    before, plain = _form(opt), copy.deepcopy(opt.state_dict())
    with capturable_window(opt, 3) as window:
        assert [g['capturable'] for g in opt.param_groups] == [True, True]
        _assert_same_state_dict(window.checkpoint_state_dict(), plain)
    assert _form(opt) == before
    _assert_same_state_dict(opt.state_dict(), plain)


def _owner(**counters):
    return types.SimpleNamespace(**dict(dict(p_epoch=0, a_epoch=0, global_iter=0), **counters))


def test_dropout_keys_next_is_the_models_schedule(monkeypatch):
    """(seed, step) = (torch.initial_seed() + golden ratio * rank, _mix64(_mix64(base) + calls)), base = (epochs << 24) +
    global_iter, calls from 1 under one base: several calls under one base, a changed global_iter, a changed epoch,
    rank 1."""
    torch.manual_seed(77)
    keys, owner = DropoutKeys(), _owner()
    got = [keys.next(owner) for _ in range(3)]
    owner.global_iter = 5
    got += [keys.next(owner), keys.next(owner)]
    owner.p_epoch = 1
    got.append(keys.next(owner))
    owner.a_epoch = 2
    got.append(keys.next(owner))
    bases_calls = [(0, 1), (0, 2), (0, 3), (5, 1), (5, 2), ((1 << 24) + 5, 1), ((3 << 24) + 5, 1)]
    assert got == [(77, _mix64(_mix64(base) + calls)) for base, calls in bases_calls]
    assert (keys.base, keys.calls) == ((3 << 24) + 5, 1)
    monkeypatch.setattr(torch.distributed, 'is_initialized', lambda: True)
    monkeypatch.setattr(torch.distributed, 'get_rank', lambda *a, **k: 1)
    assert DropoutKeys().next(_owner(global_iter=5)) == ((77 + 0x9E3779B97F4A7C15) % 2 ** 64, _mix64(_mix64(5) + 1))


def test_the_model_forwards_to_its_one_key_object(tmp_path):
    torch.manual_seed(77)
    model = SartorrasEGNN(tmp_path, 2e-3, 1e-4, silent=True, **KW)
    keys = model.dropout_keys
    assert model.dropout_keys is keys and isinstance(keys, DropoutKeys)
    assert model.next_dropout_key() == (77, _mix64(_mix64(0) + 1)) and (keys.base, keys.calls) == (0, 1)
    assert model.next_dropout_key() == (77, _mix64(_mix64(0) + 2))


@pytest.mark.parametrize('prior', ['unset', False, True])
@pytest.mark.parametrize('raises', [False, True])
def test_external_keys_restore_static_dropout(prior, raises, tmp_path):
    model = SartorrasEGNN(tmp_path, 2e-3, 1e-4, silent=True, **KW)
    if prior != 'unset':
        model.static_dropout = prior
    keys = model.dropout_keys
    try:
        with keys.external(model):
            assert model.static_dropout is True and keys.is_external
            if raises:
                raise KeyError('from the body')
    except KeyError:
        assert raises
    assert not keys.is_external
    if prior == 'unset':
        assert 'static_dropout' not in model.__dict__ and model.static_dropout is None
    else:
        assert model.__dict__['static_dropout'] is prior


def test_an_external_key_serves_one_forward(tmp_path, monkeypatch):
    """take() on the host (the table write is a launch: recorded instead)."""
    from pointvs_amd import functional as PF
    written = []
    monkeypatch.setattr(PF, 'write_dropout_key', lambda table, seed, step: written.append((seed, step)))
    torch.manual_seed(77)
    model = SartorrasEGNN(tmp_path, 2e-3, 1e-4, silent=True, **KW)
    keys = model.dropout_keys
    first, table = keys.take(model, 'cpu')         # not external: every forward pushes its own key
    second, same = keys.take(model, 'cpu')
    assert same is table and table.dtype == torch.int64 and tuple(table.shape) == (2,)
    assert written == [first, second] == [(77, _mix64(_mix64(0) + 1)), (77, _mix64(_mix64(0) + 2))]
    with keys.external(model):
        with pytest.raises(RuntimeError, match='second training forward'):
            keys.take(model, 'cpu')                # nothing pushed for this step
        pushed = model.push_dropout_key('cpu')
        assert keys.take(model, 'cpu') == (pushed, table) and written[-1] == pushed == (77, _mix64(_mix64(0) + 3))
        with pytest.raises(RuntimeError, match='second training forward'):
            keys.take(model, 'cpu')
    assert len(written) == 3


def test_the_key_object_is_no_part_of_the_state_dict(tmp_path):
    model = SartorrasEGNN(tmp_path, 2e-3, 1e-4, silent=True, **KW)
    names = list(model.state_dict().keys())
    assert names and not any('dropout' in n for n in names)
    # the 26 names of this model as the package gave them before the key object existed, in order
    assert hashlib.sha256('\n'.join(names).encode()).hexdigest() == \
        '95001bb39af2a510b2ea4095e8dfecb03ac18a914182e7783c62f309917747ab'
    model.next_dropout_key()
    with model.dropout_keys.external(model):
        pass
    model.dropout_keys.table = torch.zeros(2, dtype=torch.int64)
    assert list(model.state_dict().keys()) == names
    assert [n for n, _ in model.named_buffers()] == [n for n, _ in copy.deepcopy(model).named_buffers()]
    twin = copy.deepcopy(model)
    assert list(twin.state_dict().keys()) == names
    assert twin.dropout_keys is not model.dropout_keys and twin.dropout_keys.table is not model.dropout_keys.table
    assert (twin.dropout_keys.base, twin.dropout_keys.calls) == (model.dropout_keys.base, model.dropout_keys.calls) == (0, 1)
    assert twin.next_dropout_key() == model.next_dropout_key()
