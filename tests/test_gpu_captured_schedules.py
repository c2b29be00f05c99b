"""train_model(capture=True) under the learning-rate schedules and with SGD: the trajectories of the reference's own
`train_model` (tests/golden/train_*.npz; the SGD ones are made by tests/golden/make_golden_training_sgd.py) followed by
REPLAYED training steps. A captured step reads lr, betas / momentum from device memory, rewritten from the host's
values before every replay (pointvs_amd/optim.py `push_hyperparameters`), and `scheduler.step()` stays on the host: the
rate every step ran at must be the reference's to the last bit of a float64, whatever ran the step.

Bounds: losses within 1e-4 relative of the reference's, the project's trajectory bound
(tests/test_gpu_training_trajectory.py). For the SGD files the reference's own spread under permuted edge orders was
measured when they were made (1.8e-7, make_golden_training_sgd.py's docstring): far inside, so the bound is unchanged."""
import json

import numpy as np
import pytest
import torch

from tests._golden import needs_caching_allocator
from tests.test_gpu_training_trajectory import _load, _loaders

pytestmark = pytest.mark.gpu


class _RecordingLoader(list):
    """A list of resident batches (the same objects every epoch) that notes the optimiser's hyper-parameters each time
    it hands one out: what the step that follows runs at (the scheduler stepped after the previous one)."""

    def __init__(self, batches, model, log):
        super().__init__(batches)
        self.model, self.log = model, log

    def __iter__(self):
        for b in list.__iter__(self):
            group = self.model.optimiser.param_groups[0]
            self.log.append((float(group['lr']), float(group['momentum'] if 'momentum' in group else group['betas'][0])))
            yield b


def _model(meta, tmp_path):
    from pointvs_amd.egnn_multitask import MultitaskSatorrasEGNN
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    cls = SartorrasEGNN if meta['class'] == 'SartorrasEGNN' else MultitaskSatorrasEGNN
    torch.manual_seed(meta['seed'])
    np.random.seed(meta['seed'])
    tmp_path.mkdir(parents=True, exist_ok=True)
    return cls(tmp_path, meta['lr'], meta['wd'], None, None, silent=True, **meta['ctor'], **meta['kwargs'])


def _train(z, meta, tmp_path, capture):
    """One run over the file's phases on resident batches: (model, losses, [(lr, momentum | beta1)], capture stats)."""
    model = _model(meta, tmp_path)
    losses, log, stats = [], [], []
    for (task, n_batches, epochs), loader in zip(meta['phases'], _loaders(z, meta)):
        model.set_task(task)
        loader = _RecordingLoader([b.to('cuda') for b in loader], model, log)
        losses += [float(v) for v in model.train_model(loader, epochs=epochs, capture=capture)]
        if capture:
            stats.append((dict(model.last_capture_stats), n_batches, epochs))
    return model, losses, log, stats


def _check_against_the_file(z, meta, model, losses, log, tmp_path):
    ref_loss = z['loss']
    assert len(losses) == len(ref_loss) == len(log)
    lrs = np.asarray([v[0] for v in log], dtype=np.float64)
    assert np.array_equal(lrs, z['lr']), (lrs.tolist(), z['lr'].tolist())
    rel = np.abs(np.asarray(losses) - ref_loss) / np.abs(ref_loss)
    print(f"{meta['name']}: worst loss rel {rel.max():.2e}")
    assert rel.max() < 1e-4, (rel.tolist(), losses, ref_loss.tolist())
    assert (model.p_epoch, model.a_epoch, model.global_iter) == (meta['p_epoch'], meta['a_epoch'], meta['global_iter'])
    ckpts = sorted(str(p.relative_to(tmp_path)) for p in tmp_path.rglob('*.pt'))
    assert ckpts == meta['checkpoints']
    return ckpts


def _check_capture_counts(stats):
    for st, n_batches, epochs in stats:
        assert st['eager'] == n_batches and st['captured'] == (n_batches if epochs > 1 else 0), st
        assert st['replayed'] == n_batches * max(epochs - 2, 0), st


@needs_caching_allocator
@pytest.mark.parametrize('name', ['one_cycle', 'warm_restarts', 'k64_attention'])
def test_captured_training_steps_follow_the_reference_trajectory_under_a_scheduler(name, tmp_path):
    """The body of tests/test_gpu_training_trajectory.py's captured test on the SCHEDULED trajectories (OneCycleLR, which
    also cycles Adam's beta1, and CosineAnnealingWarmRestarts at 32 and 64 channels): every batch eager in its first
    epoch, captured in its second, replayed in its third; the per-step learning rate - sampled just before each
    replayer.step - array-equal to the reference's; losses within 1e-4 of the reference's; counters, checkpoints and
    optimiser step counts the reference's; the optimiser back in its non-capturable form afterwards.
    Against the SAME model's eager run the captured losses are held to the same 1e-4 (and the learning-rate and beta1
    sequences to equality): whether a replay is bit-identical to the eager step has not been established on hardware -
    the existing captured test does not assert it either - so the difference is printed, not held to zero."""
    from pointvs_amd.optim import FusedClipAdam
    z, meta = _load(name)
    model, losses, log, stats = _train(z, meta, tmp_path / 'captured', capture=True)
    _check_capture_counts(stats)
    ckpts = _check_against_the_file(z, meta, model, losses, log, tmp_path / 'captured')
    if name == 'one_cycle':
        assert all(u[1] != v[1] for u, v in zip(log, log[1:]))          # beta1 moved every step, through the replays too
    ck = torch.load(tmp_path / 'captured' / ckpts[-1], map_location='cpu', weights_only=False)
    opt_steps = sorted({int(s['step']) for s in ck['optimiser_state_dict']['state'].values()})
    assert opt_steps == meta['optimiser_steps_in_last_checkpoint']
    for rel_path in ckpts:      # written while the replayer had the optimiser capturable: held as the reference's
        osd = torch.load(tmp_path / 'captured' / rel_path, weights_only=False)['optimiser_state_dict']
        assert not any(g.get('capturable') for g in osd['param_groups']), rel_path
        assert all(not st['step'].is_cuda for st in osd['state'].values()), rel_path
    for k, v in model.state_dict().items():
        ref = z[f'sd1/{k}']
        if np.issubdtype(ref.dtype, np.floating):
            assert np.abs(v.detach().cpu().numpy().astype(np.float64) - ref).max() <= len(losses) * 2e-3 * 1.001, k
    assert isinstance(model.optimiser, FusedClipAdam)
    assert not any(g.get('capturable') for g in model.optimiser.param_groups)
    assert all(not s['step'].is_cuda for s in model.optimiser.state.values())

    _, eager_losses, eager_log, _ = _train(z, meta, tmp_path / 'eager', capture=False)
    assert eager_log == log
    diff = np.abs(np.asarray(losses) - np.asarray(eager_losses))
    print(f'{name}: captured vs eager losses, max |difference| {diff.max():.3e}')
    assert (diff / np.abs(np.asarray(eager_losses))).max() < 1e-4, (losses, eager_losses)


@needs_caching_allocator
@pytest.mark.parametrize('name', ['sgd', 'sgd_one_cycle'])
def test_sgd_training_follows_the_reference_trajectory_eagerly_and_captured(name, tmp_path):
    """`optimiser='sgd'` (FusedClipSGD: clip + momentum + Nesterov step in one launch) on the reference's SGD
    trajectories, constant rate and OneCycleLR (which cycles the momentum), eagerly and with captured steps: learning
    rates and momenta array-equal to the reference's, losses within 1e-4, counters and checkpoint files the
    reference's, and every checkpoint's optimiser state loads into a plain torch.optim.SGD - one momentum buffer per
    parameter that had a gradient, on whichever path wrote it. The two runs agree with each other within the same
    1e-4 (see the scheduler test above)."""
    from pointvs_amd.optim import FusedClipSGD
    z, meta = _load(name)
    runs = {}
    for capture in (False, True):
        where = tmp_path / ('captured' if capture else 'eager')
        model, losses, log, stats = _train(z, meta, where, capture=capture)
        _check_capture_counts(stats)
        ckpts = _check_against_the_file(z, meta, model, losses, log, where)
        assert np.array_equal(np.asarray([v[1] for v in log]), z['momentum'])
        assert isinstance(model.optimiser, FusedClipSGD) and not model.optimiser.capturable
        if not capture:     # (the replayer's close() drops the work list)
            assert model.optimiser._fast is not None and model.optimiser._fast['fusable']      # the kernel, not the fallback
        for rel_path in ckpts:
            ck = torch.load(where / rel_path, map_location='cpu', weights_only=False)
            assert sorted(ck.keys()) == meta['checkpoint_keys']
            osd = ck['optimiser_state_dict']
            assert 'capturable' not in osd['param_groups'][0]
            assert all(sorted(st) == meta['optimiser_state_keys'] for st in osd['state'].values())
            assert len(osd['state']) == meta['n_momentum_buffers']
            plain = torch.optim.SGD([torch.nn.Parameter(p.detach().cpu().clone()) for p in model.parameters()],
                                    lr=meta['lr'], momentum=0.9, nesterov=True, weight_decay=meta['wd'])
            plain.load_state_dict(osd)
            assert len(plain.state) == meta['n_momentum_buffers']
        runs[capture] = (model, losses)
    diff = np.abs(np.asarray(runs[True][1]) - np.asarray(runs[False][1]))
    print(f'{name}: captured vs eager losses, max |difference| {diff.max():.3e}')
    assert (diff / np.abs(np.asarray(runs[False][1]))).max() < 1e-4
    assert json.loads(str(z['meta']))['ctor']['optimiser'] == 'sgd'
