#!/usr/bin/env python3
"""Reference-generated training trajectories under SGD (`optimiser='sgd'`: torch.optim.SGD, momentum 0.9, Nesterov,
point_neural_network_base.py:86-92), beside the Adam ones of make_golden_training.py and made the same way: the
reference's own `train_model` on the same fixed list of batches (`batches(100)`), recorded per step.

    sgd               SartorrasEGNN (the `default` trajectory's model), SGD lr 2e-3 wd 1e-4, 3 epochs x 4 batches
    sgd_one_cycle     the same with use_1cycle=True (OneCycleLR over all 12 steps: cycles lr AND the momentum)

Build container only (needs /root/reference and the import-only stand-ins of make_golden.py). Output:
tests/golden/train_<name>.npz with the keys of the Adam files, minus Adam's step bookkeeping (`meta` has no
`optimiser_steps_in_last_checkpoint`: SGD's state is one `momentum_buffer` per parameter) plus `momentum`, the
momentum every step ran at.

    python tests/golden/make_golden_training_sgd.py            # writes the two files
    python tests/golden/make_golden_training_sgd.py --spread   # the reference against itself, edges permuted

How far the reference's SGD run is from ITSELF when only the order of the edge lists changes (fp32 summation order
in its scatter-adds; CPU, one thread, 2 seeded permutations per schedule, worst relative loss difference over the
twelve steps) - measured with --spread, torch 2.10, 2026-10:

    sgd             1.77e-07
    sgd_one_cycle   8.99e-08

Both are far inside the project's trajectory bound of 1e-4 relative (tests/test_gpu_training_trajectory.py), which
tests/test_gpu_captured_schedules.py therefore uses unchanged for these files.
"""
import json
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
import make_golden_training as mgt  # noqa: E402  (stubs, sys.path, cwd, one thread; batches / record_training / KW)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from point_vs.models.geometric.egnn_satorras import SartorrasEGNN  # noqa: E402

SCHEDULES = {'sgd': {'optimiser': 'sgd'}, 'sgd_one_cycle': {'optimiser': 'sgd', 'use_1cycle': True}}
SEED, EPOCHS = 7, 3


def train(ctor, loader, tmp):
    """One reference run: (model, initial state_dict, [(loss, lr, momentum)] per step)."""
    torch.manual_seed(SEED)
    np.random.seed(SEED)
    model = SartorrasEGNN(Path(tmp), 2e-3, 1e-4, None, None, silent=True, **ctor, **mgt.KW)
    sd0 = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    momenta = []
    real_backprop = model.backprop

    def backprop(y_true, y_pred):
        momenta.append(float(model.optimiser.param_groups[0]['momentum']))
        return real_backprop(y_true, y_pred)
    model.backprop = backprop                     # (record_training wraps this one in turn)
    steps = mgt.record_training(model, [('classification', loader, EPOCHS)])
    return model, sd0, [(loss, lr, m) for (_, loss, lr), m in zip(steps, momenta)]


def run(name, ctor):
    loader = mgt.batches(100)
    with tempfile.TemporaryDirectory() as tmp:
        model, sd0, steps = train(ctor, loader, tmp)
        ckpts = sorted(str(p.relative_to(tmp)) for p in Path(tmp).rglob('*.pt'))
        ck = torch.load(Path(tmp) / ckpts[-1], map_location='cpu', weights_only=False)
        state = ck['optimiser_state_dict']['state']
        assert state and all(set(s) == {'momentum_buffer'} for s in state.values())
    out = {'meta': np.array(json.dumps({
        'name': name, 'class': 'SartorrasEGNN', 'kwargs': mgt.KW, 'ctor': ctor, 'seed': SEED, 'lr': 2e-3, 'wd': 1e-4,
        'phases': [('classification', len(loader), EPOCHS)], 'tasks': ['classification'] * len(steps),
        'p_epoch': model.p_epoch, 'a_epoch': model.a_epoch, 'global_iter': model.global_iter,
        'checkpoints': ckpts, 'checkpoint_keys': sorted(ck.keys()),
        'optimiser_state_keys': ['momentum_buffer'], 'n_momentum_buffers': len(state)})),
        'loss': np.array([s[0] for s in steps], dtype=np.float64),
        'lr': np.array([s[1] for s in steps], dtype=np.float64),
        'momentum': np.array([s[2] for s in steps], dtype=np.float64)}
    for k, v in sd0.items():
        out[f'sd0/{k}'] = v
    for k, v in model.state_dict().items():
        out[f'sd1/{k}'] = v.detach().numpy()
    for bi, b in enumerate(list.__iter__(loader)):
        pre = f'in/p0b{bi}/'
        out[pre + 'x'] = b.x.numpy().astype(np.float32)
        out[pre + 'pos'] = b.pos.numpy().astype(np.float32)
        out[pre + 'edge_index'] = b.edge_index.numpy().astype(np.int32)
        out[pre + 'edge_type'] = b.edge_attr.argmax(1).numpy().astype(np.uint8)
        out[pre + 'batch'] = b.batch.numpy().astype(np.int32)
        out[pre + 'y'] = b.y.numpy().astype(np.float32)
    path = HERE / f'train_{name}.npz'
    np.savez_compressed(path, **out)
    print(f'{name:14s} steps={len(steps)} loss {steps[0][0]:.6f} -> {steps[-1][0]:.6f}  lr {steps[0][1]:.3e} .. '
          f'{max(s[1] for s in steps):.3e}  momentum {min(s[2] for s in steps):.3f} .. {max(s[2] for s in steps):.3f}  '
          f'ckpts={ckpts}  {path.stat().st_size / 1024:.0f} KiB')


def spread(name, ctor, n_perms=2):
    """Worst relative loss distance between the reference's run and its runs on the same batches with the edge lists
    in another (seeded) order."""
    def losses(perm_seed):
        loader = mgt.batches(100)
        if perm_seed is not None:
            gen = torch.Generator().manual_seed(perm_seed)
            for b in list.__iter__(loader):
                perm = torch.randperm(b.edge_index.shape[1], generator=gen)
                b.edge_index, b.edge_attr = b.edge_index[:, perm].contiguous(), b.edge_attr[perm].contiguous()
        with tempfile.TemporaryDirectory() as tmp:
            return np.array([s[0] for s in train(ctor, loader, tmp)[2]])
    base = losses(None)
    worst = max(float((np.abs(losses(20260404 + k) - base) / np.abs(base)).max()) for k in range(n_perms))
    print(f'{name:14s} worst relative loss distance over {len(base)} steps, {n_perms} edge orders: {worst:.2e}')
    return worst


def main():
    for name, ctor in SCHEDULES.items():
        if '--spread' in sys.argv[1:]:
            spread(name, ctor)
        else:
            run(name, ctor)


if __name__ == '__main__':
    main()
