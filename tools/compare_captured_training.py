"""train_model under capture, everything it leaves behind, dumped by one package and compared with another's dump.

    python tools/compare_captured_training.py --dump OUT.pt [--tree DIR]     one process per package (DIR holds pointvs_amd/)
    python tools/compare_captured_training.py --compare A.pt B.pt            no GPU needed

Both packages can load one library (PVS_EGNN_LIB). Runs, at the shapes of tests/test_gpu_captured_dropout.py (_batches():
two graphs of 207 nodes / one graph of 30; without dropout the two-graph batches only, twice each), 3 epochs of 4
resident batches, a checkpoint written at every epoch end while the replayer is open:
    {adam, sgd} x {no schedule, use_1cycle, warm_restarts} x dropout {0, 0.25}, capture=True
    the same with capture=False and static_dropout=True for dropout 0.25
    one MultitaskSatorrasEGNN run (capture=True, dropout 0.25)
    one run that loads the epoch-1 checkpoint of a captured run and continues under capture
Dumped per run: losses, final parameters, optimiser.state_dict(), every checkpoint file, last_capture_stats, and the
(seed, step, n_kept) of model.last_dropout after every step. --compare: equal means dtype, shape and bytes for every
tensor, == for everything else."""
import argparse
import hashlib
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
KW = dict(dim_input=12, k=32, dim_output=1, num_layers=2, graphnorm=False, edge_attention=True)


class _Loader(list):
    """Resident batches; after every step, what the step drew."""

    def __init__(self, batches, model):
        super().__init__(batches)
        self.model, self.drawn = model, []

    def __iter__(self):
        for b in list.__iter__(self):
            yield b
            d = getattr(self.model, 'last_dropout', None)
            self.drawn.append(None if d is None else (int(d['seed']), int(d['step']), int(d['n_kept'])))


def _host(value):
    import torch
    if torch.is_tensor(value):
        return value.detach().cpu()
    if isinstance(value, dict):
        return {k: _host(v) for k, v in value.items()}
    if isinstance(value, (list, tuple)):
        return [_host(v) for v in value]
    return value


def _one_run(cls, optimiser='adam', schedule=None, dropout=0.0, capture=True, static=None, resume_from=None, epochs=3):
    import torch
    from tests.test_gpu_captured_dropout import _batches
    save_path = Path(tempfile.mkdtemp(prefix='pvs_compare_captured_'))
    torch.manual_seed(3)
    model = cls(save_path, 2e-3, 1e-4, None, None, silent=True, optimiser=optimiser, use_1cycle=schedule == 'use_1cycle',
                warm_restarts=schedule == 'warm_restarts', **dict(KW, dropout=dropout)).cuda().train()
    if static is not None:
        model.static_dropout = static
    if resume_from is not None:
        model.load_weights(resume_from)
    torch.manual_seed(77)
    # (without dropout a batch of ONE graph is not capturable: its [0, N] offsets are built from a host list in the
    # step, PNNGeometricBase._whole_ptr; with dropout they belong to the batch's plan)
    batches = _batches() + _batches()
    loader = _Loader(batches if dropout else batches[0::2] * 2, model)
    losses = model.train_model(loader, epochs=epochs, capture=capture)
    torch.cuda.synchronize()
    files = sorted((save_path / 'checkpoints').glob('*.pt'))
    out = dict(losses=torch.tensor(losses, dtype=torch.float64), parameters=_host(dict(model.named_parameters())),
               optimiser=_host(model.optimiser.state_dict()),
               checkpoints={f.name: _host(torch.load(f, map_location='cpu', weights_only=False)) for f in files},
               stats=dict(model.last_capture_stats) if capture else None, drawn=loader.drawn,
               static_dropout_after=model.__dict__.get('static_dropout', 'unset'))
    return out, files


def dump(args):
    sys.path[:0] = [str(Path(args.tree).resolve()), str(ROOT)]
    import torch
    import pointvs_amd
    from pointvs_amd.egnn_multitask import MultitaskSatorrasEGNN
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    assert Path(pointvs_amd.__file__).resolve().parent.parent == Path(args.tree).resolve(), pointvs_amd.__file__
    runs = {}
    for optimiser in ('adam', 'sgd'):
        for schedule in (None, 'use_1cycle', 'warm_restarts'):
            for dropout in (0.0, 0.25):
                name = f'{optimiser}_{schedule or "plain"}_p{dropout}'
                runs[f'{name}_captured'], files = _one_run(SartorrasEGNN, optimiser, schedule, dropout)
                if dropout:
                    runs[f'{name}_eager_static'], _ = _one_run(SartorrasEGNN, optimiser, schedule, dropout, capture=False,
                                                               static=True)
    runs['multitask_captured'], _ = _one_run(MultitaskSatorrasEGNN, dropout=0.25)
    _, files = _one_run(SartorrasEGNN, dropout=0.25, epochs=1)
    assert [f.name for f in files] == ['pose_ckpt_epoch_1.pt'], files
    runs['resumed_captured'], _ = _one_run(SartorrasEGNN, dropout=0.25, resume_from=files[0], epochs=4)
    for name, run in runs.items():
        print(f"{name:40s} {len(run['losses'])} steps, {len(run['checkpoints'])} checkpoints, {run['stats']}", flush=True)
    torch.save(dict(package=str(Path(pointvs_amd.__file__).parent), runs=runs), args.dump)


def _leaves(value, path=''):
    import torch
    if isinstance(value, dict):
        yield path + '{}', sorted(map(repr, value.keys()))
        for k in value:
            yield from _leaves(value[k], f'{path}/{k}')
    elif isinstance(value, (list, tuple)):
        yield path + '[]', len(value)
        for k, v in enumerate(value):
            yield from _leaves(v, f'{path}/{k}')
    elif torch.is_tensor(value):
        yield path, (str(value.dtype), tuple(value.shape), value.contiguous().reshape(-1).view(torch.uint8).numpy().tobytes()
                     if value.numel() else b'')
    else:
        yield path, value


def compare(args):
    import torch
    a, b = (torch.load(f, map_location='cpu', weights_only=False) for f in args.compare)
    print(f"A: {a['package']}\nB: {b['package']}")
    assert a['runs'].keys() == b['runs'].keys()
    all_equal = True
    for name in a['runs']:
        la, lb = list(_leaves(a['runs'][name])), list(_leaves(b['runs'][name]))
        digest = hashlib.sha256(repr(la).encode()).hexdigest()[:16]
        tensors = sum(isinstance(v, tuple) and len(v) == 3 and isinstance(v[2], bytes) for _, v in la)
        differ = [pa for (pa, va), (pb, vb) in zip(la, lb) if pa != pb or va != vb]
        equal = len(la) == len(lb) and not differ
        all_equal &= equal
        run = a['runs'][name]
        print(f"  {name:38s} {len(la):5d} values ({tensors} tensors, {len(run['checkpoints'])} checkpoints) sha256 {digest}  "
              f"{'EQUAL' if equal else 'DIFFERENT: ' + ', '.join(differ[:5])}   {run['stats'] or ''}")
    print('ALL EQUAL' if all_equal else 'NOT EQUAL')
    return 0 if all_equal else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--dump', default=None)
    ap.add_argument('--tree', default=str(ROOT))
    ap.add_argument('--compare', nargs=2, default=None)
    args = ap.parse_args()
    return compare(args) if args.compare else dump(args)


if __name__ == '__main__':
    sys.exit(main())
