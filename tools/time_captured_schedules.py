"""Eager against captured training under a learning-rate schedule, for Adam and for SGD, at the real4A shape (the
reference's default: 6 layers, 32 channels, r = 4 A, ~500 atoms per graph; NOT a BASELINE configuration).

    python tools/time_captured_schedules.py [--batches 16] [--epochs 12] [--batch 32] [--out profiles/captured_schedules_time.txt]

16 resident batches of 32 graphs, `use_1cycle=True` (OneCycleLR changes lr and beta1 / the momentum every step), all in
one process: per optimiser `train_model(capture=False)` and `train_model(capture=True)`; steady-state time per step =
(time of 4 + `epochs` epochs - time of 4 epochs) / steps in between, so that under capture every counted step is a replay
(a batch is replayed from its third visit on). Median of 3 such measurements. For SGD a third row times the eager loop
with `clip_grad_value_` + torch.optim.SGD in place of FusedClipSGD - the path `optimiser='sgd'` took before the fused
step existed. Prints one line per row and writes them, with a JSON summary, to --out."""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--batches', type=int, default=16)
    ap.add_argument('--epochs', type=int, default=12)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'captured_schedules_time.txt'))
    args = ap.parse_args()

    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.synthetic import CONFIGS, synthetic_batch
    cfg = CONFIGS['real4A']
    loader = [synthetic_batch(cfg['cfg_id'], args.batch, first_graph=args.batch * k, **cfg['graph']).to('cuda')
              for k in range(args.batches)]

    def run(optimiser, capture, epochs, torch_sgd=False):
        torch.manual_seed(0)
        model = SartorrasEGNN(Path('/tmp/pvs_captured_schedules'), 2e-3, 1e-4, silent=True, use_1cycle=True,
                              optimiser=optimiser, **cfg['model'])
        model.only_save_best_models = True            # no checkpoint writes inside the timed epochs
        if torch_sgd:
            group = model.optimiser.param_groups[0]
            model.optimiser = torch.optim.SGD(model.parameters(), lr=group['lr'], momentum=group['momentum'],
                                              weight_decay=group['weight_decay'], nesterov=group['nesterov'])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = model.train_model(loader, epochs=epochs, capture=capture)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, losses

    rows = []
    for optimiser, capture, torch_sgd, label in (('adam', False, False, 'adam  eager'), ('adam', True, False, 'adam  captured'),
                                                 ('sgd', False, False, 'sgd   eager'), ('sgd', True, False, 'sgd   captured'),
                                                 ('sgd', False, True, 'sgd   eager, torch.optim.SGD + clip_grad_value_')):
        run(optimiser, capture, 3, torch_sgd)          # warm the process (first-use work of the library and of torch)
        per_step = []
        for _ in range(args.repeats):
            t_short, _ = run(optimiser, capture, 4, torch_sgd)
            t_long, losses = run(optimiser, capture, 4 + args.epochs, torch_sgd)
            per_step.append((t_long - t_short) / (args.epochs * args.batches))
        ms = statistics.median(per_step) * 1e3
        rows.append(dict(row=label, step_ms=round(ms, 4), graphs_per_s=round(args.batch / ms * 1e3, 1),
                         all_ms=[round(v * 1e3, 4) for v in per_step], last_loss=float(losses[-1])))
        print(f"{label:48s} {ms:8.4f} ms/step  {args.batch / ms * 1e3:9.1f} graphs/s  (median of {args.repeats}; "
              f"last loss {losses[-1]:.6f})", flush=True)
    summary = dict(device=torch.cuda.get_device_name(0), config='real4A', schedule='use_1cycle', batches=args.batches,
                   batch=args.batch, epochs=args.epochs, repeats=args.repeats, rows=rows)
    lines = [f"{r['row']:48s} {r['step_ms']:8.4f} ms/step  {r['graphs_per_s']:9.1f} graphs/s" for r in rows]
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text('# tools/time_captured_schedules.py: steady-state training step, real4A shape, OneCycleLR; '
                              f"median of {args.repeats}\n" + '\n'.join(lines) + '\n' + json.dumps(summary) + '\n')


if __name__ == '__main__':
    main()
