"""Training with edge dropout 0.25: eager, eager with the fixed-shape draw, and captured, at the real4A shape (the
reference's default: 6 layers, 32 channels, r = 4 A, ~500 atoms per graph; NOT a BASELINE configuration) and at cfg2.

    python tools/time_captured_dropout.py [--parent-tree DIR] [--epochs 12] [--repeats 3] [--out profiles/captured_dropout_time.txt]

Resident batches of 32 graphs (16 of them at real4A, 4 at cfg2), Adam, `dropout=0.25`, GraphNorm off (as in both
configurations). Rows per shape:
    eager, parent commit     train_model(capture=False) in a checkout of the parent commit with its own library built
                             (--parent-tree; without it the row is "not measured")
    eager                    the same here (static_dropout off: the draw sized by its result, one host read per step)
    eager, static_dropout    train_model(capture=False) with model.static_dropout = True
    captured                 train_model(capture=True)
Every row runs in a process of its own (a tree is imported once per process). Steady-state time per step = (time of 4 +
`epochs` epochs - time of 4 epochs) / steps in between, so that under capture every counted step is a replay; median of
`repeats` such measurements. The fixed-shape rows do the work of the UNDROPPED graph every step (the dead slots are
edges too), so at a shape the device bounds they are expected to lose to the eager draw."""
import argparse
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
SHAPES = {'real4A': 16, 'cfg2': 4}       # resident batches per shape
ROWS = ('eager', 'eager, static_dropout', 'captured')


def measure(args):
    """Child: one row of one shape from the tree --tree; prints one JSON line."""
    sys.path.insert(0, str(Path(args.tree).resolve()))
    import torch
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.synthetic import CONFIGS, synthetic_batch
    cfg = CONFIGS[args.shape]
    n_batches = SHAPES[args.shape]
    loader = [synthetic_batch(cfg['cfg_id'], args.batch, first_graph=args.batch * k, **cfg['graph']).to('cuda')
              for k in range(n_batches)]

    save_path = Path(tempfile.mkdtemp(prefix='pvs_captured_dropout_'))      # (silent, no checkpoints: stays empty)

    def run(epochs):
        torch.manual_seed(0)
        model = SartorrasEGNN(save_path, 2e-3, 1e-4, silent=True,
                              **dict(cfg['model'], dropout=0.25))
        model.only_save_best_models = True            # no checkpoint writes inside the timed epochs
        if args.row == 'eager, static_dropout':
            model.static_dropout = True
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        losses = model.train_model(loader, epochs=epochs, capture=args.row == 'captured')
        torch.cuda.synchronize()
        return time.perf_counter() - t0, losses

    run(3)          # warm the process (first-use work of the library and of torch)
    per_step = []
    for _ in range(args.repeats):
        t_short, _ = run(4)
        t_long, losses = run(4 + args.epochs)
        per_step.append((t_long - t_short) / (args.epochs * n_batches))
    ms = statistics.median(per_step) * 1e3
    print(json.dumps(dict(shape=args.shape, row=args.row, step_ms=round(ms, 4),
                          steps_per_s=round(1e3 / ms, 1), graphs_per_s=round(args.batch / ms * 1e3, 1),
                          all_ms=[round(v * 1e3, 4) for v in per_step], last_loss=float(losses[-1]),
                          nodes=int(loader[0].x.shape[0]), edges=int(loader[0].edge_index.shape[1]),
                          device=torch.cuda.get_device_name(0))), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--parent-tree', default=None, help='checkout of the parent commit with its library built')
    ap.add_argument('--epochs', type=int, default=12)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--shapes', default='real4A,cfg2')
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'captured_dropout_time.txt'))
    ap.add_argument('--row', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--shape', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=str(ROOT), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.row is not None:
        return measure(args)

    rows, lines = [], []
    for shape in args.shapes.split(','):
        jobs = [('eager, parent commit', 'eager', args.parent_tree)] + [(row, row, str(ROOT)) for row in ROWS]
        for label, row, tree in jobs:
            if tree is None:
                lines.append(f'{shape:7s} {label:24s} not measured (no --parent-tree)')
                print(lines[-1], flush=True)
                continue
            tree = str(Path(tree).resolve())
            out = subprocess.run([sys.executable, str(Path(__file__).resolve()), '--row', row, '--shape', shape, '--tree', tree,
                                  '--epochs', str(args.epochs), '--batch', str(args.batch), '--repeats', str(args.repeats)],
                                 check=True, stdout=subprocess.PIPE, text=True, cwd=tree, timeout=600).stdout
            rec = dict(json.loads(out.strip().splitlines()[-1]), row=label)
            rows.append(rec)
            lines.append(f"{shape:7s} {label:24s} {rec['step_ms']:8.4f} ms/step  {rec['steps_per_s']:8.1f} steps/s  "
                         f"{rec['graphs_per_s']:9.1f} graphs/s  (N = {rec['nodes']}, E = {rec['edges']})")
            print(lines[-1], flush=True)
    summary = dict(dropout=0.25, batch=args.batch, epochs=args.epochs, repeats=args.repeats, batches=SHAPES, rows=rows)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text('# tools/time_captured_dropout.py: steady-state training step with dropout = 0.25, Adam; '
                              f'median of {args.repeats}\n' + '\n'.join(lines) + '\n' + json.dumps(summary) + '\n')


if __name__ == '__main__':
    main()
