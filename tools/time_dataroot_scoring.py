#!/usr/bin/env python
"""Times data-root scoring: `val()` as it always ran against `val(capture=True)` (one captured fixed-shape step per full
batch, pointvs_amd/captured_scoring.py), and the two batch builders alone.

Writes a synthetic data root to a temporary directory - 8 receptors of about 3,000 atoms on a jittered lattice with a
pocket, 256 ligands of 20-40 atoms in the pocket, a types file of 2,048 lines - and scores it with the command line's
default settings (crop radius 10 A, edge radius 4 A, smina types, batch 32, 6-layer EGNN of 32 channels with GraphNorm).
Every figure is complexes per second, the median of 5 runs after a warm-up run, synchronised, predictions written.

The eager legs use only what the tree before the fixed-shape scorer has, so the tool runs from that tree too (it then
prints those legs alone): `python tools/time_dataroot_scoring.py --label parent --out FILE --append`.
"""
import argparse
import inspect
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

N_RECEPTORS, N_LIGANDS, N_LINES, BATCH = 8, 256, 2048, 32


def write_root(root, rng):
    import pandas as pd
    (root / 'receptors').mkdir()
    (root / 'ligands').mkdir()

    def save(path, xyz, z, types, bp):
        pd.DataFrame({'x': xyz[:, 0], 'y': xyz[:, 1], 'z': xyz[:, 2], 'atomic_number': z.astype(np.int64),
                      'types': types.astype(np.int64), 'bp': bp}).to_parquet(path)

    grid = (np.arange(15) - 7) * 2.5
    lattice = np.array([(x, y, z) for x in grid for y in grid for z in grid])
    lattice = lattice[np.linalg.norm(lattice, axis=1) > 5.0]              # the pocket
    for r in range(N_RECEPTORS):
        keep = rng.permutation(len(lattice))[:3000 - 20 * r]
        xyz = lattice[np.sort(keep)] + rng.uniform(-0.4, 0.4, (len(keep), 3))
        save(root / 'receptors' / f'rec{r}.parquet', xyz, rng.choice([6, 7, 8, 16], len(xyz)),
             rng.integers(0, 11, len(xyz)), 1)
    for k in range(N_LIGANDS):
        n = int(rng.integers(20, 41))
        steps = rng.normal(size=(n, 3))
        xyz = np.cumsum(1.5 * steps / np.linalg.norm(steps, axis=1, keepdims=True), axis=0)
        xyz = xyz - xyz.mean(axis=0)
        xyz *= min(1.0, 4.5 / np.linalg.norm(xyz, axis=1).max())          # inside the pocket
        save(root / 'ligands' / f'lig{k}.parquet', xyz, rng.choice([6, 7, 8], n), rng.integers(0, 11, n), 0)
    lines = [f'{int(rng.integers(0, 2))} -1 -1.0 receptors/rec{int(rng.integers(N_RECEPTORS))}.parquet '
             f'ligands/lig{int(rng.integers(N_LIGANDS))}.parquet' for _ in range(N_LINES)]
    (root / 'bench.types').write_text('\n'.join(lines) + '\n')
    return root / 'bench.types'


def median_rate(run, n_items, runs=5):
    run()                                                                 # warm-up
    times = []
    for _ in range(runs):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        run()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    med = statistics.median(times)
    return n_items / med, med, times


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--label', default='this tree')
    ap.add_argument('--out', default=None, help='also write the lines to this file')
    ap.add_argument('--append', action='store_true')
    ap.add_argument('--layers', type=int, default=6)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args()

    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.parquet_data import get_data_loader
    out = []

    def say(line):
        print(line, flush=True)
        out.append(line)

    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        root = tmp / 'root'
        root.mkdir()
        types = write_root(root, np.random.default_rng(args.seed))
        loader = get_data_loader(root, types_fname=types, mode='val', batch_size=BATCH, rot=False, radius=10,
                                 edge_radius=4.0, estimate_bonds=False, use_atomic_numbers=False, polar_hydrogens=False,
                                 compact=False, device='cuda:0')
        ds = loader.dataset
        torch.manual_seed(args.seed)
        model = SartorrasEGNN(tmp / 'model', 2e-3, 1e-4, silent=True, k=32, num_layers=args.layers,
                              dim_input=ds.feature_dim, dim_output=1, model_task='classification').cuda().eval()
        order = list(range(len(ds)))
        batches = [order[k:k + BATCH] for k in range(0, len(order), BATCH)]
        first = ds.build_batch(batches[0], device='cuda:0')
        say(f'# tools/time_dataroot_scoring.py [{args.label}]: {N_LINES} complexes ({N_RECEPTORS} receptors of ~3,000 atoms, '
            f'{N_LIGANDS} ligands of 20-40), batch {BATCH}: first batch {int(first.x.shape[0])} nodes / '
            f'{int(first.edge_index.shape[1])} edges; {args.layers}-layer EGNN ch=32 with GraphNorm; '
            f'{torch.cuda.get_device_name(0)}')

        def line(tag, rate, med, times, note=''):
            spread = 100 * (max(times) - min(times)) / med
            say(f'{tag:<28}{rate:9.0f} complexes/s (median of {len(times)}: {med * 1e3:7.1f} ms per pass; runs '
                + ' '.join(f'{t * 1e3:.1f}' for t in times) + f' ms; spread {spread:.1f} %){note}')

        line('val() eager', *median_rate(lambda: model.val(loader, predictions_file=tmp / 'eager.txt'), N_LINES))

        def build_all():
            for indices in batches:
                ds.build_batch(indices, device='cuda:0')
        line('build_batch alone', *median_rate(build_all, N_LINES))

        if 'capture' not in inspect.signature(model.val).parameters:
            say('(this tree has no val(capture=True): eager legs only)')
        else:
            from pointvs_amd.captured_scoring import FixedShapeScorer
            rate = median_rate(lambda: model.val(loader, predictions_file=tmp / 'captured.txt', capture=True), N_LINES)
            line('val(capture=True)', *rate, note=f'    batches {model.last_val_stats}')
            eager = [ln.split() for ln in (tmp / 'pose_eager.txt').read_text().splitlines()]
            captured = [ln.split() for ln in (tmp / 'pose_captured.txt').read_text().splitlines()]
            same = [a[:2] + a[3:] for a in eager] == [b[:2] + b[3:] for b in captured]
            worst = max(abs(float(a[2]) - float(b[2])) for a, b in zip(eager, captured))
            say(f'files: {len(captured)} lines, labels and names identical: {same}; largest printed score difference '
                f'{worst:.3f}')
            scorer = FixedShapeScorer(model, ds, BATCH, device='cuda:0')
            say(f'capacities {tuple(scorer.capacities)}')

            def build_all_cap():
                for indices in batches:
                    scorer.load(indices)
                    scorer.build()
            line('capacity builders alone', *median_rate(build_all_cap, N_LINES))
    if args.out:
        with open(args.out, 'a' if args.append else 'w', encoding='utf-8') as f:
            f.write('\n'.join(out) + '\n\n')


if __name__ == '__main__':
    main()
