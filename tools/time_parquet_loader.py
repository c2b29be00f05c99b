#!/usr/bin/env python
"""Graphs/s of the parquet data-root loader (pointvs_amd/parquet_data.py) at the CLI defaults (radius 10, edge radius 4,
smina types, non-compact, batch 32) over the fixture root tests/golden/dataroot repeated to 512 samples:

  (a) loader    one pass over the ComplexLoader alone (batches built on the GPU, nothing consumes them)
  (b) epoch     one epoch of `train_model` (eager, 6 layers, 32 channels) on that loader
  (c) step      for (a)'s comparison: the eager training step alone on the same 16 batches, built beforehand
  (d) host      for scale, the same samples built on the host in this process with pandas + scipy
                (read_parquet x 2, cdist crop, cdist edges - what the reference's __getitem__ does), first 64 samples

Each leg: one untimed pass, then 3 timed passes by the host clock between device synchronisations; medians.

    python tools/time_parquet_loader.py [--out profiles/parquet_loader_time.txt]
"""
import argparse
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
DATAROOT = ROOT / 'tests' / 'golden' / 'dataroot'


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def median_of(fn, dev, repeats=3):
    timed(fn, dev)
    return statistics.median(timed(fn, dev)[0] for _ in range(repeats))


def host_sample(root, rec, lig, radius, edge_radius):
    import pandas as pd
    from scipy.spatial.distance import cdist
    l, r = pd.read_parquet(root / lig), pd.read_parquet(root / rec)
    lx, rx = l[['x', 'y', 'z']].to_numpy(), r[['x', 'y', 'z']].to_numpy()
    r = r[(cdist(lx, rx) < radius).any(axis=0)]
    s = pd.concat([l, r], ignore_index=True)
    s = s[s['atomic_number'] > 1]
    xyz = s[['x', 'y', 'z']].to_numpy()
    d = cdist(xyz, xyz)
    return len(s), int(((d < edge_radius) & (d > 1e-7)).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'parquet_loader_time.txt'))
    ap.add_argument('--samples', type=int, default=512)
    args = ap.parse_args()
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.parquet_data import get_data_loader
    dev = torch.device('cuda:0')
    lines = (DATAROOT / 'chembl6.types').read_text().splitlines()
    with tempfile.TemporaryDirectory() as tmp:
        types = Path(tmp) / 'repeated.types'
        types.write_text('\n'.join(lines[k % len(lines)] for k in range(args.samples)) + '\n')
        loader = get_data_loader(DATAROOT, types_fname=types, mode='train', batch_size=32, radius=10, edge_radius=4,
                                 compact=False, use_atomic_numbers=False, polar_hydrogens=False, rot=False, device=dev)
        n = len(loader.dataset)
        torch.manual_seed(0)
        model = SartorrasEGNN(Path(tmp) / 'run', 2e-3, 1e-4, silent=True, k=32, num_layers=6,
                              dim_input=loader.dataset.feature_dim, dim_output=1, model_task='classification',
                              only_save_best_models=True).cuda()      # (no checkpoint write inside the timed epochs)
        t_loader = median_of(lambda: sum(b.num_graphs for b in loader), dev)
        t_epoch = median_of(lambda: model.train_model(loader, epochs=model.p_epoch + 1), dev)    # one more epoch
        batches = list(loader)
        t_step = median_of(lambda: model.train_model(batches, epochs=model.p_epoch + 1), dev)
        rows = [ln.split() for ln in lines]
        n_host = 64
        t0 = time.perf_counter()
        for k in range(n_host):
            host_sample(DATAROOT, rows[k % len(rows)][3], rows[k % len(rows)][4], 10, 4)
        t_host = time.perf_counter() - t0
    nodes = float(np.mean([b.x.shape[0] for b in batches])) / 32
    text = '\n'.join([
        f'parquet data-root loader, {n} samples (fixture root repeated), batch 32, CLI defaults, {nodes:.0f} nodes per graph',
        f'device {torch.cuda.get_device_name(0)}; medians of 3 after one untimed pass',
        f'(a) loader alone            {n / t_loader:10.0f} graphs/s   ({1e6 * t_loader / n:.1f} us per graph)',
        f'(b) train_model, one epoch  {n / t_epoch:10.0f} graphs/s   ({1e6 * t_epoch / n:.1f} us per graph)',
        f'(c) eager step, same batches{n / t_step:10.0f} graphs/s   ({1e6 * t_step / n:.1f} us per graph)',
        f'(d) host pandas + scipy     {n_host / t_host:10.0f} graphs/s   ({1e6 * t_host / n_host:.1f} us per graph, {n_host} samples)',
        f'loader / step = {t_loader / t_step:.2f}; loader vs host = {(n / t_loader) / (n_host / t_host):.0f}x', ''])
    print(text)
    Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
