#!/usr/bin/env python
"""(GPU) Ligand-atom masking of the hits of a screen, two ways (cfg5 receptor, cfg2 layer stack, `--hits` ligands of
8..64 atoms, one pose each - the best poses a sweep ends with):

  screen      `ScreeningSweep.ligand_atom_masking(hits)`: every leave-one-atom-out copy of every hit as a slot of ONE
              LibraryScreen (receptor-receptor sums and template reused, one packer launch + one captured step per
              batch)
  per hit     `attribution.masked_outputs(model, pos, x, drop, bs)` once per hit, `drop` = that hit's ligand atoms only
              (the complex's graph prepared per call, a leave-out batch built from the whole CSR per chunk). The hits'
              edge lists are made before the clock starts.

One untimed run of each (screen built, step captured), then 3 timed runs, alternating; a run is timed by the host clock
from the call to a device synchronise after it. Reports the median leave-out graphs/s of both, their ratio and the
largest difference between their raw outputs.

    python tools/time_ligand_masking.py [--hits 256] [--batch 32] [--out profiles/ligand_masking_time.txt]
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


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def measure(args, dev):
    from pointvs_amd import attribution
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.radius_graph import generate_edges
    from pointvs_amd.screening import ScreeningSweep
    from pointvs_amd.synthetic import CONFIGS, random_poses, screening_set
    cfg = CONFIGS['cfg2']
    lig30, rec, feats = screening_set()                # the cfg5 receptor
    rec_feats, rec = feats[lig30.shape[0]:].to(dev), rec.to(dev)
    lig, _, feats64 = screening_set(seed=5064, n_lig=64)
    torch.manual_seed(0)
    model = SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **cfg['model']).eval().to(dev)
    radius = cfg['graph']['edge_radius']
    sizes = torch.randint(8, 65, (args.hits,), generator=torch.Generator().manual_seed(20260405)).tolist()
    hits = [(f'lig{k}', feats64[:n].roll(k, 0).contiguous().to(dev),
             random_poses(lig[:n], 1, seed=100 + k, max_shift=6.0, device=dev)[0].contiguous())
            for k, n in enumerate(sizes)]
    n_graphs = sum(sizes) + len(sizes)
    sweep = ScreeningSweep(model, rec, rec_feats, radius, args.batch)
    complexes = []
    for name, lig_feats, pose in hits:
        pos, x = torch.cat([pose, rec], 0), torch.cat([lig_feats, rec_feats], 0)
        _, edge_index, edge_type = generate_edges(pos, x[:, -1], radius, radius, prune=False)
        drop = np.stack([np.arange(pose.shape[0]), np.full(pose.shape[0], -1)], axis=1)
        complexes.append((name, pos[None], x[None], drop, edge_index, torch.nn.functional.one_hot(edge_type.long(), 3)))

    def screen():
        sweep.ligand_atom_masking(hits, sigmoid=False)
        return {name: raw.clone() for name, raw in sweep.atom_masking_raw.items()}

    def per_hit():
        out = {}
        for name, pos, x, drop, edge_index, edge_attr in complexes:
            original, masked = attribution.masked_outputs(model, pos, x, drop, args.batch, edge_indices=edge_index,
                                                          edge_attrs=edge_attr)
            out[name] = torch.cat([original.reshape(1, -1), masked], 0)
        return out

    calls = {'screen': screen, 'per hit': per_hit}
    times, results = {k: [] for k in calls}, {}
    for call in calls.values():
        timed(call, dev)
    for _ in range(3):
        for key, call in calls.items():
            t, results[key] = timed(call, dev)
            times[key].append(t)
    diff = max(float((results['screen'][name] - results['per hit'][name]).abs().max()) for name, _, _ in hits)
    top = max(float(results['per hit'][name].abs().max()) for name, _, _ in hits)
    rate = {k: n_graphs / statistics.median(v) for k, v in times.items()}
    lines = [f'## {len(hits)} hits of 8..64 atoms ({sum(sizes)} ligand atoms), {n_graphs} graphs, batch {args.batch}, '
             f'{-(-n_graphs // args.batch)} steps a run']
    for key in calls:
        runs = ' '.join(f'{t:.3f}' for t in times[key])
        lines.append(f'{key:8s} {rate[key]:10.0f} graphs/s (median of 3; runs {runs} s)')
    lines.append(f"ratio screen / per hit = {rate['screen'] / rate['per hit']:.2f}")
    lines.append(f'max |raw difference| between the two = {diff:.2e} (max |raw| {top:.2e})')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'ligand_masking_time.txt'))
    ap.add_argument('--hits', type=int, default=256)
    ap.add_argument('--batch', type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_ligand_masking.py measures on the GPU; none found')
    dev = torch.device('cuda:0')
    text = [f'# tools/time_ligand_masking.py: receptor 1970 atoms, radius 10 A, 3-layer EGNN ch=32, '
            f'{torch.cuda.get_device_name(0)}', '']
    text += measure(args, dev) + ['']
    text = '\n'.join(text)
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
