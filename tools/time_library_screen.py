#!/usr/bin/env python
"""Library screening against per-ligand screening on the same libraries (cfg5 receptor, cfg2 model, batch 128):

  mixed    512 ligands, sizes uniform in 8..64 (fixed seed), 9 poses each: `ScreeningSweep.run` launches one padded
           batch per ligand (512), `run_library` ceil(4608 / 128) = 36 dense mixed batches
  control  36 ligands of 30 atoms with exactly 128 poses each: both paths launch 36 full batches of the same work
  wide     (--wide) 128 ligands, sizes uniform in 65..200 (fixed seed), 9 poses each: `run_library` at its default
           boundary of 64 atoms sends every ligand through its size bucket (128 padded batches, a captured step per
           size), `run_library(max_lig_atoms=200)` streams them in ceil(1152 / 128) = 9 dense mixed batches

Each path: one untimed run (buckets built, steps captured), then 3 timed runs, the two paths alternating; a run is
timed by the host clock from the call to a device synchronise after it (the predictions file is complete by then:
the writer is closed inside the call). Reports the median poses/s of both paths, their ratio and the batches
launched, and the largest difference between the two paths' scores.

    python tools/time_library_screen.py [--wide] [--out profiles/library_screen_time.txt]
"""
import argparse
import statistics
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def make_library(lig, lig_feats, sizes, n_poses, dev, seed):
    from pointvs_amd.synthetic import random_poses
    work = []
    for k, n in enumerate(sizes):
        # a ligand of n atoms: the n ligand points nearest the centre, its own feature rows
        poses = random_poses(lig[:n], n_poses, seed=seed + k, max_shift=6.0, device=dev)
        work.append((f'lig{k}', lig_feats[:n].roll(k, 0).contiguous(), poses))
    return work


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def measure(name, work, model, rec, rec_feats, radius, batch, out_dir, dev, repeats=3, paths=None):
    """paths: {label: (ScreeningSweep method name, its keyword arguments)}, two of them: the baseline first."""
    from pointvs_amd.screening import ScreeningSweep
    n_poses = sum(int(p.shape[0]) for _, _, p in work)
    paths = paths or {'run': ('run', {}), 'run_library': ('run_library', {})}
    base, other = paths
    sweeps = {key: ScreeningSweep(model, rec, rec_feats, radius, batch) for key in paths}
    files = {key: out_dir / f'{name}_{k}.txt' for k, key in enumerate(paths)}
    calls = {key: (lambda key=key, method=method, kw=kw: getattr(sweeps[key], method)(
        work, predictions_file=files[key], **kw)) for key, (method, kw) in paths.items()}
    times, scores, batches = {k: [] for k in calls}, {}, {}
    for key, call in calls.items():                    # untimed: buckets, probes, captures
        timed(call, dev)
    for _ in range(repeats):
        for key, call in calls.items():                # alternating
            before = sweeps[key].batches_run
            t, scores[key] = timed(call, dev)
            times[key].append(t)
            batches[key] = sweeps[key].batches_run - before
    diff = max(float((scores[base][n] - scores[other][n]).abs().max()) for n, _, _ in work)
    lines_equal = files[base].read_text() == files[other].read_text()
    rate = {k: n_poses / statistics.median(v) for k, v in times.items()}
    lines = [f'## {name}: {len(work)} ligands, {n_poses} poses, batch {batch}']
    for key in calls:
        runs = ' '.join(f'{t:.3f}' for t in times[key])
        lines.append(f'{key:{max(12, *map(len, paths))}s} {rate[key]:10.0f} poses/s (median of {repeats}; runs {runs} s)  '
                     f'{batches[key]:4d} batches launched')
    lines.append(f'ratio {other} / {base} = {rate[other] / rate[base]:.2f}')
    lines.append(f'max |score difference| between the paths = {diff:.2e}; predictions files identical: {lines_equal}')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'library_screen_time.txt'))
    ap.add_argument('--ligands', type=int, default=512)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--wide', action='store_true', help='also the leg with ligands of 65..200 atoms')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_library_screen.py measures on the GPU; none found')
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.synthetic import CONFIGS, screening_set
    dev = torch.device('cuda:0')
    cfg = CONFIGS['cfg2']
    lig30, rec, feats = screening_set()                # the cfg5 receptor
    rec_feats = feats[lig30.shape[0]:].to(dev)
    lig, _, feats64 = screening_set(seed=5064, n_lig=64)    # ligand atoms: the 64 innermost points of another cloud
    lig_feats = feats64[:64]
    rec = rec.to(dev)
    torch.manual_seed(0)
    model = SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **cfg['model']).eval()
    gen = torch.Generator().manual_seed(20260405)
    sizes = torch.randint(8, 65, (args.ligands,), generator=gen).tolist()
    radius = cfg['graph']['edge_radius']
    out_dir = Path(tempfile.mkdtemp())
    text = [f'# tools/time_library_screen.py: receptor {rec.shape[0]} atoms, radius {radius} A, 3-layer EGNN ch=32, '
            f'{torch.cuda.get_device_name(0)}', '']
    mixed = make_library(lig, lig_feats, sizes, 9, dev, seed=100)
    text += measure('mixed', mixed, model, rec, rec_feats, radius, args.batch, out_dir, dev) + ['']
    del mixed
    control = make_library(lig, lig_feats, [30] * 36, args.batch, dev, seed=9000)
    text += measure('control', control, model, rec, rec_feats, radius, args.batch, out_dir, dev) + ['']
    if args.wide:
        del control
        wide_lig, _, wide_feats = screening_set(seed=5200, n_lig=200)
        wide_sizes = torch.randint(65, 201, (max(args.ligands // 4, 1),), generator=gen).tolist()
        wide = make_library(wide_lig, wide_feats[:200], wide_sizes, 9, dev, seed=20000)
        text += measure('wide', wide, model, rec, rec_feats, radius, args.batch, out_dir, dev,
                        paths={'run_library': ('run_library', {}),
                               'run_library(max_lig_atoms=200)': ('run_library', dict(max_lig_atoms=200))}) + ['']
    text = '\n'.join(text)
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
