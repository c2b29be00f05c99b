#!/usr/bin/env python
"""(GPU) Pose score and affinity of a two-headed model over a docking library, two ways (cfg5 receptor, cfg2 layer
stack as MultitaskSatorrasEGNN, 512 ligands of 8..64 atoms with 9 poses each, batch 128):

  one pass    `run_library(tasks='both', predictions_file=..., hits_file=...)`: one trunk pass, both heads from one
              pooling, the best pose of every ligand picked on the device
  two passes  the same library swept twice, `tasks='pose'` then `tasks='affinity'` (what two `set_task` passes cost),
              the scores copied to the host and every ligand's best pose picked there

One untimed run of each (buckets built, steps captured), then 3 timed runs, alternating; a run is timed by the host
clock from the call to a device synchronise after it. Reports the median poses/s of both, their ratio, the largest
difference between their scores and whether they pick the same poses.

`--cfg5 PARENT_TREE` adds the single-head guard: `bench.py --config cfg5` of a built checkout of the parent commit and
of this tree, alternately, 3 runs each, both medians and both spreads.

    python tools/time_two_head_screen.py [--cfg5 PARENT_TREE] [--out profiles/two_head_screen_time.txt]
"""
import argparse
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def two_heads(args, dev):
    from pointvs_amd.egnn_multitask import MultitaskSatorrasEGNN
    from pointvs_amd.screening import ScreeningSweep
    from pointvs_amd.synthetic import CONFIGS, random_poses, screening_set
    cfg = CONFIGS['cfg2']
    lig30, rec, feats = screening_set()                # the cfg5 receptor
    rec_feats, rec = feats[lig30.shape[0]:].to(dev), rec.to(dev)
    lig, _, feats64 = screening_set(seed=5064, n_lig=64)
    torch.manual_seed(0)
    model = MultitaskSatorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **cfg['model']).eval()
    gen = torch.Generator().manual_seed(20260405)
    sizes = torch.randint(8, 65, (args.ligands,), generator=gen).tolist()
    radius = cfg['graph']['edge_radius']
    # (the `mixed` library of tools/time_library_screen.py: ligand k = the n innermost ligand points, features rolled)
    work = [(f'lig{k}', feats64[:n].roll(k, 0).contiguous(), random_poses(lig[:n], 9, seed=100 + k, max_shift=6.0, device=dev))
            for k, n in enumerate(sizes)]
    n_poses = sum(int(p.shape[0]) for _, _, p in work)
    out_dir = Path(tempfile.mkdtemp())
    sweeps = {tasks: ScreeningSweep(model, rec, rec_feats, radius, args.batch, tasks=tasks)
              for tasks in ('both', 'pose', 'affinity')}

    def one_pass():
        scores = sweeps['both'].run_library(work, predictions_file=out_dir / 'one.txt', sigmoid=False,
                                            hits_file=out_dir / 'hits.txt')
        return scores, {name: best for name, (best, _) in sweeps['both'].hits.items()}

    def two_passes():
        pose = sweeps['pose'].run_library(work, predictions_file=out_dir / 'pose_two.txt', sigmoid=False)
        aff = sweeps['affinity'].run_library(work, predictions_file=out_dir / 'affinity_two.txt')
        scores = {name: torch.cat([pose[name], aff[name]], 1) for name in pose}
        host = {name: s.cpu() for name, s in scores.items()}
        lines, best = [], {}
        for name, s in host.items():
            best[name] = int(torch.argmax(s[:, 0]))
            lines.append(' '.join(f'{v:.3f}' for v in s[best[name]].tolist()) + f' | receptor {name}_pose{best[name]}')
        (out_dir / 'hits_two.txt').write_text('\n'.join(lines) + '\n')
        return scores, best

    calls = {'one pass': one_pass, 'two passes': two_passes}
    times, results = {k: [] for k in calls}, {}
    for call in calls.values():
        timed(call, dev)
    for _ in range(3):
        for key, call in calls.items():
            t, results[key] = timed(call, dev)
            times[key].append(t)
    (one, best_one), (two, best_two) = results['one pass'], results['two passes']
    diff = max(float((one[name] - two[name]).abs().max()) for name in one)
    rate = {k: n_poses / statistics.median(v) for k, v in times.items()}
    lines = [f'## two heads: {len(work)} ligands, {n_poses} poses, batch {args.batch}']
    for key in calls:
        runs = ' '.join(f'{t:.3f}' for t in times[key])
        lines.append(f'{key:10s} {rate[key]:10.0f} poses/s (median of 3; runs {runs} s)')
    lines.append(f"ratio one pass / two passes = {rate['one pass'] / rate['two passes']:.2f}")
    lines.append(f'max |score difference| between the two = {diff:.2e}; same best poses: {best_one == best_two}; '
                 f'hits files identical: {(out_dir / "hits.txt").read_text() == (out_dir / "hits_two.txt").read_text()}')
    return lines


def cfg5_guard(parent):
    """bench.py --config cfg5 of the parent's tree and of this one, alternately, three runs each."""
    trees = {'parent': Path(parent).resolve(), 'this commit': ROOT}
    values = {k: [] for k in trees}
    for _ in range(3):
        for key, tree in trees.items():
            out = subprocess.run([sys.executable, 'bench.py', '--config', 'cfg5', '--gpus', '1', '--sweep', '12800',
                                  '--warmup', '1'], cwd=tree, capture_output=True, text=True, timeout=600, check=True)
            values[key].append(float(json.loads(out.stdout.strip().splitlines()[-1])['value']))
    lines = ['## single-head guard: bench.py --config cfg5 --gpus 1 --sweep 12800 --warmup 1, alternating']
    for key, v in values.items():
        runs = ' '.join(f'{x:.0f}' for x in v)
        lines.append(f'{key:12s} median {statistics.median(v):10.0f} poses/s (runs {runs}; spread '
                     f'{(max(v) - min(v)) / statistics.median(v) * 100:.1f} %)')
    ratio = statistics.median(values['this commit']) / statistics.median(values['parent'])
    inside = min(values['parent']) <= statistics.median(values['this commit'])
    lines.append(f'this commit / parent = {ratio:.3f}; this commit\'s median at or above the parent\'s slowest run: {inside}')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'two_head_screen_time.txt'))
    ap.add_argument('--ligands', type=int, default=512)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--cfg5', metavar='PARENT_TREE', help='a built checkout of the parent commit')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_two_head_screen.py measures on the GPU; none found')
    dev = torch.device('cuda:0')
    text = [f'# tools/time_two_head_screen.py: receptor 1970 atoms, radius 10 A, 3-layer two-headed EGNN ch=32, '
            f'{torch.cuda.get_device_name(0)}', '']
    text += two_heads(args, dev) + ['']
    if args.cfg5:
        text += cfg5_guard(args.cfg5) + ['']
    text = '\n'.join(text)
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
