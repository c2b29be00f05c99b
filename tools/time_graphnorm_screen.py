#!/usr/bin/env python
"""`run_library` on a GraphNorm model with and without `padded_graphnorm` (cfg5 receptor; the cfg2 model - k = 32,
3 layers - with graphnorm=True; 512 ligands of 8..64 atoms, fixed seed, 9 poses each; batch 128: 36 dense batches).

The legs this tree has, alternating, one untimed run each (probes, buffers, the capture) and then 3 timed ones; a run is
timed by the host clock from the call to a device synchronise after it:

  off      padded_graphnorm left off: one eager step per batch at the batch's exact node count
  padded   padded_graphnorm=True: one captured step for every batch, GraphNorm's statistics over a device row count

On a tree whose ScreeningSweep does not take the keyword (the parent of the commit that added it) only the first leg
runs, labelled `parent`: run the tool from that tree in the same session for the regression leg. Then, on a tree with
the keyword: the captured step alone (device events around 50 replays of one loaded batch, median of 5) for the
GraphNorm model and for its twin without GraphNorm - the price of GraphNorm's extra launches per layer (the first
product without its SiLU epilogue, two column reductions with their slab reductions, the shift, the tail).

    python tools/time_graphnorm_screen.py [--out profiles/graphnorm_screen_time.txt] [--append]
"""
import argparse
import inspect
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
    return [(f'lig{k}', lig_feats[:n].roll(k, 0).contiguous(),
             random_poses(lig[:n], n_poses, seed=seed + k, max_shift=6.0, device=dev)) for k, n in enumerate(sizes)]


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def replay_time(screen, dev, replays=50, repeats=5):
    """Median milliseconds of one replay of the captured step on the batch loaded into `screen`."""
    samples = []
    for _ in range(repeats + 1):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(replays):
            screen.replay()
        end.record()
        torch.cuda.synchronize(dev)
        samples.append(start.elapsed_time(end) / replays)
    return statistics.median(samples[1:]), samples[1:]      # (the first round: warm-up)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'graphnorm_screen_time.txt'))
    ap.add_argument('--append', action='store_true', help='add to --out instead of replacing it')
    ap.add_argument('--ligands', type=int, default=512)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_graphnorm_screen.py measures on the GPU; none found')
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.screening import LibraryScreen, ScreeningSweep
    from pointvs_amd.synthetic import CONFIGS, screening_set
    dev = torch.device('cuda:0')
    cfg = CONFIGS['cfg2']
    lig30, rec, feats = screening_set()                # the cfg5 receptor
    rec_feats = feats[lig30.shape[0]:].to(dev)
    lig, _, feats64 = screening_set(seed=5064, n_lig=64)
    lig_feats = feats64[:64]
    rec = rec.to(dev)
    radius = cfg['graph']['edge_radius']

    def model(graphnorm):
        torch.manual_seed(0)
        return SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **dict(cfg['model'], graphnorm=graphnorm)).eval()

    gen = torch.Generator().manual_seed(20260405)
    sizes = torch.randint(8, 65, (args.ligands,), generator=gen).tolist()
    work = make_library(lig, lig_feats, sizes, 9, dev, seed=100)
    n_poses = sum(int(p.shape[0]) for _, _, p in work)
    has_switch = 'padded_graphnorm' in inspect.signature(ScreeningSweep.__init__).parameters
    legs = {'off': {}, 'padded': dict(padded_graphnorm=True)} if has_switch else {'parent': {}}
    gn = model(True)
    sweeps = {leg: ScreeningSweep(gn, rec, rec_feats, radius, args.batch, **kw) for leg, kw in legs.items()}
    calls = {leg: (lambda s=s: s.run_library(work, sigmoid=False)) for leg, s in sweeps.items()}
    times, scores, batches = {leg: [] for leg in legs}, {}, {}
    for leg, call in calls.items():                    # untimed: the probe, the buffers, the capture
        timed(call, dev)
    for _ in range(args.repeats):
        for leg, call in calls.items():                # alternating
            before = sweeps[leg].batches_run
            t, scores[leg] = timed(call, dev)
            times[leg].append(t)
            batches[leg] = sweeps[leg].batches_run - before
    text = [f'# tools/time_graphnorm_screen.py: receptor {rec.shape[0]} atoms, radius {radius} A, 3-layer EGNN ch=32 with '
            f'GraphNorm, {len(work)} ligands of 8..64 atoms, {n_poses} poses, batch {args.batch}, '
            f'{torch.cuda.get_device_name(0)}']
    for leg in legs:
        runs = ' '.join(f'{t:.3f}' for t in times[leg])
        spread = (max(times[leg]) - min(times[leg])) / statistics.median(times[leg])
        text.append(f'{leg:8s} {n_poses / statistics.median(times[leg]):10.0f} poses/s (median of {args.repeats}; runs {runs} s; '
                    f'spread {100 * spread:.1f} % of the median)  {batches[leg]:4d} batches, captured: '
                    f'{bool(sweeps[leg].library._captured)}')
    if has_switch:
        diff = max(float((scores['off'][n] - scores['padded'][n]).abs().max()) for n, _, _ in work)
        top = max(float(scores['off'][n].abs().max()) for n, _, _ in work)
        text.append(f'ratio padded / off = {statistics.median(times["off"]) / statistics.median(times["padded"]):.2f}; '
                    f'max |raw score difference| = {diff:.2e} (largest |score| {top:.2e})')
        # the captured step alone: GraphNorm over the device count against the twin without GraphNorm
        from pointvs_amd.screening import plan_library
        first = plan_library([9] * len(sizes), sizes, args.batch, 64)[0]
        slots = [(work[k][1], work[k][2][pose]) for k, pose in first]
        step = {}
        for label, m, kw in (('graphnorm', gn, dict(padded_graphnorm=True)), ('twin', model(False), {})):
            screen = LibraryScreen(m, rec, rec_feats, args.batch, 64, radius, **kw).capture(slots)
            step[label] = replay_time(screen, dev)
            rounds = ' '.join(f'{t:.3f}' for t in step[label][1])
            text.append(f'captured step, {label:9s} {step[label][0]:.3f} ms per replay (median of 5 rounds of 50: {rounds})')
        text.append(f'GraphNorm costs {step["graphnorm"][0] - step["twin"][0]:.3f} ms per step '
                    f'({step["graphnorm"][0] / step["twin"][0]:.2f} x the twin)')
    text = '\n'.join(text) + '\n\n'
    print(text)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, 'a' if args.append else 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
