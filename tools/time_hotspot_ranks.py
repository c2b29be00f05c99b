#!/usr/bin/env python
"""(GPU) Receptor hotspot maps from atom masking and by rank, at the shape of tools/time_receptor_hotspots.py (cfg5
receptor, cfg2 layer stack with sigmoid edge attention, `--hits` ligands of 8..64 atoms, one pose each, batch 32);
medians of 3 runs, a run timed by the host clock from the call to a device synchronise after it:

  (1) `receptor_hotspots(attribution='atom_masking', atoms='contacts')` through the sweep against
      `attribution.masked_outputs` once per hit - the same copies: the whole complex, its ligand atoms and its contact
      receptor atoms left out one at a time - with the score differences reduced on the host. The per-hit leg runs the
      first `--per-hit` hits only (a hit has some hundred copies of a 2,000-node graph); hits/s and graphs/s for both.
  (2) every attribution with use_rank=True against the same call without it, the added time per batch, and
      PF.hit_value_ranks alone on [batch, n_rec] rows (a batch's cam values; with and without the ligand values)
      against torch's argsort(argsort(-rows)) on the same rows, timed with device events.
  (3) the default `receptor_hotspots` call and its captured step: 3 repetitions of `--rounds` rounds of `--replays`
      replays. `--parent TREE` repeats (3) on the package of a built checkout of the parent commit, in a process of
      its own; the margin is the spread of the three repetitions.

    python tools/time_hotspot_ranks.py [--hits 256] [--batch 32] [--parent TREE] [--out profiles/hotspot_ranks_time.txt]
"""
import argparse
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def three(calls, dev):
    """{key: [3 times]} of the calls, alternating, after one untimed run of each."""
    times = {k: [] for k in calls}
    for call in calls.values():
        timed(call, dev)
    for _ in range(3):
        for key, call in calls.items():
            times[key].append(timed(call, dev)[0])
    return times


def runs(v):
    return f"runs {' '.join(f'{t:.3f}' for t in v)} s, spread {max(v) - min(v):.3f} s"


def setup(args, dev):
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.screening import ScreeningSweep
    from pointvs_amd.synthetic import CONFIGS, random_poses, screening_set
    cfg = CONFIGS['cfg2']
    lig30, rec, feats = screening_set()                # the cfg5 receptor
    rec_feats, rec = feats[lig30.shape[0]:].to(dev), rec.to(dev)
    lig, _, feats64 = screening_set(seed=5064, n_lig=64)
    torch.manual_seed(0)
    model = SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True,
                          **dict(cfg['model'], edge_attention=True)).eval().to(dev)
    radius = cfg['graph']['edge_radius']
    sizes = torch.randint(8, 65, (args.hits,), generator=torch.Generator().manual_seed(20260405)).tolist()
    hits = [(f'lig{k}', feats64[:n].roll(k, 0).contiguous().to(dev),
             random_poses(lig[:n], 1, seed=100 + k, max_shift=6.0, device=dev)[0].contiguous())
            for k, n in enumerate(sizes)]
    return model, rec, rec_feats, radius, hits, ScreeningSweep(model, rec, rec_feats, radius, args.batch)


def default_leg(args, dev):
    """Leg (3) on whatever package is importable: the default call's times and the captured step's medians."""
    from pointvs_amd.screening import LibraryScreen
    model, rec, rec_feats, radius, hits, sweep = setup(args, dev)
    call = three({'default': lambda: sweep.receptor_hotspots(hits)['mean'].cpu()}, dev)['default']
    screen = LibraryScreen(model, rec, rec_feats, args.batch, 64, radius, contact_attention=1)
    screen.capture([(f, p) for _, f, p in hits[:args.batch]])
    screen.replay()
    step = []
    for _ in range(3):
        per_replay = []
        for _ in range(args.rounds):
            start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            for _ in range(args.replays):
                screen.replay()
            stop.record()
            stop.synchronize()
            per_replay.append(start.elapsed_time(stop) / args.replays)
        step.append(statistics.median(per_replay))
    screen.check()
    return dict(call=call, step=step)


def default_lines(name, leg, n_hits):
    call, step = leg['call'], leg['step']
    return [f'{name:8s} the call  {n_hits / statistics.median(call):10.0f} hits/s ({runs(call)})',
            f"{name:8s} the step  {' '.join(f'{t:.4f}' for t in step)} ms per replay  (median "
            f'{statistics.median(step):.4f}, spread {max(step) - min(step):.4f})']


def masking_leg(args, dev, model, rec, rec_feats, radius, hits, sweep):
    from pointvs_amd import attribution
    from pointvs_amd.radius_graph import generate_edges
    n_rec = int(rec.shape[0])
    few = hits[:args.per_hit]
    complexes = []
    for _, lig_feats, pose in few:
        n = int(pose.shape[0])
        pos, x = torch.cat([pose, rec], 0), torch.cat([lig_feats, rec_feats], 0)
        _, edge_index, edge_type = generate_edges(pos, x[:, -1], radius, radius, prune=False)
        rows = edge_index[0][edge_type == 1]
        atoms = torch.unique(rows[rows >= n]).cpu().numpy()          # the contact receptor atoms, as node rows
        drop = np.concatenate([np.arange(n), atoms])
        complexes.append((pos[None], x[None], edge_index, torch.nn.functional.one_hot(edge_type.long(), 3),
                          np.stack([drop, np.full(len(drop), -1)], 1), atoms - n))

    def through_sweep(items=hits):
        out = sweep.receptor_hotspots(items, attribution='atom_masking', sigmoid=False)
        return out['mean'].cpu().numpy()

    def per_hit():
        total, count = np.zeros(n_rec), np.zeros(n_rec)
        for pos, x, edge_index, edge_attr, drop, atoms in complexes:
            original, masked = attribution.masked_outputs(model, pos, x, drop, 32, edge_index, edge_attr)
            scores = (original.reshape(-1)[0] - masked[:, 0]).cpu().numpy()
            total[atoms] += scores[len(drop) - len(atoms):]
            count[atoms] += 1
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.where(count > 0, total / count, np.nan)

    times = three({'sweep': through_sweep, 'per hit': per_hit}, dev)
    # (the last timed run left the raw rows of all hits: one per copy, the whole complex twice)
    graphs = {'sweep': sum(int(v.shape[0]) for raw in (sweep.receptor_atom_masking_raw, sweep.atom_masking_raw)
                           for v in raw.values()),
              'per hit': sum(len(c[4]) + 1 for c in complexes)}
    a, b = through_sweep(few), per_hit()
    same = np.array_equal(np.isnan(a), np.isnan(b))
    diff = float(np.nanmax(np.abs(a - b)))
    n = {'sweep': len(hits), 'per hit': len(few)}
    lines = [f"## (1) attribution='atom_masking', atoms='contacts': the sweep over {len(hits)} hits ({graphs['sweep']} "
             f"graphs), attribution.masked_outputs per hit over the first {len(few)} ({graphs['per hit']} graphs)"]
    rate = {}
    for key, v in times.items():
        med = statistics.median(v)
        rate[key] = n[key] / med
        lines.append(f'{key:8s} {rate[key]:10.1f} hits/s {graphs[key] / med:10.0f} graphs/s (median of 3; {runs(v)})')
    lines.append(f"ratio sweep / per hit = {rate['sweep'] / rate['per hit']:.2f} (hits/s)")
    lines.append(f'max |difference| between the two maps of the first {len(few)} hits = {diff:.2e} (the same atoms '
                 f'have a value: {same})')
    return lines


def rank_leg(args, dev, hits, sweep):
    from pointvs_amd import functional as PF
    lines = ['', f'## (2) use_rank=True against the same call without it, {len(hits)} hits, '
                 f'{-(-len(hits) // args.batch)} batches a run (atom_masking: one rank call over all hits)']
    for attribution in ('edge_attention', 'cam', 'atom_masking'):
        kw = dict(attribution=attribution)
        times = three({'values': lambda: sweep.receptor_hotspots(hits, **kw)['mean'].cpu(),
                       'ranks': lambda: sweep.receptor_hotspots(hits, use_rank=True, **kw)['rank_mean'].cpu()}, dev)
        med = {k: statistics.median(v) for k, v in times.items()}
        for key, v in times.items():
            lines.append(f'{attribution:14s} {key:6s} {len(hits) / med[key]:10.1f} hits/s ({runs(v)})')
        spread = sum(max(v) - min(v) for v in times.values())
        lines.append(f"{attribution:14s} use_rank adds {1e3 * (med['ranks'] - med['values']):.2f} ms a run "
                     f"(+- {1e3 * spread:.2f}), {1e6 * (med['ranks'] - med['values']) / -(-len(hits) // args.batch):.0f} "
                     'us a batch')
    # the operator alone, on a batch's cam values
    out = sweep.receptor_hotspots(hits[:args.batch], attribution='cam', per_hit=True)
    rows = out['per_hit'].contiguous()
    lig_val = torch.cat(list(out['ligand'].values()), 0).contiguous()
    lig_ptr = torch.tensor([0] + [int(v.shape[0]) for v in out['ligand'].values()]).cumsum(0).to(device=dev,
                                                                                                 dtype=torch.int32)
    acc = PF.new_contact_accumulators(rows.shape[1], dev)
    bufs = (torch.empty_like(rows), torch.empty_like(lig_val))
    ops = {'PF.hit_value_ranks, receptor and ligand': lambda: PF.hit_value_ranks(rows, lig_val, lig_ptr, out=bufs, acc=acc),
           'PF.hit_value_ranks, receptor alone': lambda: PF.hit_value_ranks(rows, out=(bufs[0], None), acc=acc),
           'torch argsort(argsort(-rows))': lambda: torch.argsort(torch.argsort(-rows, dim=1, stable=True), dim=1)}
    lines += ['', f'## (2) the operator alone on rows [{rows.shape[0]}, {rows.shape[1]}] (a batch of cam values; '
                  f'{lig_val.numel()} ligand values), 3 repetitions of {args.rounds} rounds of {args.replays} calls; us a call']
    for key, op in ops.items():
        op()
        reps = []
        for _ in range(3):
            per_call = []
            for _ in range(args.rounds):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(args.replays):
                    op()
                stop.record()
                stop.synchronize()
                per_call.append(1e3 * start.elapsed_time(stop) / args.replays)
            reps.append(statistics.median(per_call))
        lines.append(f"{key:42s} {' '.join(f'{t:.1f}' for t in reps)}  (median {statistics.median(reps):.1f}, spread "
                     f'{max(reps) - min(reps):.1f})')
    same = torch.equal(bufs[0], torch.argsort(torch.argsort(-rows, dim=1, stable=True), dim=1).float())
    lines.append(f'(receptor alone, no NaN in these rows: the two give the same ranks: {same})')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'hotspot_ranks_time.txt'))
    ap.add_argument('--hits', type=int, default=256)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--per-hit', type=int, default=8)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--replays', type=int, default=20)
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit: leg (3) on its package too')
    ap.add_argument('--default-leg-of', default=None, help='(internal) print leg (3) of the package in this tree as JSON')
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.default_leg_of).resolve() if args.default_leg_of else ROOT))
    if not torch.cuda.is_available():
        raise SystemExit('time_hotspot_ranks.py measures on the GPU; none found')
    dev = torch.device('cuda:0')
    if args.default_leg_of:
        print('LEG ' + json.dumps(default_leg(args, dev)))
        return
    text = [f'# tools/time_hotspot_ranks.py: receptor 1970 atoms, radius 10 A, 3-layer EGNN ch=32 with edge attention, '
            f'{torch.cuda.get_device_name(0)}', '']
    parts = setup(args, dev)
    text += masking_leg(args, dev, *parts)
    text += rank_leg(args, dev, parts[4], parts[5])
    del parts
    text += ['', f'## (3) the default call (edge_attention, no new argument) and its captured step of one batch of '
                 f'{args.batch}: 3 repetitions of {args.rounds} rounds of {args.replays} replays']
    text += default_lines('this', default_leg(args, dev), args.hits)
    if args.parent:
        cmd = [sys.executable, str(Path(__file__).resolve()), '--default-leg-of', args.parent, '--hits', str(args.hits),
               '--batch', str(args.batch), '--rounds', str(args.rounds), '--replays', str(args.replays)]
        res = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if res.returncode != 0:
            raise SystemExit(f'the parent leg failed:\n{res.stderr[-2000:]}')
        leg = json.loads(next(line for line in res.stdout.splitlines() if line.startswith('LEG '))[4:])
        text += default_lines('parent', leg, args.hits)
    else:
        text.append('parent   not measured yet (no --parent tree given)')
    text = '\n'.join(text + [''])
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
