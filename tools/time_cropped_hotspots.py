#!/usr/bin/env python
"""(GPU) Receptor hotspot maps of hits on a CROPPED sweep, at the shape of tools/time_receptor_hotspots.py (cfg5 receptor,
cfg2 layer stack with sigmoid edge attention, `--hits` ligands of 8..64 atoms, one pose each, batch 32, edge radius 10)
with crop_radius 10, for layer 1 and for 'cam'. Four measurements, three repetitions each, alternating; the spread of the
repetitions is the margin of every comparison:

  (a) hits per second of `ScreeningSweep(crop_radius=10, cropped_hotspots=True).receptor_hotspots(hits, ...)` against the
      same call on a sweep without crop_radius (the uncropped maps of the same tree).
  (b) the same cropped call against `attribution.edge_attention` / `attribution.cam` once per hit on the hits' cropped
      complexes (edge lists made before the clock starts; the per-atom maximum and the mean over the hits on the host),
      and the largest difference between the two maps.
  (c) the captured cropped step of one full batch with each reduction (contact_attention=1, contact_attention=-1,
      cam=True) against the same cropped step without one, timed with device events. On a tree whose LibraryScreen has no `cropped_maps` only the
      step without a reduction is measured (that leg runs on the parent commit too).
  (d) in the same run, the uncropped captured step with and without each reduction: the added time of the uncropped
      sibling is the yardstick for the added time of a cropped reduction.

    python tools/time_cropped_hotspots.py [--hits 256] [--batch 32] [--out profiles/cropped_hotspots_time.txt]
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

CROP = 10.0
REPS = 3


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def spread(values):
    return max(values) - min(values)


def alternate(calls, dev):
    """One untimed run of each call, then REPS timed runs, alternating: ({key: [seconds]}, {key: the last result})."""
    times, results = {k: [] for k in calls}, {}
    for call in calls.values():
        timed(call, dev)
    for _ in range(REPS):
        for key, call in calls.items():
            t, results[key] = timed(call, dev)
            times[key].append(t)
    return times, results


def step_times(screens, slots, args):
    """Captured steps of the same batch, REPS repetitions of `--rounds` rounds of `--replays` replays, alternating:
    {key: [median ms per replay of each repetition]}."""
    for screen in screens.values():
        screen.capture(slots)
        screen.replay()
    reps = {k: [] for k in screens}
    for _ in range(REPS):
        per_replay = {k: [] for k in screens}
        for _ in range(args.rounds):
            for key, screen in screens.items():
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(args.replays):
                    screen.replay()
                stop.record()
                stop.synchronize()
                per_replay[key].append(start.elapsed_time(stop) / args.replays)
        for key in screens:
            reps[key].append(statistics.median(per_replay[key]))
    for screen in screens.values():
        screen.check()
    return reps


def added(reps, base='without'):
    """Per reduction: (median added us a step, the margin: the spreads of both legs added)."""
    out = {}
    for key, v in reps.items():
        if key != base:
            out[key] = (1e3 * (statistics.median(v) - statistics.median(reps[base])), 1e3 * (spread(v) + spread(reps[base])))
    return out


def measure(args, dev):
    from pointvs_amd import attribution
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.radius_graph import generate_edges
    from pointvs_amd.screening import LibraryScreen, ScreeningSweep
    from pointvs_amd.synthetic import CONFIGS, random_poses, screening_set
    has_maps = 'cropped_maps' in inspect.signature(LibraryScreen.__init__).parameters
    cfg = CONFIGS['cfg2']
    lig30, rec, feats = screening_set()                # the cfg5 receptor
    rec_feats, rec = feats[lig30.shape[0]:].to(dev), rec.to(dev)
    n_rec = int(rec.shape[0])
    lig, _, feats64 = screening_set(seed=5064, n_lig=64)
    torch.manual_seed(0)
    model = SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True,
                          **dict(cfg['model'], edge_attention=True)).eval().to(dev)
    radius = cfg['graph']['edge_radius']
    sizes = torch.randint(8, 65, (args.hits,), generator=torch.Generator().manual_seed(20260405)).tolist()
    hits = [(f'lig{k}', feats64[:n].roll(k, 0).contiguous().to(dev),
             random_poses(lig[:n], 1, seed=100 + k, max_shift=6.0, device=dev)[0].contiguous())
            for k, n in enumerate(sizes)]
    lines = []
    slots = [(f, p) for _, f, p in hits[:args.batch]]
    # (layer -1 beside the two kinds asked for: uncropped, layer 1 reduces the short ligand-touching CSR and a later layer
    # the full one, as every cropped reduction does)
    kinds = {'layer 1': dict(contact_attention=1), 'layer -1': dict(contact_attention=-1), 'cam': dict(cam=True)}

    if has_maps:
        cropped = ScreeningSweep(model, rec, rec_feats, radius, args.batch, crop_radius=CROP, cropped_hotspots=True)
        whole = ScreeningSweep(model, rec, rec_feats, radius, args.batch)
        complexes, kept_counts = [], []
        for _, lig_feats, pose in hits:
            kept = (torch.cdist(pose.double(), rec.double()) < CROP).any(0).nonzero().reshape(-1)
            kept_counts.append(int(kept.numel()))
            pos, x = torch.cat([pose, rec[kept]], 0), torch.cat([lig_feats, rec_feats[kept]], 0)
            _, edge_index, edge_type = generate_edges(pos, x[:, -1], radius, radius, prune=False)
            contact = (edge_type == 1).cpu().numpy()
            rows = edge_index[0].cpu().numpy()[contact] - int(pose.shape[0])
            complexes.append((pos[None], x[None], edge_index, torch.nn.functional.one_hot(edge_type.long(), 3), contact,
                              rows, kept.cpu().numpy(), int(pose.shape[0])))
        lines.append(f'## {len(hits)} hits of 8..64 atoms ({sum(sizes)} ligand atoms), batch {args.batch}, '
                     f'{-(-len(hits) // args.batch)} steps a run; crop {CROP:g} keeps {min(kept_counts)}..'
                     f'{max(kept_counts)} (median {int(statistics.median(kept_counts))}) of {n_rec} receptor atoms')

        def per_hit(by_cam):
            total, count = np.zeros(n_rec), np.zeros(n_rec)
            for pos, x, edge_index, edge_attr, contact, rows, kept, n in complexes:
                if by_cam:
                    top = np.asarray(attribution.cam(model, pos, x, edge_indices=edge_index, edge_attrs=edge_attr),
                                     dtype=np.float64).reshape(-1)[n:]
                else:
                    att = attribution.edge_attention(model, pos, x, edge_indices=edge_index, edge_attrs=edge_attr,
                                                     gnn_layer=1)
                    top = np.full(len(kept), -np.inf)
                    on = rows >= 0                          # the edges whose row is a receptor atom
                    np.maximum.at(top, rows[on], att[contact][on])
                has = np.isfinite(top)
                total[kept[has]] += top[has]
                count[kept[has]] += 1
            with np.errstate(invalid='ignore', divide='ignore'):
                return np.where(count > 0, total / count, np.nan)

        for name, by_cam in (('layer 1', False), ('cam', True)):
            kw = dict(attribution='cam') if by_cam else dict(gnn_layer=1)
            calls = {'cropped sweep': lambda: cropped.receptor_hotspots(hits, **kw)['mean'].cpu().numpy(),
                     'uncropped sweep': lambda: whole.receptor_hotspots(hits, **kw)['mean'].cpu().numpy(),
                     'per hit, cropped': lambda: per_hit(by_cam)}
            times, results = alternate(calls, dev)
            rate = {k: len(hits) / statistics.median(v) for k, v in times.items()}
            lines += ['', f'## (a, b) {name}: hits per second, median of {REPS} runs']
            for key in calls:
                runs = ' '.join(f'{t:.3f}' for t in times[key])
                lines.append(f'{key:18s} {rate[key]:10.0f} hits/s (runs {runs} s, spread {spread(times[key]):.3f} s)')
            lines.append(f"ratio cropped / uncropped sweep = {rate['cropped sweep'] / rate['uncropped sweep']:.2f}")
            lines.append(f"ratio cropped sweep / per hit   = {rate['cropped sweep'] / rate['per hit, cropped']:.2f}")
            a, b = results['cropped sweep'], results['per hit, cropped']
            same = np.array_equal(np.isnan(a), np.isnan(b))
            lines.append(f'max |difference| between the cropped sweep and the per-hit map = '
                         f'{float(np.nanmax(np.abs(a - b))):.2e} (the same atoms have a value: {same})')

    # (c) the cropped captured step with each reduction against the same step without one
    screens = {'without': LibraryScreen(model, rec, rec_feats, args.batch, 64, radius, crop_radius=CROP)}
    if has_maps:
        for name, kw in kinds.items():
            screens[name] = LibraryScreen(model, rec, rec_feats, args.batch, 64, radius, crop_radius=CROP,
                                          cropped_maps=True, **kw)
    cropped_reps = step_times(screens, slots, args)
    lines += ['', f'## (c) the captured CROPPED step of one batch of {args.batch} ligands: {REPS} repetitions of '
                  f'{args.rounds} rounds of {args.replays} replays, alternating; median ms per replay of each repetition']
    for key, v in cropped_reps.items():
        label = 'without a reduction' if key == 'without' else f'with {key}'
        lines.append(f'{label:22s} {" ".join(f"{t:.4f}" for t in v)}  (median {statistics.median(v):.4f}, spread '
                     f'{spread(v):.4f})')
    if not has_maps:
        lines.append('this tree has no cropped_maps: the step without a reduction only')
        return lines
    # (d) the uncropped step with and without its reductions, in the same run
    screens = {'without': LibraryScreen(model, rec, rec_feats, args.batch, 64, radius)}
    for name, kw in kinds.items():
        screens[name] = LibraryScreen(model, rec, rec_feats, args.batch, 64, radius, **kw)
    whole_reps = step_times(screens, slots, args)
    lines += ['', '## (d) the captured UNCROPPED step of the same batch, the same way']
    for key, v in whole_reps.items():
        label = 'without a reduction' if key == 'without' else f'with {key}'
        lines.append(f'{label:22s} {" ".join(f"{t:.4f}" for t in v)}  (median {statistics.median(v):.4f}, spread '
                     f'{spread(v):.4f})')
    lines += ['', '## the added time of a reduction, us a step (median with - median without; margin: both spreads)']
    for name in kinds:
        c, cm = added(cropped_reps)[name]
        u, um = added(whole_reps)[name]
        verdict = ('costs MORE than its uncropped sibling beyond the spread' if c - u > cm + um else
                   'costs less than its uncropped sibling beyond the spread' if u - c > cm + um else
                   'is within the spread of its uncropped sibling')
        lines.append(f'{name:8s} cropped {c:+7.1f} (+- {cm:.1f})   uncropped {u:+7.1f} (+- {um:.1f})   the cropped '
                     f'reduction {verdict}')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'cropped_hotspots_time.txt'))
    ap.add_argument('--hits', type=int, default=256)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--replays', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_cropped_hotspots.py measures on the GPU; none found')
    dev = torch.device('cuda:0')
    text = [f'# tools/time_cropped_hotspots.py: receptor 1970 atoms, edge radius 10 A, crop radius {CROP:g} A, 3-layer '
            f'EGNN ch=32 with edge attention, {torch.cuda.get_device_name(0)}', '']
    text += measure(args, dev) + ['']
    text = '\n'.join(text)
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
