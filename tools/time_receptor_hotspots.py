#!/usr/bin/env python
"""(GPU) Receptor hotspot map of the hits of a screen (cfg5 receptor, cfg2 layer stack with sigmoid edge attention,
`--hits` ligands of 8..64 atoms, one pose each: the library of tools/time_ligand_masking.py), two measurements:

  (a) hits per second, two ways:
        sweep     `ScreeningSweep.receptor_hotspots(hits, gnn_layer=1)`: the whole ligands as slots of ONE
                  LibraryScreen, the attention of layer 1 reduced inside the captured step (PF.contact_attention), one
                  copy to the host at the end
        per hit   `attribution.edge_attention(model, pos, x, edge_index, edge_attr, gnn_layer=1)` once per hit (one
                  forward and one [E] copy to the host each), then on the host the maximum over each receptor atom's
                  ligand-receptor edges and the mean over the hits. The hits' edge lists are made before the clock
                  starts.
      One untimed run of each (screen built, step captured), then 3 timed runs, alternating; a run is timed by the host
      clock from the call to a device synchronise after it. Also the largest difference between the two maps.
  (b) the captured step with the reduction against the same step without it: two LibraryScreens on the same full
      batch, one built with contact_attention=1, both captured; `--rounds` rounds of `--replays` replays each,
      alternating, timed with device events; median and minimum per replay.

    python tools/time_receptor_hotspots.py [--hits 256] [--batch 32] [--out profiles/receptor_hotspots_time.txt]
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
    from pointvs_amd.screening import LibraryScreen, ScreeningSweep
    from pointvs_amd.synthetic import CONFIGS, random_poses, screening_set
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
    sweep = ScreeningSweep(model, rec, rec_feats, radius, args.batch)
    complexes = []
    for _, lig_feats, pose in hits:
        pos, x = torch.cat([pose, rec], 0), torch.cat([lig_feats, rec_feats], 0)
        _, edge_index, edge_type = generate_edges(pos, x[:, -1], radius, radius, prune=False)
        contact = (edge_type == 1).cpu().numpy()
        rows = edge_index[0].cpu().numpy()[contact] - int(pose.shape[0])
        complexes.append((pos[None], x[None], edge_index, torch.nn.functional.one_hot(edge_type.long(), 3), contact,
                          rows))

    def through_sweep():
        out = sweep.receptor_hotspots(hits, gnn_layer=1)
        return out['mean'].cpu().numpy()

    def per_hit():
        total, count = np.zeros(n_rec), np.zeros(n_rec)
        for pos, x, edge_index, edge_attr, contact, rows in complexes:
            att = attribution.edge_attention(model, pos, x, edge_indices=edge_index, edge_attrs=edge_attr, gnn_layer=1)
            top = np.full(n_rec, -np.inf)
            keep = rows >= 0                            # the edges whose row is a receptor atom
            np.maximum.at(top, rows[keep], att[contact][keep])
            has = np.isfinite(top)
            total[has] += top[has]
            count += has
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.where(count > 0, total / count, np.nan)

    calls = {'sweep': through_sweep, 'per hit': per_hit}
    times, results = {k: [] for k in calls}, {}
    for call in calls.values():
        timed(call, dev)
    for _ in range(3):
        for key, call in calls.items():
            t, results[key] = timed(call, dev)
            times[key].append(t)
    same = np.array_equal(np.isnan(results['sweep']), np.isnan(results['per hit']))
    diff = float(np.nanmax(np.abs(results['sweep'] - results['per hit'])))
    rate = {k: len(hits) / statistics.median(v) for k, v in times.items()}
    lines = [f'## (a) {len(hits)} hits of 8..64 atoms ({sum(sizes)} ligand atoms), batch {args.batch}, '
             f'{-(-len(hits) // args.batch)} steps a run, layer 1']
    for key in calls:
        runs = ' '.join(f'{t:.3f}' for t in times[key])
        lines.append(f'{key:8s} {rate[key]:10.0f} hits/s (median of 3; runs {runs} s)')
    lines.append(f"ratio sweep / per hit = {rate['sweep'] / rate['per hit']:.2f}")
    lines.append(f'max |difference| between the two maps = {diff:.2e} (atoms without a contact agree: {same})')

    # (b) one full batch, the captured step with and without the reduction
    slots = [(f, p) for _, f, p in hits[:args.batch]]
    screens = {'with': LibraryScreen(model, rec, rec_feats, args.batch, 64, radius, contact_attention=1),
               'without': LibraryScreen(model, rec, rec_feats, args.batch, 64, radius)}
    for screen in screens.values():
        screen.capture(slots)
        screen.replay()
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
    for screen in screens.values():
        screen.check()
    lines += ['', f'## (b) the captured step of one batch of {args.batch} ligands, {args.rounds} rounds of {args.replays} '
                  'replays, alternating; ms per replay']
    for key, v in per_replay.items():
        lines.append(f'{key + " the reduction":22s} median {statistics.median(v):.4f}  min {min(v):.4f}')
    med = {k: statistics.median(v) for k, v in per_replay.items()}
    lines.append(f"the reduction costs {1e3 * (med['with'] - med['without']):.1f} us a step "
                 f"({100 * (med['with'] / med['without'] - 1):+.2f} %)")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'receptor_hotspots_time.txt'))
    ap.add_argument('--hits', type=int, default=256)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--replays', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_receptor_hotspots.py measures on the GPU; none found')
    dev = torch.device('cuda:0')
    text = [f'# tools/time_receptor_hotspots.py: receptor 1970 atoms, radius 10 A, 3-layer EGNN ch=32 with edge '
            f'attention, {torch.cuda.get_device_name(0)}', '']
    text += measure(args, dev) + ['']
    text = '\n'.join(text)
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
