#!/usr/bin/env python
"""(GPU) Masking attribution of hits on a cropped sweep, `ScreeningSweep(crop_radius=10, cropped_attribution=True)`,
against three baselines (cfg5 receptor, cfg2 layer stack: k = 32, 3 layers, edge radius as tools/time_cropped_screen.py
uses; `--hits` ligands of 8..64 atoms, one pose each, batch 32):

  cropped     `ligand_atom_masking(hits)` and `contact_masking(hits)` of the cropped sweep: every copy a slot of ONE
              LibraryScreen(crop_parents=True), cropped around its whole hit
  uncropped   the same calls on a sweep of this tree without crop_radius (the whole receptor in every slot: another
              complex, first-layer reuse and struck slots)
  per hit     `attribution.atom_masking` / `bond_masking` once per hit on the hit's CROPPED complex, edge lists made
              before the clock starts. atom_masking also leaves out every kept receptor atom and bond_masking scores a
              contact once per direction: the rates count the graphs each side actually ran.
  step        the captured step of a `crop_parents=True` screen against a `crop_parents=False` cropped screen on the
              same whole-ligand batch: the price of the second table. The extra packer launch of a leave-out batch is
              timed beside it (PF.leave_out_parent_pack alone).

The contact legs run on the first `--contact-hits` hits (at an edge radius of 10 A a hit has thousands of contacts).
One untimed run of each, then 3 timed runs, alternating; a run is timed by the host clock from the call to a device
synchronise after it. No rate is asserted.

    python tools/time_cropped_masking.py [--hits 256] [--contact-hits 256] [--batch 32] [--crop 10]
                                         [--out profiles/cropped_masking_time.txt]
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


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def alternate(calls, dev, runs=3):
    """{key: [seconds] * runs} and the last results: one untimed run of each call, then `runs` rounds."""
    times, results = {k: [] for k in calls}, {}
    for call in calls.values():
        timed(call, dev)
    for _ in range(runs):
        for key, call in calls.items():
            t, results[key] = timed(call, dev)
            times[key].append(t)
    return times, results


def report(lines, label, graphs, seconds):
    runs = ' '.join(f'{t:.3f}' for t in seconds)
    rate = graphs / statistics.median(seconds)
    lines.append(f'{label:34s} {rate:10.0f} graphs/s ({graphs} graphs; median of 3; runs {runs} s)')
    return rate


def measure(args, dev):
    from pointvs_amd import attribution
    from pointvs_amd import functional as PF
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.radius_graph import generate_edges
    from pointvs_amd.screening import LibraryScreen, ScreeningSweep
    from pointvs_amd.synthetic import CONFIGS, random_poses, screening_set
    cfg = CONFIGS['cfg2']
    lig30, rec, feats = screening_set()                # the cfg5 receptor
    rec_feats, rec = feats[lig30.shape[0]:].to(dev), rec.to(dev)
    lig, _, feats64 = screening_set(seed=5064, n_lig=64)
    torch.manual_seed(0)
    model = SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **cfg['model']).eval().to(dev)
    radius, crop = cfg['graph']['edge_radius'], args.crop
    sizes = torch.randint(8, 65, (args.hits,), generator=torch.Generator().manual_seed(20260405)).tolist()
    hits = [(f'lig{k}', feats64[:n].roll(k, 0).contiguous().to(dev),
             random_poses(lig[:n], 1, seed=100 + k, max_shift=6.0, device=dev)[0].contiguous())
            for k, n in enumerate(sizes)]
    few = hits[:args.contact_hits]
    cropped = ScreeningSweep(model, rec, rec_feats, radius, args.batch, crop_radius=crop, cropped_attribution=True)
    whole = ScreeningSweep(model, rec, rec_feats, radius, args.batch)
    complexes = []           # every hit's cropped complex with its edge lists, made before the clock starts
    for name, lig_feats, pose in hits:
        kept = (torch.cdist(pose.double(), rec.double()) < crop).any(0).nonzero().reshape(-1)
        pos, x = torch.cat([pose, rec[kept]], 0), torch.cat([lig_feats, rec_feats[kept]], 0)
        _, edge_index, edge_type = generate_edges(pos, x[:, -1].contiguous(), radius, radius, prune=False)
        complexes.append((name, int(pose.shape[0]), int(kept.numel()), pos[None], x[None], edge_index,
                          torch.nn.functional.one_hot(edge_type.long(), 3), int((edge_type == 1).sum())))
    kept_mean = statistics.mean(c[2] for c in complexes)
    lines = [f'## {len(hits)} hits of 8..64 atoms ({sum(sizes)} ligand atoms), batch {args.batch}, crop_radius {crop:g}, '
             f'edge radius {radius:g}; a hit keeps {kept_mean:.0f} of {rec.shape[0]} receptor atoms on average', '',
             '### ligand_atom_masking']
    calls = {
        'cropped': lambda: cropped.ligand_atom_masking(hits, sigmoid=False),
        'uncropped': lambda: whole.ligand_atom_masking(hits, sigmoid=False),
        'per hit': lambda: [attribution.atom_masking(model, pos, x, bs=args.batch, edge_indices=ei, edge_attrs=ea)
                            for _, _, _, pos, x, ei, ea, _ in complexes]}
    times, results = alternate(calls, dev)
    n_copies = sum(sizes) + len(hits)
    rates = {'cropped': report(lines, 'cropped sweep', n_copies, times['cropped']),
             'uncropped': report(lines, 'uncropped sweep (whole receptor)', n_copies, times['uncropped']),
             'per hit': report(lines, 'attribution.atom_masking per hit', sum(c[1] + c[2] + 1 for c in complexes),
                               times['per hit'])}
    lines.append(f"cropped / uncropped = {rates['cropped'] / rates['uncropped']:.2f}, cropped / per hit = "
                 f"{rates['cropped'] / rates['per hit']:.2f} (per hit also leaves out every kept receptor atom)")
    diff = max(float((results['cropped'][c[0]].double().cpu() - torch.from_numpy(ref[:c[1]])).abs().max())
               for c, ref in zip(complexes, results['per hit']))
    lines.append(f'max |score difference| cropped sweep against per hit = {diff:.2e}')

    lines += ['', f'### contact_masking (the first {len(few)} hits)']
    calls = {
        'cropped': lambda: cropped.contact_masking(few, sigmoid=False),
        'uncropped': lambda: whole.contact_masking(few, sigmoid=False),
        'per hit': lambda: [attribution.bond_masking(model, pos, x, bs=args.batch, edge_indices=ei, edge_attrs=ea)
                            for _, _, _, pos, x, ei, ea, _ in complexes[:len(few)]]}
    times, results = alternate(calls, dev)
    n_pairs = sum(int(p.shape[0]) for p, _ in results['cropped'].values())
    rates = {'cropped': report(lines, 'cropped sweep', n_pairs + len(few), times['cropped']),
             'uncropped': report(lines, 'uncropped sweep (struck slots)', n_pairs + len(few), times['uncropped']),
             'per hit': report(lines, 'attribution.bond_masking per hit', sum(c[7] + 1 for c in complexes[:len(few)]),
                               times['per hit'])}
    lines.append(f"cropped / uncropped = {rates['cropped'] / rates['uncropped']:.2f}, cropped / per hit = "
                 f"{rates['cropped'] / rates['per hit']:.2f} (per hit runs every contact once per direction)")

    # the captured step: the same whole-ligand batch through a cropped screen with and without the second table
    lines += ['', '### captured step on one batch of whole ligands']
    big = sorted(hits, key=lambda h: -h[2].shape[0])[:args.batch]
    slots = [(f, p) for _, f, p in big]
    screens = {flag: LibraryScreen(model, rec, rec_feats, args.batch, 64, radius, crop_radius=crop, crop_parents=flag)
               for flag in (False, True)}
    for screen in screens.values():
        screen.capture(slots)
    step_times = {flag: [] for flag in screens}
    for _ in range(3):
        for flag, screen in screens.items():
            t, _ = timed(lambda s=screen: [s.replay() for _ in range(50)], dev)
            step_times[flag].append(t / 50)
    med = {flag: statistics.median(v) * 1e3 for flag, v in step_times.items()}
    for flag in screens:
        runs = ' '.join(f'{t * 1e3:.3f}' for t in step_times[flag])
        lines.append(f'crop_parents={flag!s:5s} {med[flag]:8.3f} ms (median of 3 x 50 replays; {runs})')
    lines.append(f'crop_parents=True / False = {med[True] / med[False]:.3f}')
    pos = torch.cat([p for _, _, p in hits], 0)
    lig_ptr = torch.tensor([0] + sizes).cumsum(0).to(device=dev, dtype=torch.int32)
    first = torch.zeros(1, dtype=torch.int32, device=dev)
    out = PF.leave_out_parent_pack(pos, lig_ptr, lig_ptr, first, args.batch, 64)
    pack = [timed(lambda: [PF.leave_out_parent_pack(pos, lig_ptr, lig_ptr, first, args.batch, 64, out=out)
                           for _ in range(200)], dev)[0] / 200 for _ in range(3)]
    lines.append(f'PF.leave_out_parent_pack alone {statistics.median(pack) * 1e6:8.1f} us a call, host clock over 200 '
                 'back-to-back calls (the extra launch of a leave-out batch, outside the captured step)')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'cropped_masking_time.txt'))
    ap.add_argument('--hits', type=int, default=256)
    ap.add_argument('--contact-hits', type=int, default=256)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--crop', type=float, default=10.0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_cropped_masking.py measures on the GPU; none found')
    dev = torch.device('cuda:0')
    text = [f'# tools/time_cropped_masking.py: receptor 1970 atoms, 3-layer EGNN ch=32, {torch.cuda.get_device_name(0)}', '']
    text += measure(args, dev) + ['']
    text = '\n'.join(text)
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
