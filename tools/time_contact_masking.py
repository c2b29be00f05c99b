#!/usr/bin/env python
"""(GPU) Contact masking of the hits of a screen, two ways, and what struck slots cost (cfg5 receptor, cfg2 layer
stack, `--hits` ligands of 8..64 atoms, one pose each - the best poses a sweep ends with):

  screen      `ScreeningSweep.contact_masking(hits)`: the contacts listed on the device, then every leave-one-pair-out
              copy of every hit as a struck slot of ONE LibraryScreen (receptor-receptor sums and template reused, one
              packer launch + one captured step per batch)
  per hit     `attribution.bond_masking(model, pos, x, edge_indices, edge_attrs, bs)` once per hit (the complex's graph
              prepared per call, a leave-out batch built from the whole CSR per chunk; it scores every contact once per
              direction, so it runs twice the graphs - the rate below counts each unordered pair once on both sides).
              The hits' edge lists are made before the clock starts.
  step        the captured struck step on a full batch of pair copies against the captured `ligand_atom_masking` step on
              a full batch of ligand-atom copies of the same hits: the cost of the touched rows.

One untimed run of each, then 3 timed runs, alternating; a run is timed by the host clock from the call to a device
synchronise after it. Reports the median leave-out graphs/s of both, their ratio, the largest difference between
their scores, and the two steps' medians.

    python tools/time_contact_masking.py [--hits 64] [--batch 32] [--out profiles/contact_masking_time.txt]
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
    sweep = ScreeningSweep(model, rec, rec_feats, radius, args.batch)
    complexes = []
    for name, lig_feats, pose in hits:
        pos, x = torch.cat([pose, rec], 0), torch.cat([lig_feats, rec_feats], 0)
        _, edge_index, edge_type = generate_edges(pos, x[:, -1], radius, radius, prune=False)
        complexes.append((name, int(pose.shape[0]), pos[None], x[None], edge_index, edge_type,
                          torch.nn.functional.one_hot(edge_type.long(), 3)))

    def screen():
        return {name: (pairs.clone(), scores.clone())
                for name, (pairs, scores) in sweep.contact_masking(hits, sigmoid=False).items()}

    def per_hit():
        return {name: attribution.bond_masking(model, pos, x, bs=args.batch, edge_indices=edge_index, edge_attrs=edge_attr)
                for name, _, pos, x, edge_index, _, edge_attr in complexes}

    calls = {'screen': screen, 'per hit': per_hit}
    times, results = {k: [] for k in calls}, {}
    for call in calls.values():
        timed(call, dev)
    for _ in range(3):
        for key, call in calls.items():
            t, results[key] = timed(call, dev)
            times[key].append(t)
    n_pairs = sum(int(pairs.shape[0]) for pairs, _ in results['screen'].values())
    n_graphs = n_pairs + len(hits)
    diff = top = 0.0
    for name, n, _, _, edge_index, edge_type, _ in complexes:
        pairs, scores = results['screen'][name]
        ei, cls = edge_index.cpu(), edge_type.cpu()
        where = {(int(a), int(b)): e for e, (a, b) in enumerate(ei.t().tolist()) if int(cls[e]) == 1}
        ref = torch.tensor([results['per hit'][name][where[a, n + r]] for a, r in pairs.tolist()], dtype=torch.float64)
        if len(ref):
            diff = max(diff, float((scores.double().cpu() - ref).abs().max()))
            top = max(top, float(ref.abs().max()))
    rate = {k: n_graphs / statistics.median(v) for k, v in times.items()}
    lines = [f'## {len(hits)} hits of 8..64 atoms ({sum(sizes)} ligand atoms), {n_pairs} contacts, {n_graphs} graphs, '
             f'batch {args.batch}, {-(-n_graphs // args.batch)} steps a run']
    for key in calls:
        runs = ' '.join(f'{t:.3f}' for t in times[key])
        lines.append(f'{key:8s} {rate[key]:10.0f} graphs/s (median of 3; runs {runs} s)')
    lines.append(f"ratio screen / per hit = {rate['screen'] / rate['per hit']:.2f}")
    lines.append(f'max |score difference| between the two = {diff:.2e} (max |score| {top:.2e})')

    # the captured steps alone, each on the last full batch its sweep loaded
    sweep.ligand_atom_masking(hits, sigmoid=False)
    steps = {'struck step': sweep.struck, 'ligand-atom step': sweep.masking}
    step_times = {k: [] for k in steps}
    if all(s._captured for s in steps.values()):
        for _ in range(3):
            for key, s in steps.items():
                t, _ = timed(lambda s=s: [s.replay() for _ in range(50)], dev)
                step_times[key].append(t / 50)
        for key in steps:
            runs = ' '.join(f'{t * 1e3:.3f}' for t in step_times[key])
            lines.append(f'{key:16s} {statistics.median(step_times[key]) * 1e3:8.3f} ms (median of 3 x 50 replays; {runs})')
    else:
        lines.append('steps: not captured (the caching allocator is off): not timed')
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'contact_masking_time.txt'))
    ap.add_argument('--hits', type=int, default=64)
    ap.add_argument('--batch', type=int, default=32)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_contact_masking.py measures on the GPU; none found')
    dev = torch.device('cuda:0')
    text = [f'# tools/time_contact_masking.py: receptor 1970 atoms, radius 10 A, 3-layer EGNN ch=32, '
            f'{torch.cuda.get_device_name(0)}', '']
    text += measure(args, dev) + ['']
    text = '\n'.join(text)
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
