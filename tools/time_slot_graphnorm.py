#!/usr/bin/env python
"""What GraphNorm per node segment (`slot_graphnorm=True`, `per_graph_norm=True`, PVS_GRAPHNORM_SEGMENTS) costs and buys.
Every figure is the median of three runs, with the runs and their spread beside it.

  step      the captured step of the GraphNorm screen shape of tools/time_graphnorm_screen.py (cfg5 receptor, the cfg2
            model with graphnorm=True, 512 ligands of 8..64 atoms, batch 128: its first batch) with slot_graphnorm=True
            against padded_graphnorm=True on this tree, and - with --parent DIR, a built checkout of the parent commit -
            against padded_graphnorm=True of that package in a process of its own (the default path must not have slowed)
  contacts  ScreeningSweep.contact_masking of three hits on a GraphNorm model at batch 32 with slot_graphnorm=True against
            the batch_size=1 sweep that gives the same scores without the keyword
  atoms     attribution.atom_masking(per_graph_norm=True) against the default (one copy per forward) on the 500-atom
            shape of tools/time_attribution.py (real4A) with a GraphNorm model
  operator  pvs_graphnorm_stats_segments over the slots of the step's batch against pvs_graphnorm_stats_rows over the same
            rows as one range

    python tools/time_slot_graphnorm.py [--parent DIR] [--out profiles/slot_graphnorm_time.txt]
"""
import argparse
import json
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
RUNS = 3


def _summary(samples, unit, digits=3):
    med = statistics.median(samples)
    runs = ' '.join(f'{t:.{digits}f}' for t in samples)
    return med, f'{med:.{digits}f} {unit} (median of {len(samples)}: {runs}; spread {100 * (max(samples) - min(samples)) / med:.1f} %)'


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _events(fn, calls):
    """Milliseconds per call of fn, device events around `calls` calls; one warm-up round, then RUNS rounds."""
    import torch
    samples = []
    for _ in range(RUNS + 1):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        end.record()
        torch.cuda.synchronize()
        samples.append(start.elapsed_time(end) / calls)
    return samples[1:]


def _screen_shape(batch, n_ligands=512):
    """(GraphNorm model, receptor, receptor features, radius, the first batch's slots) of time_graphnorm_screen.py."""
    import torch
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.screening import plan_library
    from pointvs_amd.synthetic import CONFIGS, random_poses, screening_set
    dev = torch.device('cuda:0')
    cfg = CONFIGS['cfg2']
    lig30, rec, feats = screening_set()
    rec_feats = feats[lig30.shape[0]:].to(dev)
    lig, _, feats64 = screening_set(seed=5064, n_lig=64)
    lig_feats = feats64[:64]
    torch.manual_seed(0)
    model = SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **dict(cfg['model'], graphnorm=True)).eval()
    sizes = torch.randint(8, 65, (n_ligands,), generator=torch.Generator().manual_seed(20260405)).tolist()
    first = plan_library([9] * len(sizes), sizes, batch, 64)[0]
    slots = [(lig_feats[:sizes[k]].roll(k, 0).contiguous(),
              random_poses(lig[:sizes[k]], 9, seed=100 + k, max_shift=6.0, device=dev)[pose]) for k, pose in first]
    return model, rec.to(dev), rec_feats, cfg['graph']['edge_radius'], slots, lig, lig_feats


def step_times(batch, legs):
    """{leg: ms per replay, RUNS rounds of 50} of the captured step on the first batch; legs: {label: keywords}."""
    from pointvs_amd.screening import LibraryScreen
    model, rec, rec_feats, radius, slots, _, _ = _screen_shape(batch)
    out = {}
    for label, kw in legs.items():
        screen = LibraryScreen(model, rec, rec_feats, batch, 64, radius, **kw).capture(slots)
        out[label] = _events(screen.replay, 50)
    return out


def contact_times(lines):
    from pointvs_amd.screening import ScreeningSweep
    from pointvs_amd.synthetic import random_poses
    model, rec, rec_feats, radius, _, lig, lig_feats = _screen_shape(32, 32)
    hits = [(f'hit{n}', lig_feats[:n].roll(k, 0).contiguous(), random_poses(lig[:n], 1, seed=700 + k, max_shift=3.0)[0].contiguous())
            for k, n in enumerate((12, 30, 48))]
    sweeps = {'slot_graphnorm, batch 32': ScreeningSweep(model, rec, rec_feats, radius, 32, slot_graphnorm=True),
              'batch_size=1': ScreeningSweep(model, rec, rec_feats, radius, 1)}
    calls = {leg: (lambda s=s: s.contact_masking(hits, sigmoid=False, column=0)) for leg, s in sweeps.items()}
    got = {leg: _timed(call)[1] for leg, call in calls.items()}          # untimed: probes, buffers, the capture
    times = {leg: [] for leg in calls}
    for _ in range(RUNS):
        for leg, call in calls.items():
            times[leg].append(_timed(call)[0])
    copies = sum(int(got['batch_size=1'][n][0].shape[0]) + 1 for n, _, _ in hits)
    diff = max(float((got['slot_graphnorm, batch 32'][n][1] - got['batch_size=1'][n][1]).abs().max()) for n, _, _ in hits)
    top = max(float(got['batch_size=1'][n][1].abs().max()) for n, _, _ in hits)
    lines.append(f'contacts: contact_masking of 3 hits (12, 30, 48 atoms; {copies} copies), GraphNorm model, receptor '
                 f'{rec.shape[0]} atoms')
    meds = {}
    for leg in calls:
        meds[leg], text = _summary(times[leg], 's')
        lines.append(f'  {leg:26s} {text}')
    lines.append(f'  ratio batch_size=1 / slot_graphnorm = {meds["batch_size=1"] / meds["slot_graphnorm, batch 32"]:.2f}; '
                 f'max |score difference| = {diff:.2e} (largest |score| {top:.2e})')


def atom_times(lines):
    import torch
    from pointvs_amd import attribution
    from pointvs_amd import graph as pgraph
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.synthetic import CONFIGS, synthetic_graph
    cfg = CONFIGS['real4A']
    pgraph.CACHE_ENABLED = False
    g = synthetic_graph(1000 * cfg['cfg_id'], **cfg['graph']).to('cuda')
    torch.manual_seed(0)
    model = SartorrasEGNN(Path(tempfile.mkdtemp()), 2e-3, 1e-4, silent=True,
                          **dict(cfg['model'], graphnorm=True)).to('cuda').eval()
    p, v = g.pos[None], g.x[None]
    calls = {leg: (lambda kw=kw: attribution.atom_masking(model, p, v, bs=32, edge_indices=g.edge_index,
                                                         edge_attrs=g.edge_attr, **kw))
             for leg, kw in (('per_graph_norm=True', dict(per_graph_norm=True)), ('default', {}))}
    got = {leg: _timed(call)[1] for leg, call in calls.items()}
    times = {leg: [] for leg in calls}
    for _ in range(RUNS):
        for leg, call in calls.items():
            times[leg].append(_timed(call)[0])
    import numpy as np
    lines.append(f'atoms: attribution.atom_masking, real4A ({p.shape[1]} atoms, {g.edge_index.shape[1]} edges, '
                 f'{cfg["model"]["num_layers"]} layers) with GraphNorm, bs = 32')
    meds = {}
    for leg in calls:
        meds[leg], text = _summary(times[leg], 's')
        lines.append(f'  {leg:26s} {text}')
    lines.append(f'  ratio default / per_graph_norm = {meds["default"] / meds["per_graph_norm=True"]:.2f}; max |score '
                 f'difference| = {float(np.abs(got["default"] - got["per_graph_norm=True"]).max()):.2e} (largest |score| '
                 f'{float(np.abs(got["default"]).max()):.2e})')


def operator_times(lines, batch):
    import torch
    from pointvs_amd import functional as PF
    from pointvs_amd.screening import LibraryScreen
    model, rec, rec_feats, radius, slots, _, _ = _screen_shape(batch)
    screen = LibraryScreen(model, rec, rec_feats, batch, 64, radius, slot_graphnorm=True)
    screen(slots)
    node_ptr = screen._fast['node_ptr'].clone()
    hidden = model.layers[1].hidden_nf
    y = torch.randn(screen.n_cap, hidden, device='cuda')
    ms = torch.rand(hidden, device='cuda') + 0.5
    count = node_ptr[batch:].clone()
    out_s = torch.empty((batch, 2 * hidden), device='cuda')
    out_r = torch.empty(2 * hidden, device='cuda')
    legs = {'pvs_graphnorm_stats_segments': lambda: PF.graphnorm_stats_segments(y, ms, node_ptr, out=out_s),
            'pvs_graphnorm_stats_rows': lambda: PF.graphnorm_stats(y, ms, n_rows=count, out=out_r)}
    lines.append(f'operator: y [{screen.n_cap}, {hidden}], {batch} segments over {int(count)} rows (device events around 200 '
                 'calls, the Python wrapper included)')
    for leg, fn in legs.items():
        lines.append(f'  {leg:30s} {_summary(_events(fn, 200), "ms")[1]}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'slot_graphnorm_time.txt'))
    ap.add_argument('--parent', default=None, help='a built checkout of the parent commit (its step in a process of its own)')
    ap.add_argument('--root', default=str(ROOT), help='where pointvs_amd is imported from')
    ap.add_argument('--only-padded-step', action='store_true', help='print the padded_graphnorm step of --root as JSON')
    ap.add_argument('--batch', type=int, default=128)
    args = ap.parse_args()
    sys.path.insert(0, args.root)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('time_slot_graphnorm.py measures on the GPU; none found')
    if args.only_padded_step:
        print('JSON ' + json.dumps(step_times(args.batch, {'padded': dict(padded_graphnorm=True)})['padded']))
        return
    lines = [f'# tools/time_slot_graphnorm.py on {torch.cuda.get_device_name(0)}; every figure: median of {RUNS} runs']
    steps = step_times(args.batch, {'slot_graphnorm=True': dict(slot_graphnorm=True),
                                    'padded_graphnorm=True': dict(padded_graphnorm=True)})
    lines.append(f'step: the captured step, cfg5 receptor, cfg2 model with GraphNorm, batch {args.batch} of ligands of 8..64 '
                 'atoms (ms per replay, rounds of 50)')
    meds = {}
    for leg, samples in steps.items():
        meds[leg], text = _summary(samples, 'ms')
        lines.append(f'  {leg:34s} {text}')
    if args.parent:
        run = subprocess.run([sys.executable, str(Path(__file__).resolve()), '--root', args.parent, '--only-padded-step',
                              '--batch', str(args.batch)], capture_output=True, text=True)
        found = [line for line in run.stdout.splitlines() if line.startswith('JSON ')]
        if run.returncode == 0 and found:
            meds['parent'], text = _summary(json.loads(found[-1][5:]), 'ms')
            lines.append(f'  {"parent commit, padded_graphnorm":34s} {text}')
            lines.append(f'  padded_graphnorm: this tree / parent = {meds["padded_graphnorm=True"] / meds["parent"]:.3f}')
        else:
            lines.append(f'  parent commit: not measured (the run in {args.parent} failed: {run.stderr[-300:]!r})')
    else:
        lines.append('  parent commit: not measured (no --parent checkout given)')
    lines.append(f'  slot_graphnorm / padded_graphnorm = {meds["slot_graphnorm=True"] / meds["padded_graphnorm=True"]:.3f}')
    contact_times(lines)
    atom_times(lines)
    operator_times(lines, args.batch)
    text = '\n'.join(lines) + '\n'
    print(text)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(text)


if __name__ == '__main__':
    main()
