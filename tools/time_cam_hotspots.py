#!/usr/bin/env python
"""(GPU) Class-activation map of the hits of a screen (cfg5 receptor, cfg2 layer stack, `--hits` ligands of 8..64 atoms,
one pose each: the library of tools/time_receptor_hotspots.py), three measurements:

  (a) hits per second, two ways:
        sweep     `ScreeningSweep.receptor_hotspots(hits, attribution='cam')`: the whole ligands as slots of ONE
                  LibraryScreen, the heads applied per node and gathered per slot inside the captured step
                  (PF.node_heads, PF.slot_node_values), one copy to the host at the end
        per hit   `attribution.cam(model, pos, x, edge_index, edge_attr)` once per hit (a graph preparation, one
                  forward and one [n] copy to the host each), then on the host the mean over the hits per receptor
                  atom. The hits' edge lists are made before the clock starts.
      One untimed run of each (screen built, step captured), then 3 timed runs, alternating; a run is timed by the host
      clock from the call to a device synchronise after it. Also the largest difference between the two maps.
  (b) the captured step with the map against the same step without it (the step as it was before the option existed):
      two LibraryScreens on the same full batch, one built with cam=True, both captured; `--rounds` rounds of
      `--replays` replays each, alternating, timed with device events; median and minimum per replay.
  (c) pvs_node_heads_fwd alone on [rows, width] rows at widths 32 and 64, one output column and four: rows = 128 slots
      of 2,000 (one cfg5 batch); the launches rotate over enough separate inputs (> 512 MB in all) that no row comes from
      a cache; device events around `--replays` launches, median of `--rounds`; bytes = 4 rows (width + C), against the
      HBM rate of the data sheet (8.0 TB/s) and the rate a float4 copy reaches (6.29 TB/s).

    python tools/time_cam_hotspots.py [--hits 256] [--batch 32] [--out profiles/cam_hotspots_time.txt]
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

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def timed(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def event_ms(fn, replays):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for k in range(replays):
        fn(k)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) / replays


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
    n_rec = int(rec.shape[0])
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
    for _, lig_feats, pose in hits:
        pos, x = torch.cat([pose, rec], 0), torch.cat([lig_feats, rec_feats], 0)
        _, edge_index, edge_type = generate_edges(pos, x[:, -1], radius, radius, prune=False)
        complexes.append((pos[None], x[None], edge_index, torch.nn.functional.one_hot(edge_type.long(), 3),
                          int(pose.shape[0])))

    def through_sweep():
        return sweep.receptor_hotspots(hits, attribution='cam')['mean'].cpu().numpy()

    def per_hit():
        total = np.zeros(n_rec)
        for pos, x, edge_index, edge_attr, n in complexes:
            total += attribution.cam(model, pos, x, edge_indices=edge_index, edge_attrs=edge_attr).reshape(-1)[n:]
        return total / len(complexes)

    calls = {'sweep': through_sweep, 'per hit': per_hit}
    times, results = {k: [] for k in calls}, {}
    for call in calls.values():
        timed(call, dev)
    for _ in range(3):
        for key, call in calls.items():
            t, results[key] = timed(call, dev)
            times[key].append(t)
    diff = float(np.abs(results['sweep'] - results['per hit']).max())
    rate = {k: len(hits) / statistics.median(v) for k, v in times.items()}
    lines = [f'## (a) {len(hits)} hits of 8..64 atoms ({sum(sizes)} ligand atoms), batch {args.batch}, '
             f'{-(-len(hits) // args.batch)} steps a run']
    for key in calls:
        runs = ' '.join(f'{t:.3f}' for t in times[key])
        lines.append(f'{key:8s} {rate[key]:10.0f} hits/s (median of 3; runs {runs} s)')
    lines.append(f"ratio sweep / per hit = {rate['sweep'] / rate['per hit']:.2f}")
    lines.append(f'max |difference| between the two maps = {diff:.2e} (largest |value| {float(np.abs(results["sweep"]).max()):.3f})')

    # (b) one full batch, the captured step with and without the map
    slots = [(f, p) for _, f, p in hits[:args.batch]]
    screens = {'with': LibraryScreen(model, rec, rec_feats, args.batch, 64, radius, cam=True),
               'without': LibraryScreen(model, rec, rec_feats, args.batch, 64, radius)}
    for screen in screens.values():
        screen.capture(slots)
        screen.replay()
    per_replay = {k: [] for k in screens}
    for _ in range(args.rounds):
        for key, screen in screens.items():
            per_replay[key].append(event_ms(lambda k: screen.replay(), args.replays))
    for screen in screens.values():
        screen.check()
    lines += ['', f'## (b) the captured step of one batch of {args.batch} ligands ({screens["with"].n_cap} rows), '
                  f'{args.rounds} rounds of {args.replays} replays, alternating; ms per replay']
    for key, v in per_replay.items():
        lines.append(f'{key + " the map":22s} median {statistics.median(v):.4f}  min {min(v):.4f}')
    med = {k: statistics.median(v) for k, v in per_replay.items()}
    lines.append(f"the map costs {1e3 * (med['with'] - med['without']):.1f} us a step "
                 f"({100 * (med['with'] / med['without'] - 1):+.2f} %)")

    # (c) the per-node heads alone, every launch on rows that no cache holds
    rows = 128 * 2000
    lines += ['', f'## (c) pvs_node_heads_fwd on [{rows}, width] rows, inputs rotated (> 512 MB in all), median of '
                  f'{args.rounds} rounds of {args.replays} launches']
    gen = torch.Generator(device=dev).manual_seed(1)
    for width in (32, 64):
        n_inputs = -(-(512 << 20) // (4 * rows * width)) + 1
        inputs = [torch.randn((rows, width), device=dev, generator=gen) for _ in range(n_inputs)]
        for n_cols in (1, 4):
            heads = [(torch.randn((n_cols, width), device=dev, generator=gen), torch.randn(n_cols, device=dev, generator=gen), None)]
            out = torch.empty((rows, n_cols), device=dev)
            event_ms(lambda k: PF.node_heads(inputs[k % n_inputs], heads, out=out), n_inputs)
            ms = statistics.median(event_ms(lambda k: PF.node_heads(inputs[k % n_inputs], heads, out=out), args.replays)
                                   for _ in range(args.rounds))
            nbytes = 4 * rows * (width + n_cols)
            rate_ = nbytes / (ms * 1e-3)
            lines.append(f'width {width:3d}, {n_cols} column(s): {1e3 * ms:7.1f} us, {nbytes / 1e6:6.1f} MB, {rate_ / 1e12:.2f} TB/s = '
                         f'{100 * rate_ / HBM_SPEC:.0f} % of 8.0 TB/s (data sheet), {100 * rate_ / HBM_COPY:.0f} % of 6.29 TB/s '
                         '(float4 copy)')
        del inputs
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'cam_hotspots_time.txt'))
    ap.add_argument('--hits', type=int, default=256)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--rounds', type=int, default=9)
    ap.add_argument('--replays', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_cam_hotspots.py measures on the GPU; none found')
    dev = torch.device('cuda:0')
    text = [f'# tools/time_cam_hotspots.py: receptor 1970 atoms, radius 10 A, 3-layer EGNN ch=32, '
            f'{torch.cuda.get_device_name(0)}', '']
    text += measure(args, dev) + ['']
    text = '\n'.join(text)
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
