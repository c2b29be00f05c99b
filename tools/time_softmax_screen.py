#!/usr/bin/env python
"""`run_library` on a softmax-attention model with and without `softmax_reuse` (cfg5 receptor; the cfg2 model - k = 32,
3 layers - with edge_attention and softmax_attention; 512 ligands of 8..64 atoms, fixed seed, 9 poses each; batch 128:
36 dense batches).

Alternating legs, one untimed run each (probes, buffers, the capture) and then 3 timed ones; a run is timed by the host
clock from the call to a device synchronise after it:

  softmax off   softmax_reuse left off: the plain eager route (the general graph builder, every receptor-receptor edge
                of the first layer recomputed per pose) - the launches of the commit before the keyword existed
  softmax on    softmax_reuse=True: one captured step for every batch, the first layer over the ligand-touching edges
                on top of the receptor's softmax statistics
  sigmoid off / sigmoid on
                the sigmoid-attention model of profiles/receptor_hotspots_time.txt with the keyword off and on: the
                same route and the same bits either way - the yardstick of the session

    python tools/time_softmax_screen.py [--out profiles/softmax_screen_time.txt] [--append]
"""
import argparse
import statistics
import sys
import tempfile
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from tools.time_graphnorm_screen import make_library, timed      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'softmax_screen_time.txt'))
    ap.add_argument('--append', action='store_true', help='add to --out instead of replacing it')
    ap.add_argument('--ligands', type=int, default=512)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--repeats', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('time_softmax_screen.py measures on the GPU; none found')
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.screening import ScreeningSweep
    from pointvs_amd.synthetic import CONFIGS, screening_set
    dev = torch.device('cuda:0')
    cfg = CONFIGS['cfg2']
    lig30, rec, feats = screening_set()                # the cfg5 receptor
    rec_feats = feats[lig30.shape[0]:].to(dev)
    lig, _, feats64 = screening_set(seed=5064, n_lig=64)
    lig_feats = feats64[:64]
    rec = rec.to(dev)
    radius = cfg['graph']['edge_radius']

    def model(**flags):
        torch.manual_seed(0)
        return SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **dict(cfg['model'], **flags)).eval().to(dev)

    gen = torch.Generator().manual_seed(20260405)
    sizes = torch.randint(8, 65, (args.ligands,), generator=gen).tolist()
    work = make_library(lig, lig_feats, sizes, 9, dev, seed=100)
    n_poses = sum(int(p.shape[0]) for _, _, p in work)
    soft, sigmoid = model(edge_attention=True, softmax_attention=True), model(edge_attention=True)
    sweeps = {f'{name} {leg}': ScreeningSweep(m, rec, rec_feats, radius, args.batch, softmax_reuse=leg == 'on')
              for name, m in (('softmax', soft), ('sigmoid', sigmoid)) for leg in ('off', 'on')}
    calls = {leg: (lambda s=s: s.run_library(work, sigmoid=False)) for leg, s in sweeps.items()}
    times, scores, batches = {leg: [] for leg in sweeps}, {}, {}
    for leg, call in calls.items():                    # untimed: the probe, the buffers, the capture
        timed(call, dev)
    for _ in range(args.repeats):
        for leg, call in calls.items():                # alternating
            before = sweeps[leg].batches_run
            t, scores[leg] = timed(call, dev)
            times[leg].append(t)
            batches[leg] = sweeps[leg].batches_run - before
    text = [f'# tools/time_softmax_screen.py: receptor {rec.shape[0]} atoms, radius {radius} A, 3-layer EGNN ch=32 with edge '
            f'attention, {len(work)} ligands of 8..64 atoms, {n_poses} poses, batch {args.batch}, '
            f'{torch.cuda.get_device_name(0)}']
    for leg in sweeps:
        runs = ' '.join(f'{t:.3f}' for t in times[leg])
        spread = (max(times[leg]) - min(times[leg])) / statistics.median(times[leg])
        lib = sweeps[leg].library
        text.append(f'{leg:12s} {n_poses / statistics.median(times[leg]):10.0f} poses/s (median of {args.repeats}; runs {runs} s; '
                    f'spread {100 * spread:.1f} % of the median)  {batches[leg]:4d} batches, reuse: {bool(lib.reuse)}, '
                    f'captured: {bool(lib._captured)}')
    for name in ('softmax', 'sigmoid'):
        off, on = scores[f'{name} off'], scores[f'{name} on']
        diff = max(float((off[n] - on[n]).abs().max()) for n, _, _ in work)
        top = max(float(off[n].abs().max()) for n, _, _ in work)
        ratio = statistics.median(times[f'{name} off']) / statistics.median(times[f'{name} on'])
        text.append(f'{name}: rate on / off = {ratio:.2f}; max |raw score difference| = {diff:.2e} (largest |score| {top:.2e})')
    text = '\n'.join(text) + '\n\n'
    print(text)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with open(out, 'a' if args.append else 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
