#!/usr/bin/env python
"""(GPU) Library screening with the receptor cropped around every pose against the uncropped sweep (cfg5 receptor,
cfg2 model: k = 32, 3 layers; 512 ligands of 8..64 atoms with 9 poses each = 4,608 poses, batch 128 - the `mixed`
library of tools/time_library_screen.py):

  crop_radius None | 10 | 6   `ScreeningSweep(..., crop_radius=R).run_library` of this tree
  crop_radius 1e6             the crop that drops nothing: what the cropped step costs where it cannot pay (every layer
                              over the whole graph, no first-layer reuse, and the masks on top)
  parent                      `--parent PARENT_TREE`: the uncropped sweep of a built checkout of the parent commit

Every tree runs in a child process of its own (this file with --tree), so that neither library shares a process with
the other. Per leg: one untimed run (probe, capture), then 3 timed runs, the legs of a tree alternating; a run is
timed by the host clock from the call to a device synchronise after it. Then the captured step alone: 200 replays of
the sweep's library step on the batch it holds, host clock around them. Reports per leg the median poses/s, the
captured step time and the mean number of receptor atoms a slot keeps (uncropped: all of them).

    python tools/time_cropped_screen.py [--parent PARENT_TREE] [--out profiles/cropped_screen_time.txt]
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


def timed(fn, dev):
    import torch
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.perf_counter() - t0, out


def child(args):
    """The legs `args.legs` on the package of `args.tree`; one JSON line."""
    sys.path.insert(0, str(Path(args.tree).resolve()))
    import torch
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.screening import ScreeningSweep
    from pointvs_amd.synthetic import CONFIGS, random_poses, screening_set
    dev = torch.device('cuda:0')
    cfg = CONFIGS['cfg2']
    lig30, rec, feats = screening_set()                # the cfg5 receptor
    rec_feats, rec = feats[lig30.shape[0]:].to(dev), rec.to(dev)
    lig, _, feats64 = screening_set(seed=5064, n_lig=64)
    torch.manual_seed(0)
    model = SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **cfg['model']).eval()
    gen = torch.Generator().manual_seed(20260405)
    sizes = torch.randint(8, 65, (args.ligands,), generator=gen).tolist()
    radius = cfg['graph']['edge_radius']
    work = [(f'lig{k}', feats64[:n].roll(k, 0).contiguous(), random_poses(lig[:n], 9, seed=100 + k, max_shift=6.0, device=dev))
            for k, n in enumerate(sizes)]
    n_poses = sum(int(p.shape[0]) for _, _, p in work)
    out_dir = Path(tempfile.mkdtemp())
    names = args.legs.split(',')
    legs = [None if leg == 'none' else float(leg) for leg in names]
    # (the uncropped leg passes no keyword: the parent's ScreeningSweep has none)
    sweeps = {leg: ScreeningSweep(model, rec, rec_feats, radius, args.batch,
                                  **({} if leg is None else dict(crop_radius=leg))) for leg in legs}
    calls = {leg: (lambda leg=leg: sweeps[leg].run_library(work, predictions_file=out_dir / f'{leg}.txt')) for leg in legs}
    times, batches = {leg: [] for leg in legs}, {}
    for call in calls.values():
        timed(call, dev)
    for _ in range(3):
        for leg, call in calls.items():
            before = sweeps[leg].batches_run
            t, _ = timed(call, dev)
            times[leg].append(t)
            batches[leg] = sweeps[leg].batches_run - before
    result = {}
    for name, leg in zip(names, legs):
        screen = sweeps[leg].library
        step, _ = timed(lambda: [screen.replay() if screen._captured else screen() for _ in range(200)], dev)
        screen.check()
        if leg is None:
            kept = float(rec.shape[0])
        else:      # every pose's kept count (fp64 distances on the device: a figure for the record, not a decision)
            counts = [(torch.cdist(p.double(), rec.double()) < leg).any(1).sum(1) for _, _, p in work]
            kept = float(torch.cat(counts).double().mean())
        result[name] = dict(
            times=times[leg], poses_per_s=n_poses / statistics.median(times[leg]), batches=batches[leg],
            step_ms=step / 200 * 1e3, captured=bool(screen._captured), kept=kept, n_cap=int(screen.n_cap),
            edge_room=int(screen._fast['cap']))
    print(json.dumps(dict(n_poses=n_poses, n_rec=int(rec.shape[0]), radius=radius, device=torch.cuda.get_device_name(0),
                          legs=result)))


def run_child(tree, legs, args):
    out = subprocess.run([sys.executable, str(Path(__file__).resolve()), '--tree', str(tree), '--legs', legs,
                          '--ligands', str(args.ligands), '--batch', str(args.batch)],
                         capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise SystemExit(f'the legs {legs} of {tree} failed ({out.returncode}):\n{out.stderr[-3000:]}')
    return json.loads(out.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'cropped_screen_time.txt'))
    ap.add_argument('--ligands', type=int, default=512)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--parent', metavar='PARENT_TREE', help='a built checkout of the parent commit')
    ap.add_argument('--tree', help='(child) the tree whose package runs the legs')
    ap.add_argument('--legs', default='none,10,6,1e6', help='(child) crop radii, `none` for the uncropped sweep')
    args = ap.parse_args()
    if args.tree:
        return child(args)
    rows = []
    if args.parent:
        rows.append(('parent, uncropped', run_child(args.parent, 'none', args), 'none'))
    this = run_child(ROOT, 'none,10,6,1e6', args)
    rows += [(f'crop_radius {key.capitalize()}', this, key) for key in ('none', '10', '6', '1e6')]
    text = [f'# tools/time_cropped_screen.py: receptor {this["n_rec"]} atoms, edge radius {this["radius"]} A, 3-layer EGNN '
            f'ch=32, {this["device"]}',
            f'# {args.ligands} ligands of 8..64 atoms, {this["n_poses"]} poses, batch {args.batch}; run_library, median of 3',
            '', f'{"leg":18s} {"poses/s":>9s} {"runs (s)":>20s} {"batches":>8s} {"step (ms)":>10s} {"kept atoms/slot":>16s} '
            f'{"rows (N_cap)":>13s} {"edge room":>10s}']
    for label, res, key in rows:
        leg = res['legs'][key]
        runs = ' '.join(f'{t:.3f}' for t in leg['times'])
        text.append(f'{label:18s} {leg["poses_per_s"]:9.0f} {runs:>20s} {leg["batches"]:8d} {leg["step_ms"]:10.3f} '
                    f'{leg["kept"]:16.1f} {leg["n_cap"]:13d} {leg["edge_room"]:10d}')
    base = this['legs']['none']
    text.append('')
    for key in ('10', '6', '1e6'):
        leg = this['legs'][key]
        text.append(f'crop_radius {key} / None: poses/s x {leg["poses_per_s"] / base["poses_per_s"]:.2f}, '
                    f'step time x {leg["step_ms"] / base["step_ms"]:.2f}')
    if args.parent:
        parent = rows[0][1]['legs']['none']
        text.append(f'crop_radius None / parent: poses/s x {base["poses_per_s"] / parent["poses_per_s"]:.3f}, '
                    f'step time x {base["step_ms"] / parent["step_ms"]:.3f}')
    text = '\n'.join(text) + '\n'
    print(text)
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
