"""Atom-masking attribution of one complex: the batched path (pointvs_amd.attribution.atom_masking) against the loop a
user would write with the plain model API (per atom: masked COO list built with torch on the device, `model(graph)`,
one score back), at the reference's default shape (real4A: 500 atoms, 4 A, 6 layers) and at one cfg2-size graph
(2,000 atoms, 10 A, 3 layers).

    python tools/time_attribution.py [--repeats 3] [--bs 32] [--configs real4A,cfg2]

Each leg is warmed up once (code objects, allocator) and then timed `repeats` times with a host clock around a call that
ends with its scores on the host (so the device has finished); the legs alternate. Also timed: the share of the batched
call spent in the builder and in the layers' edge kernels (pvs_profile_read, in a run of its own), for judging the
follow-up of reusing first-layer messages between copies. Prints a table and a JSON summary."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def loop_masking(model, p, v, edge_indices, edge_attrs):
    """The reference's atom_masking loop (attribution_fns.py:405-431) on the plain model API."""
    from pointvs_amd.graph import Data
    n = p.shape[1]
    scores = np.zeros(n)
    with torch.no_grad():
        def score(x, pos, ei, ea):
            g = Data(x=x, pos=pos, edge_index=ei, edge_attr=ea, num_graphs=1,
                     batch=torch.zeros(x.shape[0], dtype=torch.long, device=x.device))
            return float(model(g))
        original = score(v[0], p[0], edge_indices, edge_attrs)
        for i in range(n):
            keep = torch.arange(n, device=p.device) != i
            mask = (edge_indices != i).all(0)
            ei = edge_indices[:, mask]
            scores[i] = original - score(v[0, keep], p[0, keep], ei - (ei > i).long(), edge_attrs[mask])
    return scores


def time_config(name, repeats, bs):
    from pointvs_amd import _lib, attribution
    from pointvs_amd import graph as pgraph
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.synthetic import CONFIGS, synthetic_graph
    cfg = CONFIGS[name]
    pgraph.CACHE_ENABLED = False
    g = synthetic_graph(1000 * cfg['cfg_id'], **cfg['graph']).to('cuda')
    torch.manual_seed(0)
    model = SartorrasEGNN(Path('/tmp/pvs_time_attr'), 2e-3, 1e-4, silent=True, **cfg['model']).to('cuda').eval()
    p, v = g.pos[None], g.x[None]
    legs = {'batched': lambda: attribution.atom_masking(model, p, v, bs=bs, edge_indices=g.edge_index,
                                                        edge_attrs=g.edge_attr),
            'loop': lambda: loop_masking(model, p, v, g.edge_index, g.edge_attr)}
    out = {k: fn() for k, fn in legs.items()}          # warm-up, and the two legs' scores
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, fn in legs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[k].append(time.perf_counter() - t0)
    lib = _lib.lib()
    lib.pvs_profile_enable(1)
    lib.pvs_profile_reset()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    legs['batched']()
    torch.cuda.synchronize()
    profiled = time.perf_counter() - t0
    share = {}
    for key in ('mask_graph', 'edge_fwd', 'graph_prepare'):
        ms, cnt = C.c_double(), C.c_int64()
        lib.pvs_profile_read(key.encode(), C.byref(ms), C.byref(cnt))
        share[key] = dict(ms=round(ms.value, 3), launches=cnt.value)
    lib.pvs_profile_enable(0)
    lib.pvs_profile_reset()
    n_layers = cfg['model']['num_layers']
    return dict(config=name, n_atoms=int(p.shape[1]), n_edges=int(g.edge_index.shape[1]), layers=n_layers,
                bs=attribution.chunk_size(bs, p.shape[1], p.shape[1], g.edge_index.shape[1]),
                batched_s=[round(t, 4) for t in times['batched']], loop_s=[round(t, 4) for t in times['loop']],
                batched_median_s=round(float(np.median(times['batched'])), 4),
                loop_median_s=round(float(np.median(times['loop'])), 4),
                speedup=round(float(np.median(times['loop']) / np.median(times['batched'])), 2),
                max_score_diff=float(np.abs(out['batched'] - out['loop']).max()),
                max_score=float(np.abs(out['loop']).max()), profiled_call_s=round(profiled, 4), kernels=share,
                first_layer_edge_ms=round(share['edge_fwd']['ms'] / n_layers, 3))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--bs', type=int, default=32)
    ap.add_argument('--configs', default='real4A,cfg2')
    args = ap.parse_args()
    rows = []
    for name in args.configs.split(','):
        r = time_config(name, args.repeats, args.bs)
        rows.append(r)
        print(f"{r['config']:7s} N={r['n_atoms']:5d} E={r['n_edges']:7d} L={r['layers']} bs={r['bs']:3d}  batched "
              f"{r['batched_median_s'] * 1e3:9.1f} ms {r['batched_s']}  loop {r['loop_median_s'] * 1e3:9.1f} ms "
              f"{r['loop_s']}  x{r['speedup']:.2f}  |scores diff| {r['max_score_diff']:.2e} of {r['max_score']:.2e}",
              flush=True)
        k = r['kernels']
        print(f"        in one batched call ({r['profiled_call_s'] * 1e3:.1f} ms with event brackets): builder "
              f"{k['mask_graph']['ms']} ms / {k['mask_graph']['launches']} launches, edge forward {k['edge_fwd']['ms']} ms"
              f" / {k['edge_fwd']['launches']} launches (one layer of {r['layers']}: ~{r['first_layer_edge_ms']} ms), "
              f"parent prepare {k['graph_prepare']['ms']} ms", flush=True)
    print(json.dumps({'device': torch.cuda.get_device_name(0), 'repeats': args.repeats, 'rows': rows}))


if __name__ == '__main__':
    main()
