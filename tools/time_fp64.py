"""fp64 training-step time (--double) at the cfg2 and real4A shapes, beside the fp32 step of the same model.

    python tools/time_fp64.py [--steps 20] [--warmup 5] [--batch 32]

One eager step = forward + BCE loss + backward + clip + Adam (torch's Adam for fp64: FusedClipAdam is fp32 only),
timed with device events over `steps` steps after `warmup`; the graphs are resident in HBM and prepared every step.
Prints one line per (config, dtype) and a JSON summary."""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def time_config(name, dtype, steps, warmup, batch_size):
    from pointvs_amd import graph as pgraph
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.synthetic import CONFIGS, synthetic_batch
    cfg = CONFIGS[name]
    pgraph.CACHE_ENABLED = False
    batch = synthetic_batch(cfg['cfg_id'], batch_size, **cfg['graph']).to('cuda')
    torch.manual_seed(0)
    model = SartorrasEGNN(Path('/tmp/pvs_time_fp64'), 2e-3, 1e-4, silent=True, **cfg['model']).to(dtype=dtype).train()
    y_true = batch.y.float()

    def step():
        y_pred, _, _, _ = model.unpack_input_data_and_predict(batch)
        return model.backprop(y_true, y_pred, sync=False)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        loss = step()
    t1.record()
    torch.cuda.synchronize()
    ms = t0.elapsed_time(t1) / steps
    return dict(config=name, dtype=str(dtype).replace('torch.', ''), step_ms=round(ms, 3),
                graphs_per_s=round(batch_size / ms * 1e3, 1), n_nodes=int(batch.x.shape[0]),
                n_edges=int(batch.edge_index.shape[1]), loss=float(loss))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--configs', default='cfg2,real4A')
    args = ap.parse_args()
    rows = []
    for name in args.configs.split(','):
        for dtype in (torch.float32, torch.float64):
            r = time_config(name, dtype, args.steps, args.warmup, args.batch)
            rows.append(r)
            print(f"{r['config']:7s} {r['dtype']:8s} step {r['step_ms']:9.3f} ms  {r['graphs_per_s']:9.1f} graphs/s  "
                  f"N={r['n_nodes']} E={r['n_edges']}", flush=True)
    for name in args.configs.split(','):
        f32, f64 = [r['step_ms'] for r in rows if r['config'] == name]
        print(f'{name}: fp64 / fp32 step time = {f64 / f32:.2f}x')
    print(json.dumps({'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'warmup': args.warmup,
                      'batch': args.batch, 'rows': rows}))


if __name__ == '__main__':
    main()
