#!/usr/bin/env python3
"""Golden vectors for masking attribution, from the real reference (build container only).

    python tests/golden/make_golden_attribution.py

Same pattern as make_golden.py: imports `/root/reference/point_vs` under the stand-ins in `_refstubs`, one thread,
fixed seeds, and drives the reference's own `attribution_fns.atom_masking` / `bond_masking` / `cam` /
`node_attention` / `edge_attention` on its own models. Writes `tests/golden/attr_*.npz`, data only: inputs,
`state_dict`, model kwargs, the unmasked output, EVERY masked graph's raw model output (`raw32`, recorded by a forward
hook on the model, in the order the reference visits the masks), the returned score array, and

    noise32 = the largest distance between the reference's fp32 masked outputs and its own `.double()` run, over the
              edge list as given and over PERMS fixed edge permutations (one thread).

noise32 is the noise term of the project's parity criterion (README "Parity"), stored here so that the GPU box does not
have to redraw it. Nothing on the GPU box runs this script or reads `/root/reference`.

What the reference can and cannot produce (checked here, on the CPU): a PNNGeometricBase model returns a 1-D output for
a single graph, so `bond_masking` raises for single-output models (`len()` of a 0-d array) and `atom_masking` raises for
three-output models (`float()` of three values: its mean-of-three branch needs a 2-D output). Atom-masking fixtures
therefore come from single-output models and bond-masking fixtures from three-output models.
"""
import importlib.util
import json
import os
import sys
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
spec = importlib.util.spec_from_file_location('make_golden', HERE / 'make_golden.py')
mg = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mg)          # sets sys.path, the NumPy aliases, the working directory and one thread

import numpy as np  # noqa: E402
import torch  # noqa: E402
from point_vs.attribution import attribution_fns as A  # noqa: E402
from point_vs.models.geometric.egnn_multitask import MultitaskSatorrasEGNN  # noqa: E402
from point_vs.models.geometric.egnn_satorras import SartorrasEGNN  # noqa: E402

torch.set_num_threads(1)
PERMS = 2
PERM_SEED = 20261016


def build(cls, kwargs, task, seed):
    torch.manual_seed(seed)
    np.random.seed(seed)
    with tempfile.TemporaryDirectory() as tmp:
        return cls(Path(tmp), 2e-3, 1e-4, None, None, silent=True, model_task=task, **kwargs).eval()


def recorded(fn, model, graph, dtype=torch.float32, perm=None, **kw):
    """fn's return value and the raw output of every forward it ran (the first one is the unmasked graph)."""
    outs = []
    handle = model.register_forward_hook(lambda mod, args, out: outs.append(out.detach().double().reshape(-1).numpy()))
    ei, ea = graph.edge_index, graph.edge_attr
    if perm is not None:
        ei, ea = ei[:, perm], ea[perm]
    default = torch.get_default_dtype()
    torch.set_default_dtype(dtype)      # atom_masking allocates its masked inputs with torch.zeros
    try:
        res = fn(model, graph.pos[None].to(dtype), graph.x[None].to(dtype), edge_indices=ei.clone(),
                 edge_attrs=ea.clone(), **kw)
    finally:
        torch.set_default_dtype(default)
        handle.remove()
    return np.asarray(res, dtype=np.float64), np.stack(outs)


def run_case(name, graph, cls, kwargs, fn_name, task='classification', seed=2, sigmoid=False, extras=False):
    fn = getattr(A, fn_name)
    A.SIGMOID = sigmoid
    model = build(cls, kwargs, task, seed)
    sd = {k: v.detach().clone().numpy() for k, v in model.state_dict().items()}
    n_edges = graph.edge_index.shape[1]
    scores, raw32 = recorded(fn, model, graph)
    # which mask each recorded forward belongs to: every atom, or the type-1 edges in list order
    if fn_name == 'atom_masking':
        visited = np.arange(graph.x.shape[0])
    else:
        visited = np.nonzero(graph.edge_attr[:, 1].numpy())[0]
    assert raw32.shape[0] == 1 + len(visited), (raw32.shape, len(visited))
    gen = torch.Generator().manual_seed(PERM_SEED)
    perms = [torch.randperm(n_edges, generator=gen) for _ in range(PERMS)]
    model64 = build(cls, kwargs, task, seed).double()
    # (the reference's unpack_graph casts features and coordinates to fp32: hand them to the fp64 layers as they are)
    model64.unpack_graph = lambda g: (g.x.double(), g.edge_index, g.pos.double(), g.edge_attr, g.batch)
    scores64, raw64 = recorded(fn, model64, graph, dtype=torch.float64)
    noise = float(np.abs(raw32 - raw64).max())
    for perm in perms:
        _, raw_p = recorded(fn, model, graph, perm=perm)
        if fn_name == 'bond_masking':     # forwards follow the permuted list: bring them back to edge ids
            order = perm.numpy()[np.nonzero(graph.edge_attr[perm][:, 1].numpy())[0]]
            back = np.empty(n_edges, dtype=np.int64)
            back[order] = np.arange(len(order))
            raw_p = np.concatenate([raw_p[:1], raw_p[1:][back[visited]]])
        noise = max(noise, float(np.abs(raw_p - raw64).max()))
    out = {
        'cfg': np.array(json.dumps({'case': name, 'class': cls.__name__, 'kwargs': dict(kwargs, model_task=task),
                                    'task': task, 'seed': seed, 'fn': fn_name, 'sigmoid': sigmoid, 'perms': PERMS,
                                    'perm_seed': PERM_SEED})),
        'in/x': graph.x.numpy().astype(np.float32), 'in/pos': graph.pos.numpy().astype(np.float32),
        'in/edge_index': graph.edge_index.numpy().astype(np.int32),
        'in/edge_type': graph.edge_attr.argmax(1).numpy().astype(np.uint8),
        'visited': visited.astype(np.int32), 'raw32': raw32.astype(np.float32), 'raw64': raw64,
        'scores': scores, 'scores64': scores64, 'noise32': np.float64(noise),
    }
    for k, v in sd.items():
        out[f'sd/{k}'] = v
    if extras:
        A.SIGMOID = False
        args = dict(edge_indices=graph.edge_index.clone(), edge_attrs=graph.edge_attr.clone())
        for extra in ('cam', 'node_attention', 'edge_attention'):
            out[f'extra/{extra}'] = np.asarray(getattr(A, extra)(build(cls, kwargs, task, seed), graph.pos[None],
                                                                 graph.x[None], **args), dtype=np.float32)
    A.SIGMOID = False
    path = HERE / f'{name}.npz'
    np.savez_compressed(path, **out)
    if fn_name == 'bond_masking':    # a contact is listed once per direction and both leave out the same two atoms: rank pairs
        ei = np.sort(graph.edge_index.numpy()[:, visited], axis=0)
        _, first = np.unique(ei[0] * graph.x.shape[0] + ei[1], return_index=True)
        ranked = np.sort(scores[visited[first]])[::-1]
    else:
        ranked = np.sort(scores)[::-1]
    bound = 2 * (1e-5 * float(np.abs(raw64).max()) + 4 * noise)
    print(f'{name:32s} N={graph.x.shape[0]:4d} E={n_edges:5d} masks={len(visited):4d} out0={raw32[0]} '
          f'noise32={noise:.2e} top gaps={np.round(ranked[:5] - ranked[1:6], 7)} 2*bound={bound:.2e} '
          f'{path.stat().st_size / 1024:.0f} KiB')
    assert ranked[0] - ranked[1] > bound, f'{name}: the top-1 gap does not exceed the bound; pick another seed'


def main():
    g1, _, _ = mg.reference_test_graphs()
    ball120 = mg.synthetic_ball_graph(120, 12, 4.0, seed=21)
    ball400 = mg.synthetic_ball_graph(400, 30, 4.0, seed=22)
    test_kwargs = {  # test/setup_and_params.py:72-87
        'cache': False, 'k': 32, 'num_layers': 6, 'dropout': 0, 'dim_input': 12,
        'dim_output': 1, 'dim_hidden': 32, 'pooling_only': True, 'graphnorm': True,
        'update_coords': True, 'node_attention': True, 'residual': True,
        'edge_attention': True, 'softmax_attention': True}
    cli_default = {  # parse_args.py store_true flags all False, point_vs.py:189-221
        'dim_input': 12, 'k': 32, 'dim_output': 1, 'num_layers': 3, 'residual': False,
        'edge_residual': False, 'edge_attention': False, 'normalize': False, 'tanh': False,
        'dropout': 0.0, 'graphnorm': False, 'update_coords': True,
        'permutation_invariance': False, 'node_attention': False, 'gated_residual': False,
        'rezero': False, 'softmax_attention': False}
    for f in sorted(HERE.glob('attr_*.npz')):
        f.unlink()
    run_case('attr_clidefault_ball120', ball120, SartorrasEGNN, cli_default, 'atom_masking')
    run_case('attr_clidefault_ball400', ball400, SartorrasEGNN, cli_default, 'atom_masking')
    run_case('attr_clidefault_g1', g1, SartorrasEGNN, cli_default, 'atom_masking')
    run_case('attr_testkwargs_g1', g1, SartorrasEGNN, test_kwargs, 'atom_masking', extras=True)
    run_case('attr_sigmoid_ball120', ball120, SartorrasEGNN, cli_default, 'atom_masking', sigmoid=True)
    run_case('attr_dimout3_ball120', ball120, SartorrasEGNN, dict(cli_default, dim_output=3), 'bond_masking')
    run_case('attr_multitask_reg_ball120', ball120, MultitaskSatorrasEGNN, dict(cli_default, dim_output=3),
             'bond_masking', task='regression')


if __name__ == '__main__':
    main()
