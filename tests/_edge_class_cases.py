"""Inputs of the edge-class tests (tests/test_gpu_edge_classes.py; pinned on the host by
tests/test_edge_class_cases_host.py): small graphs whose edges carry A = 0 ... 8 one-hot classes, shaped so that a
kernel that mishandles a class count gives wrong numbers.

`class_graph`   one graph as an arbitrary-order COO list (the sort path of pvs_graph_prepare)
`class_runs`    a batch in the reference loader's layout (two row-sorted runs per graph: pvs_graph_prepare_runs)
"""
from types import SimpleNamespace

import numpy as np
import torch

N_NODES = 96
ISOLATED = (7, 30, 31, 64, 95)      # no edge touches them: rows without edges between rows with edges, and the last row
HUB = 40                            # one row of HUB_EDGES edges
HUB_EDGES = 200
N_RANDOM = 3000                     # random directed pairs (duplicates allowed, no self loops)
CLASS_COUNTS = (0, 1, 2, 3, 4, 5, 8)


def n_live_classes(A):
    """Classes that have edges: all of them, except that A = 8 leaves its last class empty."""
    return 7 if A == 8 else A


def draw_classes(rng, n_edges, A, must_hold):
    """Class vector [n_edges] for A >= 1. With K = n_live_classes(A): class K - 1 (K >= 2) has exactly ONE edge, the
    classes 0 ... K - 2 get shares that fall as 2^-c, and the positions `must_hold` (K of them: edges of the hub row)
    carry the classes 0 ... K - 1 in this order, so the hub row holds every class that has edges."""
    K = n_live_classes(A)
    common = max(K - 1, 1)
    p = 0.5 ** np.arange(common)
    et = rng.choice(common, size=n_edges, p=p / p.sum())
    et[np.asarray(must_hold[:K])] = np.arange(K)
    return et.astype(np.int64)


def one_hot(et, A):
    return torch.nn.functional.one_hot(torch.from_numpy(et), A)       # int64, as the reference loader emits it


def class_graph(A, seed, odd_edges=False):
    """-> namespace(pos [96, 3] fp32, edge_index int64 [2, E], edge_attr int64 one-hot [E, A] or None (A = 0),
    etype int64 [E] or None, n_nodes). E = 3200 (3201 with odd_edges)."""
    rng = np.random.default_rng(seed)
    live = np.setdiff1d(np.arange(N_NODES), ISOLATED)
    n_rand = N_RANDOM + (1 if odd_edges else 0)
    row = rng.choice(live, size=n_rand)
    col = rng.choice(live, size=n_rand)
    clash = row == col                                  # no self loops: redraw the column among the other nodes
    while clash.any():
        col[clash] = rng.choice(live, size=int(clash.sum()))
        clash = row == col
    others = live[live != HUB]
    hub_col = rng.choice(others, size=HUB_EDGES)
    row = np.concatenate([row, np.full(HUB_EDGES, HUB)])
    col = np.concatenate([col, hub_col])
    order = rng.permutation(row.size)                   # the order of a COO list is arbitrary: the hub's edges lie scattered
    row, col = row[order], col[order]
    et = None
    if A:
        et = draw_classes(rng, row.size, A, np.flatnonzero(row == HUB))
    pos = (rng.normal(size=(N_NODES, 3)) * 3).astype(np.float32)
    return SimpleNamespace(
        pos=torch.from_numpy(pos), edge_index=torch.from_numpy(np.vstack([row, col]).astype(np.int64)),
        edge_attr=None if et is None else one_hot(et, A), etype=None if et is None else torch.from_numpy(et),
        n_nodes=N_NODES)


RUNS_SIZES = ((120, 10, 5.0), (57, 5, 5.0), (90, 8, 6.0))     # (nodes, ligand atoms, radius) of synthetic_graph


def class_runs(A, seed, odd_edges=False):
    """A Batch of three synthetic complexes in the loader's layout (tagged edge_layout == 'generate_edges'), its three
    structural classes replaced by A classes drawn as in `class_graph` (the row of most edges plays the hub). The
    loader's lists have an even number of edges (both directions of every pair); odd_edges drops the last edge of the
    last graph, which leaves two row-sorted runs. -> (batch, etype int64 [E] or None); batch.edge_attr is None for A = 0."""
    from pointvs_amd.graph import Batch
    from pointvs_amd.synthetic import synthetic_graph
    items = [synthetic_graph(seed + k, n_nodes=n, n_lig=nl, edge_radius=r) for k, (n, nl, r) in enumerate(RUNS_SIZES)]
    if odd_edges:
        last = items[-1]
        last.edge_index = last.edge_index[:, :-1].contiguous()
        last.edge_attr = last.edge_attr[:-1].contiguous()
    batch = Batch.from_data_list(items)
    rows = batch.edge_index[0].numpy()
    et = None
    if A:
        hub = int(np.bincount(rows).argmax())
        et = draw_classes(np.random.default_rng(seed), rows.size, A, np.flatnonzero(rows == hub))
    batch.edge_attr = None if et is None else one_hot(et, A)
    return batch, (None if et is None else torch.from_numpy(et))


def prepared_definition(edge_index, etype, n_nodes):
    """What pvs_graph_prepare must produce, by its definition in numpy (CSR by row, stable; CSC lists over the sorted
    edges, stable): dict of rowptr, row, col, etype (None for A = 0), perm, inv_deg, colptr, cedge."""
    row = edge_index[0].numpy().astype(np.int64)
    col = edge_index[1].numpy().astype(np.int64)
    perm = np.argsort(row, kind='stable')
    row_s, col_s = row[perm], col[perm]
    nodes = np.arange(n_nodes + 1)
    rowptr = np.searchsorted(row_s, nodes)
    deg = np.diff(rowptr)
    cedge = np.argsort(col_s, kind='stable')
    return dict(rowptr=rowptr, row=row_s, col=col_s, etype=None if etype is None else etype.numpy()[perm], perm=perm,
                inv_deg=(1.0 / np.maximum(deg, 1)).astype(np.float32), colptr=np.searchsorted(col_s[cedge], nodes),
                cedge=cedge)
