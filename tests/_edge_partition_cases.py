"""Inputs of the work-partition tests of the MFMA edge kernels (tests/test_gpu_edge_partitions.py and the partition
test of tests/test_edge_dispatch.py; pinned on the host by tests/test_edge_partition_cases_host.py). Plain numpy.

Every MFMA edge kernel walks its edge range as `for (chunk = first; chunk < n_chunks; chunk += total_waves)` over
row-aligned chunks (edge_mfma_common.h chunk_begin) on the grid that pvs_edge_grid plans (edge_dispatch.h). At the
3,200 edges of the test graphs the default plan gives every wave exactly one chunk. PARTITIONS holds the environment
overrides (read by the library at every call) that bring the other regimes down to that size; GRAPHS the row layouts
that put empty chunks at the start, in the middle and at the end of the range.
"""
from types import SimpleNamespace

import numpy as np
import torch

from tests import _edge_class_cases as ecc

PARTITIONS = {
    # the default grid, several chunks per wave (team); many chunks are shorter than a row
    'many_chunks': {'PVS_CHUNK_EDGES': '16'},
    # one workgroup whose waves take 9 ... 25 chunks each in turn: neighbouring chunks belong to different waves of one
    # block (the team kernels keep their 512 edges per team: seven blocks of 15 chunks)
    'one_block': {'PVS_EDGES_PER_WAVE': '4096', 'PVS_CHUNK_EDGES': '32'},
    # the grid at its block cap, about one edge per chunk slot: almost every chunk is empty (the team kernels keep
    # their floor, so this is their default plan)
    'fine': {'PVS_EDGES_PER_WAVE': '1'},
}

N_NODES = ecc.N_NODES
LAST = N_NODES - 1
# name -> (hub row, isolated nodes). `mixed` is ecc.class_graph itself; the hub variants move the 200-edge row to the
# first and to the last node (which `mixed` leaves isolated: there another node takes its place).
GRAPHS = {
    'mixed': (ecc.HUB, ecc.ISOLATED),
    'hub_first': (0, ecc.ISOLATED),
    'hub_last': (LAST, (7, 30, 31, 64, LAST - 1)),
}
N_EDGES = ecc.N_RANDOM + ecc.HUB_EDGES


def hub_graph(A, seed, hub, isolated):
    """The recipe of ecc.class_graph (same draws in the same order) with the hub row and the isolated nodes as
    arguments: hub_graph(A, seed, ecc.HUB, ecc.ISOLATED) IS class_graph(A, seed) (pinned by the host test)."""
    rng = np.random.default_rng(seed)
    live = np.setdiff1d(np.arange(N_NODES), isolated)
    row = rng.choice(live, size=ecc.N_RANDOM)
    col = rng.choice(live, size=ecc.N_RANDOM)
    clash = row == col
    while clash.any():
        col[clash] = rng.choice(live, size=int(clash.sum()))
        clash = row == col
    others = live[live != hub]
    hub_col = rng.choice(others, size=ecc.HUB_EDGES)
    row = np.concatenate([row, np.full(ecc.HUB_EDGES, hub)])
    col = np.concatenate([col, hub_col])
    order = rng.permutation(row.size)
    row, col = row[order], col[order]
    et = None
    if A:
        et = ecc.draw_classes(rng, row.size, A, np.flatnonzero(row == hub))
    pos = (rng.normal(size=(N_NODES, 3)) * 3).astype(np.float32)
    return SimpleNamespace(
        pos=torch.from_numpy(pos), edge_index=torch.from_numpy(np.vstack([row, col]).astype(np.int64)),
        edge_attr=None if et is None else ecc.one_hot(et, A), etype=None if et is None else torch.from_numpy(et),
        n_nodes=N_NODES)


def graph(name, A):
    """The graph `name` with A classes, seeded as the edge-class tests seed theirs (100 + A)."""
    if name == 'mixed':
        return ecc.class_graph(A, seed=100 + A)
    hub, isolated = GRAPHS[name]
    return hub_graph(A, 100 + A, hub, isolated)


def chunk_bounds(rowptr, row_sorted, n_chunks):
    """chunk_begin (edge_mfma_common.h) for k = 0 ... n_chunks over the full range: chunk k is
    [bounds[k], bounds[k + 1]); it starts at the row that contains edge k * E / n_chunks."""
    e = int(row_sorted.size)
    t = np.arange(1, n_chunks, dtype=np.int64) * e // n_chunks
    inner = np.asarray(rowptr, dtype=np.int64)[np.asarray(row_sorted)[t]]
    return np.concatenate([[0], inner, [e]])


# ---- the launch sites of pvs_edge_grid, as the GPU tests reach them ------------------------------------------------------
# site -> (waves or teams per block, block cap, honours PVS_EDGES_PER_WAVE, default chunk size): the SITES table of
# tests/test_edge_dispatch.py, with the floor as a flag (the team kernels pass a literal 512).
SITES = {
    'fwd_256': (4, 1024, True, 4096),
    'fwd_512': (8, 256, True, 4096),
    'fwd_768': (12, 256, True, 4096),
    'fwd_wide': (4, 256, True, 4096),
    'bwd_f16': (8, 256, True, 8192),
    'bwd_h64': (4, 256, True, 4096),
    'bwd_wide': (1, 256, False, 4096),
    'exact_wide': (1, 256, False, 4096),
    'exact_h32': (4, 512, True, 4096),
    'exact_h64': (1, 512, False, 4096),
}
TEAM_FLOOR = 512
SLAB_CAPACITY = 512


def site_parameters(site, partition):
    """(waves per block, cap, edges-per-wave floor, chunk size) of a launch site under a partition's environment."""
    nw, cap, honours_floor, chunk = SITES[site]
    env = PARTITIONS[partition]
    floor = int(env.get('PVS_EDGES_PER_WAVE', 64)) if honours_floor else TEAM_FLOOR
    return nw, cap, floor, int(env.get('PVS_CHUNK_EDGES', chunk))
