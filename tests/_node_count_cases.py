"""Inputs of the node-side tests (tests/test_gpu_node_side.py; pinned on the host by
tests/test_node_count_cases_host.py): graphs whose NODE COUNT sits on a boundary of the node-level kernels. The edge
side is kept ordinary on purpose (three classes, about six edges per node, at most 30,000): the edge kernels have
their own tests on the 96-node graphs of tests/_edge_class_cases.py.

`node_graph`    one graph of N nodes as an arbitrary-order COO list, the namespace of _edge_class_cases.class_graph
"""
from types import SimpleNamespace

import numpy as np
import torch

N_CLASSES = 3
EDGES_PER_NODE = 6
MAX_EDGES = 30000
FORCED_FROM = 8          # node counts from here on hold the four forced kinds of node

# node count -> the boundary it sits on (csrc/dense_ops.hip, node_ops.hip, edge_v0.hip)
NODE_COUNTS = {
    1: 'one row: every tile, wave and workgroup ragged; k_node_out_* clamps the other nodes of the wave to N - 1 = 0',
    2: 'half a wave of k_node_out_*<32> (2 nodes per wave), half a wave of <16> (4 per wave)',
    3: 'odd: the second wave of k_node_out_*<32> holds one node and one clamped lane group',
    5: 'one node past a full wave of k_node_out_*<16>; gather grid of 2 blocks (column-strided map)',
    31: 'one row short of a 32-row MFMA tile (k_node_mlp_*, linear_mfma_block); gather grid 8: XCD-contiguous map',
    32: 'exactly one 32-row MFMA tile; gather grid 8: XCD-contiguous map',
    33: 'one row into the second MFMA tile; gather grid 9: column-strided map',
    127: 'one row short of a 128-row workgroup (node_mlp_blocks, pvs_colreduce_blocks)',
    128: 'exactly one 128-row workgroup; gather grid 32: XCD-contiguous map',
    129: 'one row into the second 128-row workgroup',
    255: 'one row short of a 256-row block of k_node_wgrads (kWgRowsPerBlock)',
    256: 'exactly one row block of k_node_wgrads; gather grid 64: XCD-contiguous map',
    257: 'one row into the second row block of k_node_wgrads: two slabs to reduce',
    511: 'one row short of the 512 rows of a tsgemm block (kRowsPerBlock)',
    513: 'one row into the second tsgemm block',
    5121: 'first N above the 1280-block cap of k_node_gather (N > 5120): its waves loop over columns',
    8200: 'first cell above the 2048-block cap of the generic edge kernels (N > 8192); N H > 2^20 at H = 128',
    16400: 'N H > 2^20 at H = 64: the grid-stride loops of k_node_tail_* / k_node_out_* iterate (ew_grid caps at 4096)',
    32800: 'N H > 2^20 at H = 32, and N >= 32768: rows_m = 256 of the folded node MLP and of the g_h job',
}
ONLY_AT_WIDTH = {16400: 64, 32800: 32}       # run at this width alone; every other count at every width
EDGELESS_N = 37                              # one more graph: 37 nodes without an edge (N = 1 has none either)


def gather_map_is_xcd_contiguous(n_nodes):
    """k_node_gather sweeps the columns XCD by XCD when its grid is a multiple of 8; the grid is ceil(N / 4) blocks
    (capped at 1280 with weight sums, 2048 without)."""
    return ((n_nodes + 3) // 4) % 8 == 0


def forced_nodes(n_nodes):
    """(isolated, column_only, row_only, last) for N >= FORCED_FROM, else None.
    isolated      no edge touches it
    column_only   in-edges only: it is the column of edges, the row of none (its message sum is empty, its column
                  gather is not)
    row_only      out-edges only: the row of edges, the column of none (an empty column between columns with edges)
    last          node N - 1 as a column with edges (and as a row)"""
    if n_nodes < FORCED_FROM:
        return None
    return n_nodes // 2, n_nodes // 3, (2 * n_nodes) // 3, n_nodes - 1


def node_graph(n_nodes, seed, edges=True):
    """-> namespace(pos [N, 3] fp32, edge_index int64 [2, E], edge_attr int64 one-hot [E, 3], etype int64 [E], n_nodes).
    E = min(6 N, 30000) random directed pairs in arbitrary order (duplicates allowed, no self loops); N = 1 or
    edges=False: E = 0."""
    rng = np.random.default_rng(seed)
    n = int(n_nodes)
    e = min(EDGES_PER_NODE * n, MAX_EDGES) if (edges and n > 1) else 0
    forced = forced_nodes(n)
    nodes = np.arange(n)
    if forced is None:
        as_row = as_col = nodes
    else:
        isolated, column_only, row_only, last = forced
        as_row = np.setdiff1d(nodes, (isolated, column_only))
        as_col = np.setdiff1d(nodes, (isolated, row_only))
    row = rng.choice(as_row, size=e) if e else np.zeros(0, np.int64)
    col = rng.choice(as_col, size=e) if e else np.zeros(0, np.int64)
    clash = row == col                                   # no self loops: redraw the column
    while clash.any():
        col[clash] = rng.choice(as_col, size=int(clash.sum()))
        clash = row == col
    if forced is not None and e:
        row[:3] = (0, last, row_only)
        col[:3] = (last, column_only, 0)
    et = rng.integers(0, N_CLASSES, size=e)
    if e >= N_CLASSES:
        et[:N_CLASSES] = np.arange(N_CLASSES)            # every class has an edge
    order = rng.permutation(e)                           # the order of a COO list is arbitrary
    row, col, et = row[order], col[order], et[order].astype(np.int64)
    pos = (rng.normal(size=(n, 3)) * 3).astype(np.float32)
    etype = torch.from_numpy(et)
    return SimpleNamespace(
        pos=torch.from_numpy(pos), edge_index=torch.from_numpy(np.vstack([row, col]).astype(np.int64).reshape(2, e)),
        edge_attr=torch.nn.functional.one_hot(etype, N_CLASSES), etype=etype, n_nodes=n)


def graph_for(n_nodes, edges=True):
    """The graph every test of a node count shares (one seed per count)."""
    return node_graph(n_nodes, seed=1000 + n_nodes + (0 if edges else 500000), edges=edges)
