"""Host-side pins of the node-count inputs (tests/_node_count_cases.py): a GPU result on these graphs is a finding
only while the graphs have the shape the GPU tests rely on - the node counts on their boundaries, the four forced kinds
of node, both column-to-wave maps of the column gather. No GPU."""
import numpy as np
import pytest
import torch

from tests import _node_count_cases as ncc

COUNTS = tuple(ncc.NODE_COUNTS)


def test_the_node_counts_are_the_boundaries():
    assert COUNTS == (1, 2, 3, 5, 31, 32, 33, 127, 128, 129, 255, 256, 257, 511, 513, 5121, 8200, 16400, 32800)
    assert ncc.ONLY_AT_WIDTH == {16400: 64, 32800: 32}
    for tile in (32, 128, 256):                          # one below, on and one above every row tile
        assert {tile - 1, tile, tile + 1} <= set(COUNTS)
    assert {511, 513} <= set(COUNTS)
    assert min(n for n in COUNTS if n > 5120) == 5121    # the gather's 1280 blocks of 4 columns
    assert any(8192 < n <= 8200 for n in COUNTS)         # the generic edge kernels' 2048 blocks of 4 rows
    # ew_grid: 4096 blocks of 256 threads, one element each - the loops iterate above 2^20 elements
    for hid, first in ((128, 8200), (64, 16400), (32, 32800)):
        at_width = [n for n in COUNTS if ncc.ONLY_AT_WIDTH.get(n, hid) == hid]
        assert min(n for n in at_width if n * hid > 1 << 20) == first
        assert max(n for n in at_width if n < first) * hid <= 1 << 20
    assert max(COUNTS) >= 32768 and ncc.ONLY_AT_WIDTH[max(COUNTS)] == 32      # rows_m = 256


def test_both_gather_maps_occur_below_and_above_the_grid_cap():
    below = {ncc.gather_map_is_xcd_contiguous(n) for n in COUNTS if n <= 5120}
    above = {ncc.gather_map_is_xcd_contiguous(n) for n in COUNTS if n > 5120}
    assert below == {False, True} and above == {False, True}
    assert ncc.gather_map_is_xcd_contiguous(32) and not ncc.gather_map_is_xcd_contiguous(33)
    assert ncc.gather_map_is_xcd_contiguous(32800) and not ncc.gather_map_is_xcd_contiguous(5121)
    # every width class meets both maps: the counts a width does not run leave both parities behind
    for hid in (16, 32, 64, 128):
        seen = {ncc.gather_map_is_xcd_contiguous(n) for n in COUNTS
                if ncc.ONLY_AT_WIDTH.get(n, hid) == hid and (n <= 8200 or hid in (32, 64))}
        assert seen == {False, True}, hid


@pytest.mark.parametrize('n', COUNTS)
def test_node_graph_has_the_promised_shape(n):
    g = ncc.graph_for(n)
    ei = g.edge_index.numpy()
    e = ei.shape[1]
    assert g.n_nodes == n and g.pos.shape == (n, 3) and g.pos.dtype == torch.float32
    assert g.edge_index.dtype == torch.int64 and tuple(g.edge_index.shape) == (2, e)
    assert e == (0 if n == 1 else min(6 * n, 30000))
    assert g.edge_attr.dtype == torch.int64 and tuple(g.edge_attr.shape) == (e, 3)
    assert g.etype.dtype == torch.int64 and tuple(g.etype.shape) == (e,)
    if e == 0:
        return
    assert ei.min() >= 0 and ei.max() < n
    assert not (ei[0] == ei[1]).any(), 'self loops make normalize=True ill-conditioned'
    assert np.array_equal(g.edge_attr.numpy().argmax(1), g.etype.numpy()) and (g.edge_attr.sum(1) == 1).all()
    assert (np.bincount(g.etype.numpy(), minlength=3) > 0).all()
    assert (np.diff(ei[0]) < 0).any(), 'the list is not sorted by row: the sort path of the graph preparation'
    forced = ncc.forced_nodes(n)
    assert (forced is not None) == (n >= 8)
    if forced is None:
        return
    isolated, column_only, row_only, last = forced
    assert len({isolated, column_only, row_only, last}) == 4 and last == n - 1
    as_row, as_col = np.bincount(ei[0], minlength=n), np.bincount(ei[1], minlength=n)
    assert as_row[isolated] == 0 and as_col[isolated] == 0
    assert as_row[column_only] == 0 and as_col[column_only] > 0
    assert as_row[row_only] > 0 and as_col[row_only] == 0
    assert as_col[last] > 0 and as_row[last] > 0


def test_the_edgeless_graph():
    g = ncc.graph_for(ncc.EDGELESS_N, edges=False)
    assert ncc.EDGELESS_N == 37 and g.n_nodes == 37 and tuple(g.pos.shape) == (37, 3)
    assert tuple(g.edge_index.shape) == (2, 0) and g.edge_index.dtype == torch.int64
    assert tuple(g.edge_attr.shape) == (0, 3) and g.edge_attr.dtype == torch.int64 and tuple(g.etype.shape) == (0,)
    assert int(ncc.graph_for(1).edge_index.shape[1]) == 0


@pytest.mark.parametrize('n', [1, 5, 33, 5121])
def test_node_graph_is_deterministic(n):
    a, b = ncc.graph_for(n), ncc.graph_for(n)
    for name in ('pos', 'edge_index', 'edge_attr', 'etype'):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    if n > 1:
        assert not torch.equal(a.edge_index, ncc.node_graph(n, seed=7).edge_index)
