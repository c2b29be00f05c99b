"""Host-side pins of the work-partition inputs (tests/_edge_partition_cases.py): the GPU tests of
tests/test_gpu_edge_partitions.py say something about the seams between chunks only while the graphs and the chunk
plans have the shape they rely on - several chunks per wave, empty chunks at the start (e_end = 0), inside and at the
end of the range, a last chunk that ends on a partial tile. No GPU."""
import numpy as np
import pytest
import torch

from tests import _edge_class_cases as ecc
from tests import _edge_partition_cases as epc
from tests.test_edge_dispatch import parent_grid


def _sorted(g):
    d = ecc.prepared_definition(g.edge_index, g.etype, g.n_nodes)
    return d['rowptr'], d['row']


@pytest.mark.parametrize('A', ecc.CLASS_COUNTS)
def test_hub_graph_is_the_class_graph_recipe(A):
    a, b = ecc.class_graph(A, seed=100 + A), epc.hub_graph(A, 100 + A, ecc.HUB, ecc.ISOLATED)
    assert torch.equal(a.edge_index, b.edge_index) and torch.equal(a.pos, b.pos)
    assert (a.etype is None and b.etype is None) or torch.equal(a.etype, b.etype)
    assert (a.edge_attr is None and b.edge_attr is None) or torch.equal(a.edge_attr, b.edge_attr)
    m = epc.graph('mixed', A)
    assert torch.equal(m.edge_index, a.edge_index) and torch.equal(m.pos, a.pos)


@pytest.mark.parametrize('name', list(epc.GRAPHS))
def test_graphs_have_the_promised_shape(name):
    hub, isolated = epc.GRAPHS[name]
    g = epc.graph(name, 3)
    ei = g.edge_index.numpy()
    assert ei.shape == (2, epc.N_EDGES) and g.n_nodes == 96 and g.pos.dtype == torch.float32
    assert not (ei[0] == ei[1]).any() and not np.isin(ei, isolated).any() and len(isolated) == 5
    rowptr, row = _sorted(g)
    deg = np.diff(rowptr)
    assert deg[hub] >= ecc.HUB_EDGES and deg.argmax() == hub and np.sort(deg)[-2] < 64
    et = g.etype.numpy()
    counts = np.bincount(et, minlength=3)
    assert (counts > 0).all() and counts[2] == 1 and set(et[ei[0] == hub]) == {0, 1, 2}
    assert np.array_equal(g.edge_attr.numpy().argmax(1), et)
    if name == 'hub_first':
        assert rowptr[0] == 0 and rowptr[1] == deg[hub]
    if name == 'hub_last':
        assert rowptr[-1] == epc.N_EDGES and rowptr[-2] == epc.N_EDGES - deg[hub]
        # the range ends on a partial tile of every tile size in use (32 and 16 edges), however the last chunk starts
        assert deg[hub] % 16 != 0
    if name == 'mixed':
        assert deg[-1] == 0 and deg[0] > 0, 'the last node is isolated, the first is not'


@pytest.mark.parametrize('site', list(epc.SITES))
@pytest.mark.parametrize('partition', list(epc.PARTITIONS))
@pytest.mark.parametrize('name', list(epc.GRAPHS))
def test_chunk_plans_hold_the_seams_the_gpu_tests_are_about(name, partition, site):
    hub, _ = epc.GRAPHS[name]
    rowptr, row = _sorted(epc.graph(name, 3))
    nw, cap, floor, chunk = epc.site_parameters(site, partition)
    blocks, n_chunks = parent_grid(epc.N_EDGES, nw, cap, floor, chunk)
    b = epc.chunk_bounds(rowptr, row, n_chunks)
    # the chunks tile the range, in order, and every chunk starts at a row start: each row has one owner
    assert b[0] == 0 and b[-1] == epc.N_EDGES and (np.diff(b) >= 0).all() and np.isin(b, rowptr).all()
    lens = np.diff(b)
    per_wave = n_chunks // (blocks * nw)
    slot = epc.N_EDGES / n_chunks
    team = not epc.SITES[site][2]
    if partition in ('many_chunks', 'one_block'):
        assert per_wave >= 2
        # a wave's (team's) chunks k, k + waves, ...: a quarter of the waves or more run two or more chunks that hold
        # edges (one such wave would do), so the state of an open row at a chunk's end meets a fresh chunk
        waves = blocks * nw
        busy = (lens.reshape(per_wave, waves) > 0).sum(axis=0)
        assert (busy >= 2).sum() >= max(waves // 4, 1), busy
        # and chunks without edges lie between chunks with edges (the hub row is longer than several slots)
        assert slot < 40 and (lens == 0).sum() >= 3
    if partition == 'fine' and not team:
        assert slot <= 4 and (lens > 0).sum() <= 91 < n_chunks // 4, 'at most one chunk per row with edges holds edges'
        if cap <= epc.N_EDGES // nw:
            assert blocks == cap
    if partition == 'fine' and team:
        assert (blocks, n_chunks) == parent_grid(epc.N_EDGES, nw, cap, epc.TEAM_FLOOR, 4096), 'the default plan'
    if not (partition == 'fine' and team):
        hub_lo, hub_hi = int(rowptr[hub]), int(rowptr[hub + 1])
        inside = [k for k in range(n_chunks) if hub_lo <= k * epc.N_EDGES // n_chunks < hub_hi]
        assert len(inside) >= 4
        # every slot inside the hub row starts at the row's first edge: all but the last of them are empty, the last
        # owns the row
        assert (b[inside] == hub_lo).all() and (lens[inside[:-1]] == 0).all() and lens[inside[-1]] >= hub_hi - hub_lo
        if name == 'hub_first':
            assert b[1] == 0 and b[2] == 0, 'the first chunks are [0, 0): e_end = 0'
        if name == 'hub_last':
            assert inside[-1] == n_chunks - 1 and lens[-2] == 0 and lens[-1] == hub_hi - hub_lo
            assert lens[-1] % 32 != 0 and lens[-1] % 16 != 0


def test_exact_h32_under_fine_leaves_every_slab_the_workspace_holds():
    nw, cap, floor, chunk = epc.site_parameters('exact_h32', 'fine')
    blocks, _ = parent_grid(epc.N_EDGES, nw, cap, floor, chunk)
    assert blocks == cap == epc.SLAB_CAPACITY
