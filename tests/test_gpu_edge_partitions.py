"""The MFMA edge kernels on other work partitions than one chunk per wave.

Every MFMA edge kernel (forward at 256 / 512 / 768 threads, the two-launch H = 128 forward, the H = 32 f16x2, H = 64
split and H = 128 team backwards, the three exact-fp32 backwards) loops `for (chunk = first; chunk < n_chunks;
chunk += total_waves)` over row-aligned chunks. At the 3,200 ... 60,000 edges of the oracle tests every wave runs that
loop once; a second trip starts at 1 M ... 16.7 M edges. PVS_CHUNK_EDGES and PVS_EDGES_PER_WAVE (edge_dispatch.h, read at
every call) bring the other regimes down to a 3,200-edge graph (tests/_edge_partition_cases.py, pinned on the host by
tests/test_edge_partition_cases_host.py and, for the grids, by tests/test_edge_dispatch.py):

    many_chunks   the default grid, several chunks per wave: the per-chunk reset of the open-row accumulators, cur_row,
                  the running softmax maximum and prev_row, LDS tiles reused after a chunk's last partial tile, weight-
                  gradient accumulators that must survive from chunk to chunk
    one_block     one workgroup, 9 ... 25 chunks per wave in turn
    fine          the grid at its block cap (exact H = 32: every slab the workspace holds), almost every chunk empty

on graphs whose 200-edge row lies inside, at the start (chunks [0, 0): e_end = 0) and at the end of the range.

Arbiter and bound: those of tests/test_gpu_edge_classes.py, whose Problem this file reuses - autograd on the fp64
oracle layer, assert_strict with three fp32 oracle draws, per tensor, the class columns on their own.
"""
import contextlib
import functools
import os

import pytest

from tests import _edge_partition_cases as epc
from tests.test_gpu_edge_classes import Problem, _environment, problem

pytestmark = pytest.mark.gpu

PARTITION_NAMES = tuple(epc.PARTITIONS)


def _cell(graph, A, hid, family, flags, partition):
    tag = f'{graph}-A{A}-H{hid}-{family}-{flags}-{partition}'
    return pytest.param(dict(graph=graph, A=A, hid=hid, family=family, flags=flags, partition=partition,
                             env=epc.PARTITIONS[partition], tag=tag), id=tag)


def _cells():
    out = []
    # every kernel of both families under every partition (H = 128 'exact': the wide forward, the exact backward)
    for hid in (32, 64, 128):
        for family in ('default', 'exact'):
            for flags in ('plain', 'full', 'soft'):
                out += [_cell('mixed', 3, hid, family, flags, part) for part in PARTITION_NAMES]
    # empty chunks at the start and at the end of the range
    for graph in ('hub_first', 'hub_last'):
        for hid in (32, 64, 128):
            for family in ('default', 'exact'):
                out += [_cell(graph, 3, hid, family, 'full', part) for part in ('many_chunks', 'fine')]
    # the 512-thread forward with the generic backward; a null etype; hidden 100 zero-padded to the 128-channel kernels
    out += [_cell('mixed', 5, 64, 'default', 'soft', part) for part in PARTITION_NAMES]
    out.append(_cell('mixed', 0, 32, 'default', 'plain', 'many_chunks'))
    out.append(_cell('mixed', 2, 100, 'default', 'full', 'many_chunks'))
    return out


CELLS = _cells()


@functools.lru_cache(maxsize=None)
def _problem(graph, A, hid, flags):
    """Inputs and oracle references, built once per (graph, A, hid, flags) and left unchanged; `mixed` is the problem
    of the edge-class tests itself."""
    if graph == 'mixed':
        return problem(A, hid, flags)
    return Problem(A, hid, flags, graph=epc.graph(graph, A))


@contextlib.contextmanager
def _nothing_set():
    """The default partition: neither override is in the environment."""
    names = ('PVS_CHUNK_EDGES', 'PVS_EDGES_PER_WAVE')
    old = {k: os.environ.pop(k, None) for k in names}
    try:
        yield
    finally:
        os.environ.update({k: v for k, v in old.items() if v is not None})


@pytest.mark.parametrize('cell', CELLS)
def test_layer_on_another_work_partition_matches_the_fp64_oracle(cell):
    """Outputs, input gradients and every parameter gradient of one EGNNLayer.forward + backward under the strict
    bound, with the edge range cut as the cell's partition says."""
    p = _problem(cell['graph'], cell['A'], cell['hid'], cell['flags'])
    with _nothing_set(), _environment(cell):
        got = p.gpu()
    p.check(got, cell['tag'])


@pytest.mark.parametrize('family', ['default', 'exact'])
@pytest.mark.parametrize('hid', [32, 64, 128])
def test_chunk_override_reaches_the_backward_launcher(hid, family):
    """The witness that the cells above ran on another partition: more chunks per wave hand every wave other edges,
    so the weight-gradient slabs are summed over other subsets - another summation tree, other low-order bits in
    grad edge_mlp.2.weight than with nothing set (and the same bits when the same call is made twice)."""
    p = _problem('mixed', 3, hid, 'full')
    key = 'grad edge_mlp.2.weight'
    with _nothing_set():
        with _environment(dict(family=family, env={})):
            default, again = p.gpu()[key], p.gpu()[key]
        with _environment(dict(family=family, env=epc.PARTITIONS['many_chunks'])):
            many = p.gpu()[key]
    assert default.tobytes() == again.tobytes()
    assert default.tobytes() != many.tobytes(), 'PVS_CHUNK_EDGES did not change the backward launch'


@pytest.mark.parametrize('partition', PARTITION_NAMES)
@pytest.mark.parametrize('hid', [32, 64, 128])
def test_layer_on_another_work_partition_is_bitwise_reproducible(hid, partition):
    p = _problem('mixed', 3, hid, 'full')
    with _nothing_set(), _environment(dict(family='default', env=epc.PARTITIONS[partition])):
        first, second = p.gpu(), p.gpu()
    assert set(first) == set(second)
    differing = [k for k in first if first[k].tobytes() != second[k].tobytes()]
    assert not differing, differing
