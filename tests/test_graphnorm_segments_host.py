"""GraphNorm per node segment, the host side (no GPU): the fp64 restatement (tests/_graphnorm_segments_ref.py) is pinned
to tests/_graphnorm_rows_ref.py applied to every segment alone, to the oracle's GraphNorm run on each graph alone, and to
its independence of the rows that belong to no segment; then the ABI: version and PvsGraph unchanged, the flag's value, the
export in the header, in the library and in the binding. tests/test_gpu_graphnorm_segments.py holds the kernels to this
reference.
"""
import ctypes
import re
from pathlib import Path

import pytest
import torch

from oracle import egnn_oracle as orc
from tests import _graphnorm_rows_ref as rref
from tests import _graphnorm_segments_ref as sref

ROOT = Path(__file__).resolve().parents[1]
# (N_cap, table): unowned rows in front and behind, an empty segment, single rows; out-of-range and backward entries
TABLES = [
    (40, [0, 40]),
    (40, [3, 3, 4, 6, 30, 37]),
    (300, [10, 10, 11, 13, 140, 268, 290]),
    (50, [-4, 7, 7, 61]),              # clamped to [0, 7, 7, 50]
    (50, [5, 20, 12, 40]),             # a segment that ends in front of its start has length 0
]


def _rel(got, want):
    scale = float(want.abs().max())
    return float((got - want).abs().max()) / (scale if scale > 0 else 1.0)


@pytest.mark.parametrize('hidden', [16, 30])
@pytest.mark.parametrize('n_cap, table', TABLES)
def test_every_segment_is_the_row_reference_on_its_rows_alone(n_cap, table, hidden):
    y, w, b, ms, _ = rref.case(n_cap, hidden)
    st = sref.stats(y, ms, table)
    out = sref.forward(y, w, b, ms, table)
    assert st.shape == (len(table) - 1, 2 * hidden)
    spans = sref.clamped(table, n_cap)
    for s, (a, n) in enumerate(spans):
        rows = y[a:a + n]
        mean, var = rref.stats(rows, ms, n)
        assert torch.equal(st[s, :hidden], mean) and torch.equal(st[s, hidden:], var), s
        if n:
            later = any(a2 < a + n and a < a2 + n2 for a2, n2 in spans[s + 1:] if n2)      # (overlap: the last one wins)
            if not later:
                assert _rel(out[a:a + n], rref.forward(rows, w, b, ms, n)) <= 1e-14, s
                # ... which is the oracle's GraphNorm on that graph alone (GraphNorm called without a batch vector)
                assert _rel(out[a:a + n], orc.graph_norm(rows, w, b, ms)) <= 1e-13, s
        else:
            assert not st[s].any()
    # rows of no segment: mean = var = 0, the n = 0 contract of the row-count route; finite
    free = ~sref.owned(table, n_cap)
    if free.any():
        assert torch.equal(out[free], rref.forward(y[free], w, b, ms, 0))
        assert torch.isfinite(out[free]).all()


def test_the_clamp_and_the_lengths():
    assert sref.clamped([-4, 7, 7, 61], 50) == [(0, 7), (7, 0), (7, 43)]
    assert sref.clamped([5, 20, 12, 40], 50) == [(5, 15), (20, 0), (12, 28)]
    assert sref.clamped([0, 0], 0) == [(0, 0)]


@pytest.mark.parametrize('poison', ['random', 1e30, float('nan')])
def test_unowned_rows_reach_no_segment(poison):
    n_cap, table, hidden = 300, [10, 10, 11, 13, 140, 268, 290], 16
    y, w, b, ms, _ = rref.case(n_cap, hidden)
    free = ~sref.owned(table, n_cap)
    other = y.clone()
    other[free] = torch.randn(int(free.sum()), hidden, dtype=torch.float64) * 7 if poison == 'random' else poison
    assert torch.equal(sref.stats(y, ms, table), sref.stats(other, ms, table))
    assert torch.equal(sref.forward(y, w, b, ms, table)[~free], sref.forward(other, w, b, ms, table)[~free])


def test_one_segment_over_every_row_is_the_oracles_graphnorm():
    y, w, b, ms, _ = rref.case(207, 32)
    assert _rel(sref.forward(y, w, b, ms, [0, 207]), orc.graph_norm(y, w, b, ms)) <= 1e-14


def test_abi_unchanged_flag_value_and_export():
    from pointvs_amd import _lib
    from pointvs_amd import functional as PF
    from pointvs_amd.graph import PreparedGraph
    header = (ROOT / 'include' / 'pvs_egnn.h').read_text()
    # what cannot move
    assert _lib.MIN_VERSION == 113 and _lib.lib().pvs_version() == 113
    assert ctypes.sizeof(_lib.PvsGraph) == 104 == _lib.PVS_GRAPH_SIZEOF
    assert _lib.PvsGraph.n_norm_rows_dev.offset == 96
    assert 'sizeof(PvsGraph) == 104 && offsetof(PvsGraph, n_norm_rows_dev) == 96' in header
    # the flag: bit 12, the first free one behind PVS_SOFTMAX_ATT, the same in the header and in the binding
    stated = re.search(r'PVS_GRAPHNORM_SEGMENTS\s*=\s*1u\s*<<\s*(\d+)', header)
    assert stated and int(stated.group(1)) == 12
    assert _lib.GRAPHNORM_SEGMENTS == 1 << 12 == 2 * _lib.SOFTMAX_ATT
    flags = [_lib.RESIDUAL, _lib.EDGE_RESIDUAL, _lib.EDGE_ATTENTION, _lib.NORMALIZE, _lib.TANH, _lib.GRAPHNORM,
             _lib.UPDATE_COORDS, _lib.PERM_INVARIANT, _lib.NODE_ATTENTION, _lib.GATED_RESIDUAL, _lib.REZERO,
             _lib.SOFTMAX_ATT, _lib.GRAPHNORM_SEGMENTS]
    assert flags == [1 << k for k in range(13)]
    # the contract is written down at both places
    member = header[header.index('const int32_t* graph_eptr;'):header.index('const int32_t* n_norm_rows_dev;')]
    assert 'PVS_GRAPHNORM_SEGMENTS' in member
    for name, n_args in (('pvs_graphnorm_stats_segments', 10), ('pvs_graphnorm_stats_segments_workspace_bytes', 3)):
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert name in _lib.EXPORTED_SYMBOLS and len(_lib._PROTOTYPES[name][1]) == n_args and hasattr(_lib.lib(), name)
    assert callable(PF.graphnorm_stats_segments) and callable(PreparedGraph.set_norm_segments)
    # the workspace of the operator: grows with the segments and with the rows, never zero
    ws = _lib.lib().pvs_graphnorm_stats_segments_workspace_bytes
    assert 0 < ws(0, 1, 16) <= ws(1000, 1, 16) <= ws(1000, 9, 16) <= ws(1000, 9, 128)
    # the layer workspace grows under the flag, for both the full and the partial forwards, and only under it
    size = _lib.lib().pvs_egnn_layer_workspace_bytes
    for mode in (0, 2, 3):
        plain = size(ctypes.byref(_lib.PvsLayerDesc(32, 3, _lib.GRAPHNORM, 0)), 500, 4000, mode)
        segs = size(ctypes.byref(_lib.PvsLayerDesc(32, 3, _lib.GRAPHNORM | _lib.GRAPHNORM_SEGMENTS, 0)), 500, 4000, mode)
        assert segs >= plain + 4 * (2 * 500 * 32 + (500 + 500 // 128 + 1) * 32), mode
