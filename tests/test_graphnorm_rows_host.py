"""GraphNorm over a leading row range, the host side (no GPU): the fp64 restatement (tests/_graphnorm_rows_ref.py) is
pinned to the oracle's GraphNorm, to its independence of the rows behind the range, and its closed-form backward - the
one the kernels compute - to torch.autograd; then the ABI: the new PvsGraph member, the export, the version.
tests/test_gpu_graphnorm_rows.py holds the kernels to this reference.
"""
import ctypes
import inspect
import re
from pathlib import Path

import pytest
import torch

from oracle import egnn_oracle as orc
from tests import _graphnorm_rows_ref as gref

ROOT = Path(__file__).resolve().parents[1]
GRAD_SHAPES = [(1, 1), (5, 3), (130, 129), (7, 0)]      # (N_cap, n)
KEYS = ('y', 'weight', 'bias', 'mean_scale', 'bias_in_front')


def _rel(got, want):
    scale = float(want.abs().max())
    return float((got - want).abs().max()) / (scale if scale > 0 else 1.0)


@pytest.mark.parametrize('hidden', [16, 32])
@pytest.mark.parametrize('n', [1, 5, 207])
def test_the_reference_is_the_oracles_graphnorm_when_every_row_counts(hidden, n):
    y, w, b, ms, _ = gref.case(n, hidden)
    want = orc.graph_norm(y, w, b, ms)
    got = gref.forward(y, w, b, ms, n)
    assert _rel(got, want) <= 1e-14


@pytest.mark.parametrize('poison', ['random', 1e30, float('nan')])
@pytest.mark.parametrize('n_cap, n', [(5, 3), (130, 129), (300, 43), (7, 0)])
def test_statistics_and_leading_rows_do_not_depend_on_the_rows_behind_the_range(n_cap, n, poison):
    hidden = 16
    y, w, b, ms, _ = gref.case(n_cap, hidden)
    other = y.clone()
    other[n:] = torch.randn(n_cap - n, hidden, dtype=torch.float64) * 7 if poison == 'random' else poison
    for a, c in zip(gref.stats(y, ms, n), gref.stats(other, ms, n)):
        assert torch.equal(a, c)
    assert torch.equal(gref.forward(y, w, b, ms, n)[:n], gref.forward(other, w, b, ms, n)[:n])
    if n == 0:
        mean, var = gref.stats(other, ms, 0)
        assert not mean.any() and not var.any()
        assert torch.isfinite(gref.forward(y, w, b, ms, 0)).all()       # rstd = 1 / sqrt(eps)


@pytest.mark.parametrize('hidden', [16, 32])
@pytest.mark.parametrize('n_cap, n', GRAD_SHAPES)
def test_closed_form_backward_is_autograds(n_cap, n, hidden):
    y, w, b, ms, g = gref.case(n_cap, hidden)
    closed = gref.closed_form_backward(y, w, ms, n, g)
    auto = gref.autograd_backward(y, w, b, ms, n, g)
    for key in KEYS:
        assert closed[key].shape == auto[key].shape
        assert _rel(closed[key], auto[key]) <= 1e-12, (key, _rel(closed[key], auto[key]))
    # the row bound: a row behind the range gets g_out * weight * rstd alone
    if n < n_cap:
        _, var = gref.stats(y, ms, n)
        assert _rel(closed['y'][n:], g[n:] * w / (var + gref.EPS).sqrt()) <= 1e-14


@pytest.mark.parametrize('hidden', [16, 32])
@pytest.mark.parametrize('n_cap, n', [(5, 3), (130, 129), (400, 207)])
def test_zero_gradient_behind_the_range_gives_the_unpadded_gradients(n_cap, n, hidden):
    y, w, b, ms, g = gref.case(n_cap, hidden)
    g[n:] = 0
    padded = gref.closed_form_backward(y, w, ms, n, g)
    alone = gref.autograd_backward(y[:n], w, b, ms, n, g[:n])
    assert not padded['y'][n:].any()
    assert _rel(padded['y'][:n], alone['y']) <= 1e-12
    for key in KEYS[1:]:
        assert _rel(padded[key], alone[key]) <= 1e-12, key


def test_abi_graph_member_export_and_version():
    from pointvs_amd import _lib
    from pointvs_amd import functional as PF
    from pointvs_amd.graph import PreparedGraph
    header = (ROOT / 'include' / 'pvs_egnn.h').read_text()
    assert _lib.MIN_VERSION == 113 and _lib.lib().pvs_version() == 113
    fields = [name for name, _ in _lib.PvsGraph._fields_]
    assert fields[-1] == 'n_norm_rows_dev' and fields[-3:-1] == ['graph_eptr', 'n_graphs']
    # the layout the header states (and static_asserts when compiled as C++)
    stated = re.search(r'sizeof\(PvsGraph\) = (\d+), offsetof\(PvsGraph, n_norm_rows_dev\) = (\d+)', header)
    assert stated, 'include/pvs_egnn.h no longer states the layout of PvsGraph'
    size, offset = int(stated.group(1)), int(stated.group(2))
    assert f'sizeof(PvsGraph) == {size} && offsetof(PvsGraph, n_norm_rows_dev) == {offset}' in header
    assert ctypes.sizeof(_lib.PvsGraph) == size == _lib.PVS_GRAPH_SIZEOF
    assert _lib.PvsGraph.n_norm_rows_dev.offset == offset == _lib.PVS_GRAPH_NORM_ROWS_OFFSET
    for name, n_args in (('pvs_graphnorm_stats_rows', 9), ('pvs_graphnorm_stats_rows_workspace_bytes', 2)):
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert name in _lib.EXPORTED_SYMBOLS and len(_lib._PROTOTYPES[name][1]) == n_args and hasattr(_lib.lib(), name)
    assert callable(PF.graphnorm_stats) and callable(PreparedGraph.set_norm_rows)


def test_the_screens_take_the_keyword_and_default_to_off():
    from pointvs_amd.screening import LibraryScreen, ScreeningSweep
    for cls in (LibraryScreen, ScreeningSweep):
        assert inspect.signature(cls.__init__).parameters['padded_graphnorm'].default is False
