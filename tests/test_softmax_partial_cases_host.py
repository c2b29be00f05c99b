"""Host-side pins of the softmax partial-first-layer references (tests/_softmax_partial_cases.py): the merge of the two
sets' softmax statistics IS the oracle layer on the union graph, the fp32 merge stays inside the strict bound the GPU
test (tests/test_gpu_softmax_partial_layer.py) applies, and the inputs tell a wrong merge from the right one by a wide
margin - all from the oracle alone. No GPU."""
import numpy as np
import pytest
import torch

from tests import _partial_cases as pc
from tests import _softmax_partial_cases as spc
from tests._golden import CaseLog

FLAG_NAMES = tuple(spc.flag_sets())
CELLS = [(f, 3, hid, 'base') for f in FLAG_NAMES for hid in (32, 64)] + \
        [('soft-full', 3, 128, 'base'), ('soft', 0, 32, 'base'), ('soft-full', 5, 64, 'base'), ('soft-full', 3, 32, 'partial')]


def test_exports_prototypes_and_keywords():
    """The two entries in the header, the library and the ctypes table (the partial entry: the arguments of
    pvs_egnn_layer_fwd_partial_att; the statistics entry: those of pvs_egnn_layer_edge_sums), and the opt-in keyword,
    off by default, on the three screening classes."""
    import inspect
    import re
    from pathlib import Path
    from pointvs_amd import _lib
    from pointvs_amd.screening import LibraryScreen, ReceptorScreen, ScreeningSweep
    header = (Path(__file__).resolve().parent.parent / 'include' / 'pvs_egnn.h').read_text()
    declared = set(re.findall(r'\b(pvs_[a-z0-9_]+)\s*\(', header))
    for name, twin in (('pvs_egnn_layer_edge_stats_softmax', 'pvs_egnn_layer_edge_sums'),
                       ('pvs_egnn_layer_fwd_partial_softmax', 'pvs_egnn_layer_fwd_partial_att')):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
        assert _lib._PROTOTYPES[name] == _lib._PROTOTYPES[twin]
    for cls in (ReceptorScreen, LibraryScreen, ScreeningSweep):
        assert inspect.signature(cls.__init__).parameters['softmax_reuse'].default is False


def test_flag_sets_are_softmax_layers_without_edge_residual():
    assert FLAG_NAMES == ('soft', 'soft-natt', 'soft-full', 'soft-nocoords')
    for name, flags in spc.flag_sets().items():
        assert flags['edge_attention'] and flags['softmax_attention'] and not flags.get('edge_residual')
    full = spc.flag_sets()['soft-full']
    assert all(full[k] for k in ('node_attention', 'normalize', 'tanh', 'graphnorm', 'gated_residual'))
    assert spc.flag_sets()['soft-nocoords']['update_coords'] is False


@pytest.mark.parametrize('flags,A,hid,ends', CELLS)
def test_fp64_merge_is_the_oracle_layer(flags, A, hid, ends):
    """stats(base) merged with stats(partial), then finish: h', x', node attention and the partial edges' attention of
    egnn_layer on the union graph, fp64, 1e-12; rows without a base edge have all-zero base rows."""
    p = spc.problem(A, hid, flags, ends)
    got = spc.merged_layer(p, torch.float64)
    assert set(got) == {'h_out', 'x_out', 'att'} | ({'natt'} if p.kw['node_attention'] else set())
    for key, value in got.items():
        ref = p.ref64[key]
        assert np.abs(value - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300), key
    rows = p.reference_base_rows()
    assert rows.shape == (p.case.n_nodes, hid + 4) and rows.dtype == np.float32
    no_base = np.flatnonzero(p.ref64['base_deg'] == 0)
    assert len(no_base) >= 30 and not rows[no_base].any() and not rows[:, hid + 2:].any()
    with_base = np.flatnonzero(p.ref64['base_deg'] > 0)
    assert (rows[with_base, hid + 1] >= 1).all(), 'a set with an edge has S >= 1'
    if not p.kw['update_coords']:
        assert np.array_equal(got['x_out'], p.case.pos.double().numpy())


@pytest.mark.parametrize('flags,A,hid,ends', CELLS)
def test_fp32_merge_holds_the_strict_bound_on_every_row_kind(flags, A, hid, ends):
    p = spc.problem(A, hid, flags, ends)
    log = CaseLog(f'host-softmax-{flags}-A{A}-H{hid}-{ends}')
    p.check(spc.merged_layer(p, torch.float32), log.case, log)
    log.finish()


def _moved(p, key, got, kinds):
    table = p.part_edges if key == 'att' else p.case.rows
    ratios = [float(np.abs(got[table[k]] - p.ref64[key][table[k]]).max()) / p.bound(key, table[k]) for k in kinds]
    ratios.append(float(np.abs(got - p.ref64[key]).max()) / p.bound(key))
    return min(ratios)


@pytest.mark.parametrize('flags,hid', [(f, hid) for f in FLAG_NAMES for hid in (32, 64, 128)])
def test_wrong_merges_are_far_outside_the_bound(flags, hid):
    """Each defect moves the fp64 result on the rows it concerns by more than 100 x the strict bound of those rows (and
    of the whole tensor):
      dropped base         h' on base-only and mixed rows
      partial attention    att left normalised over the partial set alone: the partial edges of mixed rows
      no shift             weights S_b, S_g without exp(mu_. - mu): h' on mixed rows
      sigmoid node gate    the node attention with the sigmoid that the reference replaces by Identity: every row
    The third defect reweights the two sets by exp(|mu_b - mu_g|), so what it moves is set by how far apart the two
    maxima lie, not by the layer: with _new_layer's att_mlp the gaps stay within about one unit (within half a unit at
    H = 64 and 128, where the initial weights are smaller), and the defect is held at the smallest gain of the wide
    variant, 6, where they are six times that; its figure at gain 1 is printed."""
    p = spc.problem(3, hid, flags)
    spread = spc.problem(3, hid, flags, 'base', spc.GAINS[-1])
    f64 = torch.float64
    figures = {
        'dropped base: h_out': _moved(p, 'h_out', spc.merged_layer(p, f64, drop_base=True)['h_out'], ('base', 'mixed')),
        'partial attention: att': _moved(p, 'att', spc.merged_layer(p, f64, partial_att=True)['att'], ('mixed',)),
        'no shift (gain 6): h_out': _moved(spread, 'h_out', spc.merged_layer(spread, f64, no_shift=True)['h_out'], ('mixed',)),
    }
    print('no shift at gain 1:', _moved(p, 'h_out', spc.merged_layer(p, f64, no_shift=True)['h_out'], ('mixed',)))
    if p.kw['node_attention']:
        figures['sigmoid node gate: natt'] = _moved(p, 'natt', spc.merged_layer(p, f64, sigmoid_node=True)['natt'], pc.KINDS)
    print(flags, hid, {k: f'{v:.0f}x' for k, v in figures.items()})
    assert all(v > 100 for v in figures.values()), figures


@pytest.mark.parametrize('flags,hid', [(f, 32) for f in FLAG_NAMES])
def test_wide_variant_spreads_the_maxima_and_underflows_one_side(flags, hid):
    """att_mlp.0.weight x 60 at H = 32 (att_mlp's initial weights shrink with the width: at H = 64 and 128 the same gain
    spreads the maxima by half as much): mu_b - mu_g passes +60 and -60 on the case's own mixed rows; the base weight of
    row dry[0] and the partial weight of row dry[1] are exactly 0 in fp32; the fp64 merge is still the oracle layer and
    the fp32 merge holds the bound."""
    p = spc.problem(3, hid, flags, 'base', 60)
    gap, mixed = p.gaps()
    base_dry, part_dry = p.case.dry
    assert {base_dry, part_dry} <= set(mixed) and base_dry != part_dry
    old = np.setdiff1d(mixed, [base_dry, part_dry])          # the mixed rows of the case itself
    assert gap[old].max() > 60 and gap[old].min() < -60, (gap[old].min(), gap[old].max())
    assert gap[base_dry] < -spc.UNDERFLOW and gap[part_dry] > spc.UNDERFLOW, (gap[base_dry], gap[part_dry])
    assert np.exp(np.float32(-abs(gap[base_dry]))) == 0 and np.exp(np.float32(-abs(gap[part_dry]))) == 0
    assert (np.diff(p.case.part_index[0].numpy()) >= 0).all(), 'the partial list is CSR-sorted'
    got = spc.merged_layer(p, torch.float64)
    for key, value in got.items():
        ref = p.ref64[key]
        assert np.abs(value - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1e-300), key
    part_row = p.case.part_index[0].numpy()
    assert p.ref64['att'][part_row == part_dry].max() < 1e-40 and p.ref64['att'][part_row == base_dry].min() == 1.0
    log = CaseLog(f'host-softmax-wide60-{flags}-H{hid}')
    p.check(spc.merged_layer(p, torch.float32), log.case, log)
    log.finish()
