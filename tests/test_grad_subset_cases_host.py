"""Host-side pins of the layer-call contract cells (tests/_grad_subset_cases.py): a GPU result of a cell is a finding only
while the cell reaches the launches it is there for. csrc/layer_plan.h is compiled alone with the host compiler, as
tests/test_layer_bwd_plan_host.py does, with a small program that reads one set of PvsBwdFacts per line and prints the
plan; every cell's facts go through it under the cell's switches. No GPU.

Pinned: the header's plan of every cell equals the table's restated one; what the union of cells at hidden 32 / 64
covers; `same_launches_as_full` from the header's plans; the launch counts of the cells that the issue names.

Mutations (each applied to a copy of the header / judged from layer_api.hip; none of them survives):
  own_edge_w1's second product ignoring m.perm (layer_api.hip, bwd_weight_tail: `false` for `m.perm`)
      no plan field changes - the five GPU cells *-perm-all-split_wgrads (N = 33 / 513 at H = 32 / 64, and A = 5) fail their
      accuracy check (seen on a scratch build): the second product overwrites the first one's columns of
      edge_mlp.0.weight.grad instead of adding to them
  gate_in_wgrads not requiring both node-attention slots (layer_plan.h)
      test_header_plan_equals_the_table fails at natt-*-no-node_att_w (gate_in_wgrads 1 != 0); on the GPU that cell's
      route check fails (no column sum of its own for node_att_b)
  prep left as SIDE_JOB when gm_epilogue_ok is false (layer_plan.h)
      test_header_plan_equals_the_table fails at base-N33-H16-full-all (prep 1 != 2); on the GPU the hidden 16 / 128 cells
      raise from pvs_launch_linear ("the extras need the MFMA path")
test_the_plan_probe_bites applies the two header mutations and checks that the comparison does fail at those cells.
"""
import os
import shutil
import subprocess
from pathlib import Path

import pytest

from tests import _grad_subset_cases as gsc

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'pointvs_amd' / 'csrc'
CXX = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')

PROGRAM = r'''
#include "layer_plan.h"
#include <stdio.h>
int main() {
    int v[26];
    for (;;) {
        for (int k = 0; k < 26; ++k) if (scanf("%d", &v[k]) != 1) return 0;
        PvsBwdFacts f;
        int k = 0;
        f.H = v[k++]; f.flags = (uint32_t)v[k++]; f.n_attr = v[k++];
        f.has_m_prev = v[k++]; f.has_g_x_out = v[k++]; f.has_g_x = v[k++]; f.no_edges = v[k++];
        f.gr_node_w2 = v[k++]; f.gr_node_b2 = v[k++]; f.gr_node_w1 = v[k++]; f.gr_node_b1 = v[k++];
        f.gr_edge_w1 = v[k++]; f.gr_edge_b1 = v[k++]; f.gr_node_att_w = v[k++]; f.gr_node_att_b = v[k++];
        f.gr_node_gate = v[k++];
        f.wgrads_supported = v[k++]; f.mlp_fused_ok = v[k++]; f.chain_aligned = v[k++]; f.gu_epilogue_ok = v[k++];
        f.gu_passthrough_epilogue_ok = v[k++]; f.gm_epilogue_ok = v[k++]; f.both_epilogue_ok = v[k++];
        f.sy1_aligned = v[k++]; f.gpq_aligned = v[k++]; f.gh_gpq_aligned = v[k++];
        f.sw = pvs_layer_switches();
        const PvsBwdPlan p = pvs_layer_bwd_plan(f);
        printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d\n",
               (int)p.fam, (int)p.mfma_bwd, (int)p.first_layer, (int)p.coord_bwd, (int)p.soft_dots, (int)p.edge_res,
               (int)p.node_out_bwd, (int)p.g_o_is_g_h_out, (int)p.gate_in_wgrads, (int)p.own_node_att_w,
               (int)p.own_node_att_b, (int)p.own_node_gate, (int)p.fused_wgrads, (int)p.gu_product,
               (int)p.fuse_tail_bwd, (int)p.tail_bwd1, (int)p.graphnorm, (int)p.gh_gm, (int)p.gh_accumulate,
               (int)p.prep, (int)p.own_node_w2, (int)p.own_node_b2, (int)p.own_node_w1, (int)p.own_node_b1,
               (int)p.own_edge_w1, (int)p.own_edge_b1, (int)p.node_b1_from_coefs, (int)p.slab_reduce,
               (int)p.tail_folded, (int)p.gh_folded, p.has_att, (int)p.has_gate);
    }
}
'''
F32 = [c for c in gsc.CELLS if c['dtype'] == 'f32']


def _build(d, header_text=None):
    """The probe over csrc/layer_plan.h, or over `header_text` in its place (edge_dispatch.h still from csrc)."""
    (d / 'main.cpp').write_text(PROGRAM)
    include = ['-I', str(CSRC)]
    if header_text is not None:
        (d / 'layer_plan.h').write_text(header_text)
        include = ['-I', str(d)] + include
    exe = d / 'plan_probe'
    out = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror'] + include + [str(d / 'main.cpp'), '-o', str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return exe


def _plans(exe):
    """tag -> {plan field: int} from the header, one run of the probe per distinct switch setting."""
    res = {}
    for env in {tuple(sorted(c['env'].items())) for c in F32}:
        cells = [c for c in F32 if tuple(sorted(c['env'].items())) == env]
        lines = [' '.join(str(int(gsc.facts_for(c)[k])) for k in gsc.FACT_FIELDS) for c in cells]
        clean = {k: v for k, v in os.environ.items() if not k.startswith('PVS_')}
        clean.update(dict(env))
        text = subprocess.run([str(exe)], input='\n'.join(lines) + '\n', capture_output=True, text=True, check=True,
                              env=clean).stdout
        rows = [list(map(int, line.split())) for line in text.splitlines()]
        assert len(rows) == len(cells) and all(len(r) == len(gsc.PLAN_FIELDS) for r in rows)
        for c, row in zip(cells, rows):
            res[c['tag']] = dict(zip(gsc.PLAN_FIELDS, row))
    return res


def _mismatches(plans):
    return [(c['tag'], k, plans[c['tag']][k], want[k]) for c in F32 for want in [gsc.plan_for(c)]
            for k in gsc.PLAN_FIELDS if plans[c['tag']][k] != want[k]]


@pytest.fixture(scope='module')
def plans(tmp_path_factory):
    if CXX is None:
        pytest.skip('no host C++ compiler')
    return _plans(_build(tmp_path_factory.mktemp('grad_subset_plan')))


def test_flag_sets_are_those_of_the_layer_tests():
    from tests.test_gpu_edge_classes import FLAGS
    plan_keys = {name for name, _, _ in gsc._BITS}
    for name, kw in gsc.FLAG_KW.items():
        assert {k: v for k, v in FLAGS[name].items() if k in plan_keys} == kw, name
    assert gsc.layer_flags('plain') == 1 | 1 << 6                             # residual, update_coords
    assert gsc.layer_flags('perm') == 1 | 1 << 6 | 1 << 7
    assert gsc.layer_flags('full') == 1 | 2 | 4 | 8 | 16 | 32 | 64 | 1 << 8 | 1 << 9
    assert gsc.live_slots('plain') == ('edge_w1', 'edge_b1', 'edge_w2', 'edge_b2', 'coord_w1', 'coord_b1', 'coord_w2',
                                       'node_w1', 'node_b1', 'node_w2', 'node_b2')
    assert gsc.live_slots('full') == gsc.PARAM_FIELDS
    assert gsc.live_slots('gated+') == gsc.live_slots('plain') + ('node_gate',)


def test_the_cells_are_the_ones_asked_for():
    tags = set(gsc.BY_TAG)
    for hid in (32, 64):
        for n in (33, 513):
            for flags in gsc.FLAG_KW:
                assert f'base-N{n}-H{hid}-{flags}-all' in tags
            for want in ('bias-N{n}-H{hid}-plain-no-node_b2+node_b1+edge_b1', 'unfused-N{n}-H{hid}-full-no-node_w2',
                         'unfused-N{n}-H{hid}-natt-tanh-no-node_w1', 'unfused-N{n}-H{hid}-plain-no-edge_w1',
                         'unfused-N{n}-H{hid}-perm-no-edge_w1', 'natt-N{n}-H{hid}-natt-tanh-no-node_att_w',
                         'natt-N{n}-H{hid}-natt-tanh-no-node_att_b', 'gate-N{n}-H{hid}-gated+-no-node_gate',
                         'gn-N{n}-H{hid}-gn-no-gn_weight', 'gn-N{n}-H{hid}-gn-no-gn_bias', 'gn-N{n}-H{hid}-gn-no-gn_mean_scale',
                         'inputs-N{n}-H{hid}-full-none', 'inputs-N{n}-H{hid}-plain-none',
                         'switch-N{n}-H{hid}-plain-all-split_wgrads', 'switch-N{n}-H{hid}-full-all-split_wgrads',
                         'switch-N{n}-H{hid}-perm-all-split_wgrads'):
                assert want.format(n=n, hid=hid) in tags, want.format(n=n, hid=hid)
            for slot in ('edge_w2', 'edge_b2', 'att_w', 'att_b', 'coord_w1', 'coord_b1', 'coord_w2', 'edge_gate'):
                assert f'edge-N{n}-H{hid}-full-no-{slot}' in tags
            for flags in ('plain', 'natt-tanh', 'full'):
                for names in (('g_h_out',), ('g_h',), ('saved',), ('h', 'h_out'), ('h', 'h_out', 'saved', 'g_h_out', 'g_h')):
                    assert f'offset-N{n}-H{hid}-{flags}-all-off-' + '+'.join(names) in tags
    assert 'base-N96-H32-perm-all-split_wgrads-A5' in tags
    for hid in (16, 128):
        assert {f'unfused-N33-H{hid}-full-no-node_w2', f'inputs-N33-H{hid}-full-none'} <= tags
    assert {'unfused-N33-H32-full-no-node_w2-f64', 'inputs-N33-H32-full-none-f64'} <= tags
    for c in gsc.CELLS:
        assert gsc.baseline_of(c) is not None, c['tag']
        assert c['n'] in (33, 513, 96) and c['n'] <= 513
        if c['skip'] == gsc.ALL:
            assert gsc.requested(c) == ()
        else:
            assert set(gsc.requested(c)) == set(gsc.live_slots(c['flags'])) - set(c['skip'])


def test_header_plan_equals_the_table(plans):
    assert _mismatches(plans) == []


def test_the_union_of_cells_covers_what_the_gpu_suite_never_ran(plans):
    rows = [(c, plans[c['tag']], gsc.facts_for(c)) for c in F32 if c['hid'] in (32, 64)]

    def some(pred):
        return any(pred(c, p, f) for c, p, f in rows)
    for field in gsc.PLAN_FIELDS:
        if field.startswith('own_'):
            assert some(lambda c, p, f: p[field] == 1), field
    assert some(lambda c, p, f: p['fused_wgrads'] and not (f['gr_node_b2'] and f['gr_node_b1'] and f['gr_edge_b1']))
    natt = gsc._lib.NODE_ATTENTION
    assert some(lambda c, p, f: f['flags'] & natt and p['fused_wgrads'] and not p['gate_in_wgrads'])
    assert some(lambda c, p, f: p['slab_reduce'] == gsc.REDUCE_TWO_SETS and p['mfma_bwd'])
    assert {p['gh_folded'] for c, p, f in rows if p['tail_folded']} == {0, 1}
    assert {p['gh_gm'] for c, p, f in rows} == {gsc.GHGM_CHAIN, gsc.GHGM_ONE, gsc.GHGM_TWO}
    assert {p['gh_gm'] for c, p, f in rows if c['hid'] == 64} == {gsc.GHGM_CHAIN, gsc.GHGM_TWO}
    assert some(lambda c, p, f: c['hid'] == 32 and p['gh_gm'] == gsc.GHGM_ONE)
    assert {p['prep'] for c, p, f in rows} == {gsc.PREP_CHAIN, gsc.PREP_SIDE, gsc.PREP_OWN}
    assert some(lambda c, p, f: p['tail_bwd1'] and not p['graphnorm'])
    assert {p['fuse_tail_bwd'] for c, p, f in rows if p['gu_product']} == {0, 1}
    gn_slots = ('gn_weight', 'gn_bias', 'gn_mean_scale')
    with_gn = {all(s in gsc.requested(c) for s in gn_slots) for c, p, f in rows if p['node_b1_from_coefs']}
    assert with_gn == {False, True}
    assert some(lambda c, p, f: p['node_b1_from_coefs'] and not any(s in gsc.requested(c) for s in gn_slots))
    # the unfused products at the layer's own strides: with accumulation (perm), and on rows that start on no 16 bytes
    perm = gsc._lib.PERM_INVARIANT
    assert some(lambda c, p, f: p['own_edge_w1'] and f['flags'] & perm and c['A'] == 3)
    assert some(lambda c, p, f: p['own_edge_w1'] and f['flags'] & perm and c['A'] == 5 and p['fam'] == gsc.GENERIC)
    # the other widths never fuse, never fold
    for c in F32:
        if c['hid'] in (16, 128):
            p = plans[c['tag']]
            assert not p['fused_wgrads'] and p['gh_gm'] == gsc.GHGM_TWO and p['prep'] == gsc.PREP_OWN, c['tag']


def test_same_launches_as_full_follows_the_header(plans):
    n_same = 0
    for c in F32:
        base = gsc.baseline_of(c)
        want = (base is not c and not gsc.FORWARD_OFFSETS & set(c['offsets'])
                and gsc.same_launches(plans[c['tag']], plans[base['tag']]))
        assert gsc.same_launches_as_full(c) == want, c['tag']
        n_same += want
    by_group = {}
    for c in gsc.CELLS:
        by_group.setdefault(c['group'], set()).add(gsc.same_launches_as_full(c))
    # skipping a bias, a GraphNorm slot, the residual gate or an edge-side slot changes no launch; skipping a weight of the
    # fused pass, one of the node gate's two slots or everything does. An offset on h, h_out or saved moves the forward;
    # on g_h_out or g_h the plan moves unless the flag set takes none of the launches they gate (`full` with g_h_out off:
    # pvs_node_out_bwd reads it element by element)
    assert by_group['bias'] == by_group['gate'] == by_group['gn'] == by_group['edge'] == {True}
    assert by_group['natt'] == {False} and by_group['base'] == {False}
    same_offsets = {c['tag'] for c in gsc.CELLS if c['group'] == 'offset' and gsc.same_launches_as_full(c)}
    assert same_offsets == {f'offset-N{n}-H{hid}-full-all-off-g_h_out' for n in (33, 513) for hid in (32, 64)}
    assert by_group['unfused'] == {False, True} and by_group['inputs'] == {False, True}       # (True: hidden 16 / 128, fp64)
    assert n_same >= 60


def test_launch_counts_of_the_named_cells():
    def routes(tag):
        return gsc.routes_for(gsc.BY_TAG[tag])
    for hid in (32, 64):
        r = routes(f'unfused-N33-H{hid}-full-no-node_w2')
        assert 'node_wgrads' not in r and r['tsgemm_mfma'] == 4
        r = routes(f'switch-N513-H{hid}-full-all-split_wgrads')
        assert 'node_wgrads' not in r and r['tsgemm_mfma'] == 5
        # three biases, node gate weight, residual gate, S1, S2 on four columns at a time; the node gate's bias alone
        assert r['colreduce4'] == 7 and r['colreduce'] == 1
        r = routes(f'inputs-N33-H{hid}-plain-none')
        assert r == {'node_mlp_bwd': 1, 'linear_mfma': 1}
        for names in ('g_h', 'g_h_out', 'saved', 'h+h_out+saved+g_h_out+g_h'):
            assert 'node_mlp_bwd' not in routes(f'offset-N33-H{hid}-plain-all-off-{names}'), names
        assert routes(f'offset-N33-H{hid}-plain-all-off-h+h_out') == routes(f'base-N33-H{hid}-plain-all')
        assert routes(f'offset-N33-H{hid}-plain-all-off-g_h')['linear_generic'] == 2
    assert routes('base-N33-H32-plain-all') == {'node_mlp_bwd': 1, 'node_wgrads': 1}
    assert routes('base-N33-H64-plain-all') == {'node_mlp_bwd': 1, 'node_wgrads': 1, 'linear_mfma': 1}
    assert routes('base-N33-H32-full-all') == {'node_out_bwd': 1, 'node_tail': 2, 'node_wgrads': 1, 'linear_mfma': 2,
                                               'colreduce4': 3}
    assert not gsc.forward_chain(gsc.BY_TAG['offset-N33-H32-plain-all-off-h+h_out'])
    assert gsc.forward_chain(gsc.BY_TAG['offset-N33-H32-plain-all-off-g_h'])
    assert not gsc.forward_chain(gsc.BY_TAG['base-N33-H32-full-all'])


MUTATIONS = {
    'gate_in_wgrads': ('p.gate_in_wgrads = natt && p.fused_wgrads && !split_small && f.gr_node_att_w && f.gr_node_att_b;',
                       'p.gate_in_wgrads = natt && p.fused_wgrads && !split_small;',
                       'natt-N33-H32-natt-tanh-no-node_att_w', 'gate_in_wgrads'),
    'prep': ('p.prep = prep_side ? PVS_BWD_PREP_SIDE_JOB : PVS_BWD_PREP_OWN_LAUNCH;',
             'p.prep = PVS_BWD_PREP_SIDE_JOB;', 'base-N33-H16-full-all', 'prep'),
}


@pytest.mark.parametrize('name', sorted(MUTATIONS))
def test_the_plan_probe_bites(name, tmp_path):
    if CXX is None:
        pytest.skip('no host C++ compiler')
    old, new, tag, field = MUTATIONS[name]
    text = (CSRC / 'layer_plan.h').read_text()
    assert text.count(old) == 1
    bad = _mismatches(_plans(_build(tmp_path, text.replace(old, new))))
    assert (tag, field) in {(t, k) for t, k, _, _ in bad}, bad[:5]
