"""The launch plan of a layer's backward (csrc/layer_plan.h: pvs_layer_bwd_plan), on the host (CPU).

The header is compiled alone with the host compiler, as tests/test_edge_dispatch.py compiles edge_dispatch.h, and prints
the plan for a product of facts: hidden size {16, 32, 64, 128} x the 2^9 combinations of the flags that the backward's host
path reads x 40 rows that cycle the 8 presences of m_prev / g_x_out / g_x, the class count {0, 3, 4}, an empty graph,
the gradient slots (all, or one of node_w2 / edge_w1 / node_att_w missing) and the pointer answers (all true, or one of
the nine false) - every value of every factor meets every flag combination and every hidden size - once per switch
setting (none, PVS_EGNN_SPLIT_SMALL, PVS_EGNN_SPLIT_WGRADS, PVS_EGNN_KERNELS=generic, PVS_EGNN_FIRST_LAYER_BWD=0).

The first test compares every field of every row with the rules that pvs_egnn_layer_bwd carried inline before it had a
plan, restated here in numpy from that source under its own names (chain_bwd, plain_out, prep_side, prep_done, ...). The
second asserts what wrong gradients come from: who clears, who initialises, who writes - each exactly once.
"""
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'pointvs_amd' / 'csrc'
CXX = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')

# the shape halves of the call site's answers, as dense_ops.hip has them: pvs_node_mlp_fused_supported and
# pvs_node_wgrads_supported take H = 32, 64; pvs_linear_epilogue_supported takes K % 32 == 0, C % 32 == 0, C <= 64 and
# K in {32, 64, 128} (the backward's products have one operand) - the pointer halves are the nine toggles
PROGRAM = r'''
#include "layer_plan.h"
#include <stdio.h>
static bool lin_shape(int K, int C) { return K % 32 == 0 && C % 32 == 0 && C <= 64 && (K == 32 || K == 64 || K == 128); }
int main() {
    const int Hs[] = {16, 32, 64, 128}, As[] = {0, 3, 4};
    const uint32_t bits[] = {PVS_RESIDUAL, PVS_EDGE_RESIDUAL, PVS_EDGE_ATTENTION, PVS_SOFTMAX_ATT, PVS_GRAPHNORM,
                             PVS_UPDATE_COORDS, PVS_NODE_ATTENTION, PVS_GATED_RESIDUAL, PVS_REZERO};
    for (int H : Hs)
        for (int fm = 0; fm < 512; ++fm)
            for (int j = 0; j < 40; ++j) {
                uint32_t F = 0;
                for (int b = 0; b < 9; ++b) if (fm & (1 << b)) F |= bits[b];
                const int pres = j % 8, off = j % 10, A = As[(j / 8) % 3], slots = (j / 10) % 4, no_edges = (j / 8) % 2;
                bool a[9];
                for (int k = 0; k < 9; ++k) a[k] = off != k + 1;
                PvsBwdFacts f;
                f.H = H; f.flags = F; f.n_attr = A;
                f.has_m_prev = pres & 1; f.has_g_x_out = pres & 2; f.has_g_x = pres & 4;
                f.no_edges = no_edges;
                f.gr_node_w2 = slots != 1; f.gr_edge_w1 = slots != 2; f.gr_node_att_w = slots != 3;
                f.gr_node_b2 = f.gr_node_w1 = f.gr_node_b1 = f.gr_edge_b1 = f.gr_node_att_b = f.gr_node_gate = true;
                f.wgrads_supported = H == 32 || H == 64;
                f.mlp_fused_ok = (H == 32 || H == 64) && a[0];
                f.chain_aligned = a[1];
                f.gu_epilogue_ok = lin_shape(H, H) && a[2];
                f.gu_passthrough_epilogue_ok = lin_shape(H, H) && a[3];
                f.gm_epilogue_ok = lin_shape(H, H) && a[4];
                f.both_epilogue_ok = lin_shape(H, 2 * H) && a[5];
                f.sy1_aligned = a[6]; f.gpq_aligned = a[7]; f.gh_gpq_aligned = a[8];
                f.sw = pvs_layer_switches();
                const PvsBwdPlan p = pvs_layer_bwd_plan(f);
                printf("%d %u %d %d %d %d %d  %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d "
                       "%d %d %d %d %d  %d\n",
                       H, (unsigned)F, A, pres, slots, off, no_edges,
                       (int)p.fam, (int)p.mfma_bwd, (int)p.first_layer, (int)p.coord_bwd, (int)p.soft_dots, (int)p.edge_res,
                       (int)p.node_out_bwd, (int)p.g_o_is_g_h_out, (int)p.gate_in_wgrads, (int)p.own_node_att_w,
                       (int)p.own_node_att_b, (int)p.own_node_gate, (int)p.fused_wgrads, (int)p.gu_product,
                       (int)p.fuse_tail_bwd, (int)p.tail_bwd1, (int)p.graphnorm, (int)p.gh_gm, (int)p.gh_accumulate,
                       (int)p.prep, (int)p.own_node_w2, (int)p.own_node_b2, (int)p.own_node_w1, (int)p.own_node_b1,
                       (int)p.own_edge_w1, (int)p.own_edge_b1, (int)p.node_b1_from_coefs, (int)p.slab_reduce,
                       (int)p.tail_folded, (int)p.gh_folded, p.has_att, (int)p.has_gate,
                       (int)pvs_first_layer_bwd(H, F, A, f.has_m_prev, f.has_g_x_out, f.has_g_x));
            }
    return 0;
}
'''
INPUTS = ['H', 'F', 'A', 'pres', 'slots', 'off', 'no_edges']
FIELDS = ['fam', 'mfma_bwd', 'first_layer', 'coord_bwd', 'soft_dots', 'edge_res', 'node_out_bwd', 'g_o_is_g_h_out',
          'gate_in_wgrads', 'own_node_att_w', 'own_node_att_b', 'own_node_gate', 'fused_wgrads', 'gu_product',
          'fuse_tail_bwd', 'tail_bwd1', 'graphnorm', 'gh_gm', 'gh_accumulate', 'prep', 'own_node_w2', 'own_node_b2',
          'own_node_w1', 'own_node_b1', 'own_edge_w1', 'own_edge_b1', 'node_b1_from_coefs', 'slab_reduce', 'tail_folded',
          'gh_folded', 'has_att', 'has_gate']
COLUMNS = INPUTS + FIELDS + ['first_layer_says']
GENERIC, SPLIT, EXACT, WIDE = range(4)                      # PvsEdgeFamily
GHGM_CHAIN, GHGM_ONE, GHGM_TWO = range(3)                   # PvsBwdGhGm
PREP_CHAIN, PREP_SIDE, PREP_OWN = range(3)                  # PvsBwdPrep
REDUCE_ONE_SET, REDUCE_TWO_SETS, REDUCE_FOLDED = range(3)   # PvsBwdSlabReduce
# include/pvs_egnn.h
RESIDUAL, EDGE_RESIDUAL, EDGE_ATTENTION, GRAPHNORM, UPDATE_COORDS = 1 << 0, 1 << 1, 1 << 2, 1 << 5, 1 << 6
NODE_ATTENTION, GATED_RESIDUAL, REZERO, SOFTMAX_ATT = 1 << 8, 1 << 9, 1 << 10, 1 << 11
FLAG_BITS = (RESIDUAL, EDGE_RESIDUAL, EDGE_ATTENTION, SOFTMAX_ATT, GRAPHNORM, UPDATE_COORDS, NODE_ATTENTION,
             GATED_RESIDUAL, REZERO)

SWITCHES = {
    'none': {},
    'split_small': {'PVS_EGNN_SPLIT_SMALL': '1'},
    'split_wgrads': {'PVS_EGNN_SPLIT_WGRADS': '1'},
    'generic': {'PVS_EGNN_KERNELS': 'generic'},
    'general_pair': {'PVS_EGNN_FIRST_LAYER_BWD': '0'},
}


@pytest.fixture(scope='module')
def tables(tmp_path_factory):
    """name of the switch setting -> {column: int array}, one run of the program each."""
    if CXX is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('layer_bwd_plan')
    (d / 'main.cpp').write_text(PROGRAM)
    exe = d / 'layer_bwd_plan_probe'
    out = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', str(CSRC), str(d / 'main.cpp'), '-o', str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    res = {}
    for name, env in SWITCHES.items():
        clean = {k: v for k, v in os.environ.items() if not k.startswith('PVS_')}
        clean.update(env)
        text = subprocess.run([str(exe)], capture_output=True, text=True, check=True, env=clean).stdout
        t = np.array(text.split(), dtype=np.int64).reshape(-1, len(COLUMNS))
        assert len(t) == 4 * 512 * 40
        res[name] = {c: t[:, i] for i, c in enumerate(COLUMNS)}
    return res


def test_the_product_covers_every_value_under_every_flag_combination(tables):
    t = tables['none']
    flags = sorted(sum(b for k, b in enumerate(FLAG_BITS) if fm & (1 << k)) for fm in range(512))
    assert sorted(set(t['F'].tolist())) == flags
    cell = t['H'] * (1 << 12) + t['F']
    assert len(set(cell.tolist())) == 4 * 512
    for column, values in (('A', (0, 3, 4)), ('pres', range(8)), ('slots', range(4)), ('off', range(10)), ('no_edges', (0, 1))):
        for v in values:
            assert len(set(cell[t[column] == v].tolist())) == 4 * 512, (column, v)


def parent_plan(t, env):
    """pvs_egnn_layer_bwd before the plan, rule for rule, over the columns of one table (numpy booleans)."""
    H, F, A = t['H'], t['F'], t['A']
    m_prev, g_x_out, g_x = (t['pres'] & 1) != 0, (t['pres'] & 2) != 0, (t['pres'] & 4) != 0
    E0 = t['no_edges'] != 0
    gr_node_w2, gr_edge_w1, gr_node_att_w = t['slots'] != 1, t['slots'] != 2, t['slots'] != 3
    gr_node_b2 = gr_node_w1 = gr_node_b1 = gr_edge_b1 = gr_node_att_b = gr_node_gate = np.ones_like(m_prev)
    a = [t['off'] != k + 1 for k in range(9)]
    h3264 = (H == 32) | (H == 64)

    def lin_shape(K, C):
        return (K % 32 == 0) & (C % 32 == 0) & (C <= 64) & ((K == 32) | (K == 64) | (K == 128))
    mlp_fused_supported = h3264 & a[0]                    # pvs_node_mlp_fused_supported(H, g_h_out, sy1, w.g_u, g_h)
    chain_pointers = a[1]                                 # (w.gM | w.gPQ | so | w.g_o | w.t1) & 15
    gu_supported_ws, gu_supported_pass = lin_shape(H, H) & a[2], lin_shape(H, H) & a[3]
    gm_supported, both_supported = lin_shape(H, H) & a[4], lin_shape(H, 2 * H) & a[5]
    sy1_16, gpq_16, gh_gpq_16 = a[6], a[7], a[8]
    split_small = np.full_like(m_prev, 'PVS_EGNN_SPLIT_SMALL' in env)
    split_wgrads = 'PVS_EGNN_SPLIT_WGRADS' in env

    def flag(b):
        return (F & b) != 0
    eatt, soft = flag(EDGE_ATTENTION), flag(SOFTMAX_ATT)
    eres = flag(EDGE_RESIDUAL) & m_prev
    gn, natt = flag(GRAPHNORM), flag(NODE_ATTENTION)
    gates = flag(RESIDUAL) & (flag(REZERO) | flag(GATED_RESIDUAL))
    coord_bwd = flag(UPDATE_COORDS) & g_x_out
    fused_wgrads = h3264 & gr_node_w2 & gr_node_w1 & gr_edge_w1 & (not split_wgrads)
    # pvs_edge_family(H, F, A, PVS_EDGE_BWD) without the BF16X3 switches
    generic = np.full_like(m_prev, env.get('PVS_EGNN_KERNELS', '')[:1] == 'g') | ~(h3264 | (H == 128)) | (A > 3)
    fam = np.where(generic, GENERIC, np.where(H == 128, WIDE, SPLIT))
    mfma_bwd = fam != GENERIC
    # pvs_first_layer_bwd(H, F, A, m_prev, g_x_out, g_x)
    first_layer = ((env.get('PVS_EGNN_FIRST_LAYER_BWD', '')[:1] != '0') & ~g_x & g_x_out & flag(UPDATE_COORDS) & (H == 32) &
                   (A <= 3) & (fam == SPLIT) & ~eatt & ~eres)
    chain_bwd = ~gn & ~gates & ~split_small & mlp_fused_supported & chain_pointers
    plain_out = ~flag(RESIDUAL) & ~natt & ~split_small
    g_o_is_g_h_out = plain_out | (chain_bwd & ~natt)
    node_out_launch = ~plain_out & ~chain_bwd
    gate_in_wgrads = natt & fused_wgrads & ~split_small & gr_node_att_w & gr_node_att_b
    fuse_tail_bwd = ~gn & np.where(g_o_is_g_h_out, gu_supported_pass, gu_supported_ws) & sy1_16
    prep_side = ~split_small & gpq_16 & gm_supported
    one_product = ~chain_bwd & (H == 32) & prep_side & both_supported
    prep_done = chain_bwd | one_product | prep_side
    tail_folded = mfma_bwd & fused_wgrads & ~split_small
    gate_grad = eres | (flag(EDGE_RESIDUAL) & E0)
    return {
        'fam': fam, 'mfma_bwd': mfma_bwd, 'first_layer': first_layer, 'coord_bwd': coord_bwd, 'soft_dots': eatt & soft,
        'edge_res': eres, 'node_out_bwd': node_out_launch, 'g_o_is_g_h_out': g_o_is_g_h_out,
        'gate_in_wgrads': gate_in_wgrads,
        'own_node_att_w': natt & ~gate_in_wgrads & gr_node_att_w, 'own_node_att_b': natt & ~gate_in_wgrads & gr_node_att_b,
        'own_node_gate': gates & gr_node_gate, 'fused_wgrads': fused_wgrads, 'gu_product': ~chain_bwd,
        'fuse_tail_bwd': fuse_tail_bwd, 'tail_bwd1': ~fuse_tail_bwd & ~chain_bwd, 'graphnorm': gn,
        'gh_gm': np.where(chain_bwd, GHGM_CHAIN, np.where(one_product, GHGM_ONE, GHGM_TWO)),
        'gh_accumulate': ~plain_out,
        'prep': np.where(chain_bwd, PREP_CHAIN, np.where(prep_done, PREP_SIDE, PREP_OWN)),
        'own_node_w2': gr_node_w2 & ~fused_wgrads, 'own_node_b2': gr_node_b2 & ~fused_wgrads,
        'own_node_w1': gr_node_w1 & ~fused_wgrads, 'own_node_b1': gr_node_b1 & ~fused_wgrads,
        'own_edge_w1': gr_edge_w1 & ~fused_wgrads, 'own_edge_b1': gr_edge_b1 & ~fused_wgrads,
        'node_b1_from_coefs': gn & gr_node_b1,
        'slab_reduce': np.where(~mfma_bwd, REDUCE_ONE_SET, np.where(tail_folded, REDUCE_FOLDED, REDUCE_TWO_SETS)),
        'tail_folded': tail_folded, 'gh_folded': tail_folded & gh_gpq_16,
        'has_att': np.where(eatt, np.where(soft, 2, 1), 0),
        'has_gate': gate_grad & (flag(REZERO) | flag(GATED_RESIDUAL)),
    }


@pytest.mark.parametrize('switch', list(SWITCHES))
def test_plan_matches_the_rules_the_backward_carried_inline(tables, switch):
    t = tables[switch]
    want = parent_plan(t, SWITCHES[switch])
    assert sorted(want) == sorted(FIELDS)
    for field in FIELDS:
        bad = np.flatnonzero(t[field] != want[field].astype(np.int64))
        assert bad.size == 0, (field, {c: int(t[c][bad[0]]) for c in COLUMNS}, int(want[field][bad[0]]))
    # every branch is reached somewhere in the product
    if switch == 'none':
        for field, n in (('gh_gm', 3), ('prep', 3), ('slab_reduce', 3), ('fam', 3), ('has_att', 3)):
            assert len(set(t[field].tolist())) == n, field
        assert set(t['first_layer'].tolist()) == {0, 1}


@pytest.mark.parametrize('switch', list(SWITCHES))
def test_each_buffer_has_exactly_one_producer(tables, switch):
    """From the plan's fields and what each step of layer_api.hip enqueues for them:
    the chain kernel (gh_gm = chain) always carries the row side jobs; the double-width product always carries them; the gM
    product of the two-product form carries them when prep = side job; pvs_prep_edge_bwd clears and scales when prep = own
    launch. The side jobs hold the clears under an MFMA family and gxagg under a coordinate gradient."""
    t = tables[switch]
    chain, one, two = (t['gh_gm'] == k for k in (GHGM_CHAIN, GHGM_ONE, GHGM_TWO))
    carriers = (chain.astype(int) + one.astype(int) + (two & (t['prep'] == PREP_SIDE)).astype(int) +
                (t['prep'] == PREP_OWN).astype(int))
    # the row half of gPQ and gx_row (MFMA families), gxagg (coordinate gradient): one launch; and always at most one
    assert np.all(carriers == 1)
    assert np.all((t['prep'] == PREP_CHAIN) == chain)
    # g_h: one launch initialises it, and it is the first that touches it - pvs_node_out_bwd (step 1), the chain kernel
    # (step 1) or a non-accumulating product (step 3); an accumulating product needs pvs_node_out_bwd before it; the
    # g_P / g_Q product of step 5 always accumulates
    product = one | two
    init = t['node_out_bwd'] + chain.astype(int) + (product & (t['gh_accumulate'] == 0)).astype(int)
    assert np.all(init == 1)
    assert np.all(t['node_out_bwd'][product & (t['gh_accumulate'] == 1)] == 1)
    assert np.all(t['gu_product'] == (~chain).astype(int))
    # g_y1 = g_u * SiLU'(y1) without GraphNorm: the chain kernel, the product's epilogue or pvs_node_tail_bwd1 - one of them
    no_gn = t['graphnorm'] == 0
    assert np.all((chain.astype(int) + ((~chain) & (t['fuse_tail_bwd'] == 1)).astype(int) + t['tail_bwd1'])[no_gn] == 1)
    assert np.all(t['tail_bwd1'][~no_gn & ~chain] == 1) and not np.any(chain & ~no_gn)
    # the slabs are reduced by one launch; folded only into a weight-gradient pass that runs
    assert np.all((t['slab_reduce'] == REDUCE_FOLDED) == (t['tail_folded'] == 1))
    assert np.all(t['fused_wgrads'][t['tail_folded'] == 1] == 1) and np.all(t['tail_folded'][t['gh_folded'] == 1] == 1)
    assert np.all((t['slab_reduce'] == REDUCE_ONE_SET) == (t['mfma_bwd'] == 0))
    # every present gradient slot has one writer among the weight-gradient launches: the fused pass or a launch of its
    # own (GraphNorm's closed form then REPLACES node_b1: node_b1_from_coefs, the last launch of the call); an absent
    # slot has none
    present = {'node_w2': t['slots'] != 1, 'edge_w1': t['slots'] != 2, 'node_att_w': t['slots'] != 3}
    everywhere = np.ones(len(t['H']), bool)
    for slot in ('node_w2', 'node_b2', 'node_w1', 'node_b1', 'edge_w1', 'edge_b1'):
        writers = t['own_' + slot] + t['fused_wgrads']
        # (the fused pass needs node_w2, node_w1 and edge_w1: without one of them every slot falls back to its own launch)
        assert np.all(writers[present.get(slot, everywhere)] == 1), slot
        assert np.all(t['own_' + slot][~present.get(slot, everywhere)] == 0), slot
    natt = (t['F'] & NODE_ATTENTION) != 0
    for slot in ('node_att_w', 'node_att_b'):
        writers = t['own_' + slot] + t['gate_in_wgrads']
        here = natt & present.get(slot, everywhere)
        assert np.all(writers[here] == 1) and np.all(t['own_' + slot][~here] == 0), slot
    assert np.all(t['fused_wgrads'][t['gate_in_wgrads'] == 1] == 1)
    assert np.all(present['node_att_w'][t['gate_in_wgrads'] == 1])
    gates = ((t['F'] & RESIDUAL) != 0) & ((t['F'] & (REZERO | GATED_RESIDUAL)) != 0)
    assert np.all(t['own_node_gate'] == gates.astype(int))
    # the first-layer pair exactly where pvs_first_layer_bwd says, and only in the split family - so the one gather call,
    # which passes the edge launcher's gx_row, passes the workspace's whenever the generic family runs
    assert np.all(t['first_layer'] == t['first_layer_says'])
    assert np.all(t['fam'][t['first_layer'] == 1] == SPLIT)
    if switch in ('generic', 'general_pair'):
        assert not np.any(t['first_layer'])


def test_edge_launcher_and_gather_share_one_gx_row():
    """gx_row == NULL is how both launchers of the first-layer pair are told: the backward names the workspace's gx_row
    once, where the plan's first_layer picks NULL instead, and the edge launcher's io and the gather both take that pick."""
    src = re.sub(r'//[^\n]*', '', (CSRC / 'layer_api.hip').read_text())       # (code only)
    assert len(re.findall(r'\bw\.gx_row\b', src)) == 1
    assert re.search(r'c\.gx_row = plan\.first_layer \? nullptr : w\.gx_row;', src)
    assert re.search(r'io\.gx_row = c\.gx_row;', src)
    assert re.search(r'pvs_launch_node_gather\(s, H, \*g, plan\.mfma_bwd, w\.gz1, w\.gd, c\.gx_row,', src)
    # and no step reads the environment or asks the selectors again
    steps = src[src.index('struct BwdCall {'):src.index('extern "C" int pvs_egnn_layer_bwd(')]
    assert steps.count('const PvsBwdPlan& plan') == 6 and not re.search(r'getenv|pvs_edge_family|pvs_first_layer_bwd|pvs_layer_switches', steps)
