"""Cells of the layer-call contract tests (tests/test_gpu_layer_call_contract.py; pinned on the host by
tests/test_grad_subset_cases_host.py): one layer backward through the C entry with some gradient slots NULL, some
caller tensors 4 bytes off a 16-byte boundary, or a layer-level switch set.

pvs_egnn_layer_bwd picks its launches in csrc/layer_plan.h from three kinds of facts: flags and width, which members of
PvsLayerGrads are non-NULL, and which caller pointers sit on 16 bytes. A cell is (n, hid, flags, skip, offsets, env) and
this module states, per cell and WITHOUT the library,

  facts_for(cell)       the PvsBwdFacts that the call site (layer_api.hip: pvs_egnn_layer_bwd) forms for it
  expected_plan(facts)  the plan, restated rule for rule in Python (the host test compares it with the header's own)
  routes_for(cell)      launches of the backward per measurement-hook group, as the steps of layer_api.hip enqueue them
  forward_chain(cell)   whether the forward takes the folded chain k_node_mlp_fwd
  same_launches_as_full(cell)
                        the plan equals the all-slots, aligned plan of the same (n, hid, flags, env) in every field but
                        those that only drop a write: skipping must then change no bit of anything else

Node counts: 33 (one row into the second MFMA tile) and 513 (second tsgemm block: two slabs to reduce), the graphs of
tests/_node_count_cases.py; one cell on the 5-class graph of tests/_edge_class_cases.py (ld1 no multiple of 4).
"""
from pointvs_amd import _lib

PARAM_FIELDS = _lib.PARAM_FIELDS
ALL = 'ALL'                                 # skip: every slot NULL (input gradients only)
BIASES = ('node_b2', 'node_b1', 'edge_b1')
COORD_MLP = ('coord_w1', 'coord_b1', 'coord_w2')
OFFSET_NAMES = ('h', 'h_out', 'saved', 'g_h_out', 'g_h')
OFFSET_SETS = (('g_h_out',), ('g_h',), ('saved',), ('h', 'h_out'), OFFSET_NAMES)
SPLIT_WGRADS = {'PVS_EGNN_SPLIT_WGRADS': '1'}
SPLIT_SMALL = {'PVS_EGNN_SPLIT_SMALL': '1'}

# the flag sets of tests/test_gpu_edge_classes.py FLAGS that the cells use, as EGNNLayer keyword arguments that matter to
# the plan (the host test compares them with FLAGS itself)
FLAG_KW = {
    'plain': dict(),
    'full': dict(edge_residual=True, gated_residual=True, residual=True, edge_attention=True, node_attention=True,
                 normalize=True, tanh=True, graphnorm=True),
    'perm': dict(permutation_invariance=True),
    'gn': dict(graphnorm=True),
    'natt-tanh': dict(node_attention=True),
    'gated+': dict(residual=True, gated_residual=True),
}
_BITS = (('residual', _lib.RESIDUAL, True), ('edge_residual', _lib.EDGE_RESIDUAL, False),
         ('edge_attention', _lib.EDGE_ATTENTION, False), ('normalize', _lib.NORMALIZE, False), ('tanh', _lib.TANH, False),
         ('graphnorm', _lib.GRAPHNORM, False), ('update_coords', _lib.UPDATE_COORDS, True),
         ('permutation_invariance', _lib.PERM_INVARIANT, False), ('node_attention', _lib.NODE_ATTENTION, False),
         ('gated_residual', _lib.GATED_RESIDUAL, False), ('rezero', _lib.REZERO, False),
         ('softmax_attention', _lib.SOFTMAX_ATT, False))


def layer_flags(flags):
    """EGNNLayer._flags() of a layer built with FLAG_KW[flags]."""
    kw = FLAG_KW[flags]
    return sum(bit for name, bit, default in _BITS if kw.get(name, default))


def live_slots(flags):
    """The slots of PARAM_FIELDS that _EGNNLayerFn.backward fills for this flag set when a coordinate gradient and the
    messages of a layer before arrive (what the tests' loss makes so): the layer's parameters minus `dead_grads`."""
    F = layer_flags(flags)
    gates = bool(F & (_lib.REZERO | _lib.GATED_RESIDUAL))
    has = {'att_w': F & _lib.EDGE_ATTENTION, 'att_b': F & _lib.EDGE_ATTENTION, 'gn_weight': F & _lib.GRAPHNORM,
           'gn_bias': F & _lib.GRAPHNORM, 'gn_mean_scale': F & _lib.GRAPHNORM, 'node_att_w': F & _lib.NODE_ATTENTION,
           'node_att_b': F & _lib.NODE_ATTENTION, 'edge_gate': gates and F & _lib.EDGE_RESIDUAL,
           'node_gate': gates and F & _lib.RESIDUAL}
    return tuple(name for name in PARAM_FIELDS if has.get(name, True))


def requested(cell):
    live = live_slots(cell['flags'])
    if cell['skip'] == ALL:
        return ()
    assert set(cell['skip']) <= set(live), (cell['tag'], cell['skip'])
    return tuple(name for name in live if name not in cell['skip'])


def _cell(group, n, hid, flags, skip=(), offsets=(), env=None, dtype='f32', A=3, twice=False):
    env = dict(env or {})
    skip_tag = 'all' if not skip else ('none' if skip == ALL else 'no-' + '+'.join(skip))
    tag = f'{group}-N{n}-H{hid}-{flags}-{skip_tag}'
    if offsets:
        tag += '-off-' + '+'.join(offsets)
    if env:
        tag += '-' + '-'.join(k.replace('PVS_EGNN_', '').lower() for k in env)
    if dtype != 'f32':
        tag += '-' + dtype
    if A != 3:
        tag += f'-A{A}'
    return dict(group=group, n=n, hid=hid, flags=flags, skip=skip if skip == ALL else tuple(skip), offsets=tuple(offsets),
                env=env, dtype=dtype, A=A, twice=twice, tag=tag)


NODE_N = (33, 513)
CLASS_GRAPH_N = 96                          # tests/_edge_class_cases.py: class_graph


def _cells():
    out = []
    for hid in (32, 64):
        for n in NODE_N:
            # every slot: the baseline of each flag set
            out += [_cell('base', n, hid, flags) for flags in FLAG_KW]
            # the three biases missing: the fused pass stays
            out += [_cell('bias', n, hid, flags, BIASES) for flags in ('plain', 'full')]
            # one weight missing: everything unfused
            out.append(_cell('unfused', n, hid, 'full', ('node_w2',), twice=True))
            out.append(_cell('unfused', n, hid, 'natt-tanh', ('node_w1',), twice=True))
            out += [_cell('unfused', n, hid, flags, ('edge_w1',), twice=True) for flags in ('plain', 'perm')]
            # one of the node gate's two slots beside the fused pass
            for slot in ('node_att_w', 'node_att_b'):
                out += [_cell('natt', n, hid, flags, (slot,)) for flags in ('natt-tanh', 'full')]
            out += [_cell('gate', n, hid, flags, ('node_gate',)) for flags in ('gated+', 'full')]
            out += [_cell('gn', n, hid, 'gn', (slot,)) for slot in ('gn_weight', 'gn_bias', 'gn_mean_scale')]
            out.append(_cell('gn', n, hid, 'full', ('gn_weight', 'gn_bias', 'gn_mean_scale')))
            # each edge-side slot
            for slot in ('edge_w2', 'edge_b2', 'att_w', 'att_b') + COORD_MLP + ('edge_gate',):
                out.append(_cell('edge', n, hid, 'full', (slot,)))
            # input gradients only
            out += [_cell('inputs', n, hid, flags, ALL, twice=True) for flags in ('plain', 'natt-tanh', 'full')]
            # PVS_EGNN_SPLIT_WGRADS with every slot
            out += [_cell('switch', n, hid, flags, env=SPLIT_WGRADS, twice=True) for flags in ('plain', 'full', 'perm')]
            # 4 bytes off
            for flags in ('plain', 'natt-tanh', 'full'):
                out += [_cell('offset', n, hid, flags, offsets=names, twice=True) for names in OFFSET_SETS]
        # every folded node-level launch apart: the only way to PVS_BWD_PREP_OWN_LAUNCH at these widths
        out += [_cell('switch', 33, hid, flags, env=SPLIT_SMALL) for flags in ('plain', 'full')]
    # ld1 = H + 1 + 5: the unfused edge_mlp.0 products write rows that start on no 16 bytes; generic edge backward
    out += [_cell('base', CLASS_GRAPH_N, 32, 'perm', env=SPLIT_WGRADS, A=5)]
    # the other widths (no fused pass, no folded chain)
    for hid in (16, 128):
        out += [_cell('base', 33, hid, 'full'), _cell('unfused', 33, hid, 'full', ('node_w2',)),
                _cell('inputs', 33, hid, 'full', ALL)]
    # fp64
    out += [_cell('base', 33, 32, 'full', dtype='f64'), _cell('unfused', 33, 32, 'full', ('node_w2',), dtype='f64'),
            _cell('inputs', 33, 32, 'full', ALL, dtype='f64')]
    return out


CELLS = _cells()
BY_TAG = {c['tag']: c for c in CELLS}
assert len(BY_TAG) == len(CELLS)


def baseline_of(cell):
    """The all-slots, aligned cell of the same (n, hid, flags, env, dtype, A)."""
    want = (cell['n'], cell['hid'], cell['flags'], cell['env'], cell['dtype'], cell['A'])
    for c in CELLS:
        if not c['skip'] and not c['offsets'] and (c['n'], c['hid'], c['flags'], c['env'], c['dtype'], c['A']) == want:
            return c
    return None


# ---- the facts of the call site ------------------------------------------------------------------------------------------
FACT_FIELDS = ('H', 'flags', 'n_attr', 'has_m_prev', 'has_g_x_out', 'has_g_x', 'no_edges', 'gr_node_w2', 'gr_node_b2',
               'gr_node_w1', 'gr_node_b1', 'gr_edge_w1', 'gr_edge_b1', 'gr_node_att_w', 'gr_node_att_b', 'gr_node_gate',
               'wgrads_supported', 'mlp_fused_ok', 'chain_aligned', 'gu_epilogue_ok', 'gu_passthrough_epilogue_ok',
               'gm_epilogue_ok', 'both_epilogue_ok', 'sy1_aligned', 'gpq_aligned', 'gh_gpq_aligned')


def _lin_shape(K, C):
    """The shape half of pvs_linear_epilogue_supported (dense_ops.hip) for a product with one operand."""
    return K % 32 == 0 and C % 32 == 0 and C <= 64 and K in (32, 64, 128)


def facts_for(cell):
    """layer_api.hip:900-917 for the call tests/_layer_call.py makes: m_prev where the layer has an edge residual, a
    coordinate gradient in and out, a graph with edges, the workspace as the allocator gives it (256-byte pieces). The
    pointer answers: every saved piece (y1, o, ...) starts a multiple of 16 bytes behind `saved`."""
    H, F = cell['hid'], layer_flags(cell['flags'])
    got = set(requested(cell))
    on16 = {name: name not in cell['offsets'] for name in OFFSET_NAMES}
    wide = H in (32, 64)
    f = dict(H=H, flags=F, n_attr=cell['A'], has_m_prev=bool(F & _lib.EDGE_RESIDUAL), has_g_x_out=True, has_g_x=True,
             no_edges=False)
    for slot in ('node_w2', 'node_b2', 'node_w1', 'node_b1', 'edge_w1', 'edge_b1', 'node_att_w', 'node_att_b', 'node_gate'):
        f['gr_' + slot] = slot in got
    f.update(
        wgrads_supported=wide,
        mlp_fused_ok=wide and on16['g_h_out'] and on16['saved'] and on16['g_h'],    # (g_h_out, saved y1, w.g_u, g_h)
        chain_aligned=on16['saved'],                                                # (gM | gPQ | saved o | g_o | t1)
        gu_epilogue_ok=_lin_shape(H, H),                                            # (y = w.g_u, x = w.g_o)
        gu_passthrough_epilogue_ok=_lin_shape(H, H) and on16['g_h_out'],            # (x = g_h_out)
        gm_epilogue_ok=_lin_shape(H, H),                                            # (y = w.gM, x = w.g_u)
        both_epilogue_ok=_lin_shape(H, 2 * H) and on16['g_h'],                      # (y = g_h, 2 H outputs)
        sy1_aligned=on16['saved'], gpq_aligned=True, gh_gpq_aligned=on16['g_h'])
    return f


# ---- the plan, restated ----------------------------------------------------------------------------------------------------
GENERIC, SPLIT, EXACT, WIDE = range(4)                      # PvsEdgeFamily
GHGM_CHAIN, GHGM_ONE, GHGM_TWO = range(3)                   # PvsBwdGhGm
PREP_CHAIN, PREP_SIDE, PREP_OWN = range(3)                  # PvsBwdPrep
REDUCE_ONE_SET, REDUCE_TWO_SETS, REDUCE_FOLDED = range(3)   # PvsBwdSlabReduce
PLAN_FIELDS = ('fam', 'mfma_bwd', 'first_layer', 'coord_bwd', 'soft_dots', 'edge_res', 'node_out_bwd', 'g_o_is_g_h_out',
               'gate_in_wgrads', 'own_node_att_w', 'own_node_att_b', 'own_node_gate', 'fused_wgrads', 'gu_product',
               'fuse_tail_bwd', 'tail_bwd1', 'graphnorm', 'gh_gm', 'gh_accumulate', 'prep', 'own_node_w2', 'own_node_b2',
               'own_node_w1', 'own_node_b1', 'own_edge_w1', 'own_edge_b1', 'node_b1_from_coefs', 'slab_reduce',
               'tail_folded', 'gh_folded', 'has_att', 'has_gate')
# fields that only say whether a gradient is WRITTEN by a launch of its own / a copy: with the rest of the plan equal,
# dropping one drops that write and nothing else
WRITE_ONLY_FIELDS = ('own_node_att_w', 'own_node_att_b', 'own_node_gate', 'own_node_w2', 'own_node_b2', 'own_node_w1',
                     'own_node_b1', 'own_edge_w1', 'own_edge_b1', 'node_b1_from_coefs')


def expected_plan(f, env):
    """pvs_layer_bwd_plan over one set of facts, for the switches this module's cells set (no family switch)."""
    H, F, A = f['H'], f['flags'], f['n_attr']

    def flag(bit):
        return bool(F & bit)
    split_small, split_wgrads = 'PVS_EGNN_SPLIT_SMALL' in env, 'PVS_EGNN_SPLIT_WGRADS' in env
    gn, natt = flag(_lib.GRAPHNORM), flag(_lib.NODE_ATTENTION)
    gates = flag(_lib.RESIDUAL) and (flag(_lib.REZERO) or flag(_lib.GATED_RESIDUAL))
    eatt, soft = flag(_lib.EDGE_ATTENTION), flag(_lib.SOFTMAX_ATT)
    p = dict(graphnorm=gn, edge_res=flag(_lib.EDGE_RESIDUAL) and f['has_m_prev'],
             coord_bwd=flag(_lib.UPDATE_COORDS) and f['has_g_x_out'], soft_dots=eatt and soft)
    p['fused_wgrads'] = (f['wgrads_supported'] and f['gr_node_w2'] and f['gr_node_w1'] and f['gr_edge_w1']
                         and not split_wgrads)
    p['fam'] = GENERIC if (H not in (32, 64, 128) or A > 3) else (WIDE if H == 128 else SPLIT)
    p['mfma_bwd'] = p['fam'] != GENERIC
    p['first_layer'] = False                                  # (the cells ask for g_x)
    assert f['has_g_x']
    chain = not gn and not gates and not split_small and f['mlp_fused_ok'] and f['chain_aligned']
    plain_out = not flag(_lib.RESIDUAL) and not natt and not split_small
    p['g_o_is_g_h_out'] = plain_out or (chain and not natt)
    p['node_out_bwd'] = not plain_out and not chain
    p['gate_in_wgrads'] = natt and p['fused_wgrads'] and not split_small and f['gr_node_att_w'] and f['gr_node_att_b']
    p['own_node_att_w'] = natt and not p['gate_in_wgrads'] and f['gr_node_att_w']
    p['own_node_att_b'] = natt and not p['gate_in_wgrads'] and f['gr_node_att_b']
    p['own_node_gate'] = gates and f['gr_node_gate']
    p['gu_product'] = not chain
    gu_ok = f['gu_passthrough_epilogue_ok'] if p['g_o_is_g_h_out'] else f['gu_epilogue_ok']
    p['fuse_tail_bwd'] = not gn and gu_ok and f['sy1_aligned']
    p['tail_bwd1'] = not p['fuse_tail_bwd'] and not chain
    p['gh_accumulate'] = not plain_out
    prep_side = not split_small and f['gpq_aligned'] and f['gm_epilogue_ok']
    if chain:
        p['gh_gm'], p['prep'] = GHGM_CHAIN, PREP_CHAIN
    elif H == 32 and prep_side and f['both_epilogue_ok']:
        p['gh_gm'], p['prep'] = GHGM_ONE, PREP_SIDE
    else:
        p['gh_gm'], p['prep'] = GHGM_TWO, (PREP_SIDE if prep_side else PREP_OWN)
    for slot in ('node_w2', 'node_b2', 'node_w1', 'node_b1', 'edge_w1', 'edge_b1'):
        p['own_' + slot] = f['gr_' + slot] and not p['fused_wgrads']
    p['tail_folded'] = p['mfma_bwd'] and p['fused_wgrads'] and not split_small
    p['slab_reduce'] = REDUCE_ONE_SET if not p['mfma_bwd'] else REDUCE_FOLDED if p['tail_folded'] else REDUCE_TWO_SETS
    p['gh_folded'] = p['tail_folded'] and f['gh_gpq_aligned']
    p['node_b1_from_coefs'] = gn and f['gr_node_b1']
    p['has_att'] = (2 if soft else 1) if eatt else 0
    p['has_gate'] = (p['edge_res'] or (flag(_lib.EDGE_RESIDUAL) and f['no_edges'])) and (flag(_lib.REZERO) or
                                                                                        flag(_lib.GATED_RESIDUAL))
    assert sorted(p) == sorted(PLAN_FIELDS)
    return {k: int(p[k]) for k in PLAN_FIELDS}


def plan_for(cell):
    return expected_plan(facts_for(cell), cell['env'])


# tensors of the forward: 4 bytes off, its own dispatch moves too (node_mlp_forward: can_epi, the fused chain; node_pre_forward)
# and the backward starts from other bits whatever its plan says
FORWARD_OFFSETS = frozenset(('h', 'h_out', 'saved'))


def same_launches(plan, base_plan):
    return all(plan[k] == base_plan[k] for k in PLAN_FIELDS if k not in WRITE_ONLY_FIELDS)


def same_launches_as_full(cell):
    """True: the cell's plan is the baseline's in every field outside WRITE_ONLY_FIELDS, so every tensor both runs return
    must agree bit for bit. (fp64 has no plan: layer_f64.hip guards each gradient's own launches by its slot, and the
    launches every result shares do not depend on the slots - true whenever only slots differ.)"""
    base = baseline_of(cell)
    if base is None or base is cell:
        return False
    if cell['dtype'] == 'f64':
        return not cell['offsets']
    if FORWARD_OFFSETS & set(cell['offsets']):
        return False
    return same_launches(plan_for(cell), plan_for(base))


# ---- the launches of a plan ------------------------------------------------------------------------------------------------
COUNTED = ('node_mlp_bwd', 'node_wgrads', 'node_out_bwd', 'node_tail', 'tsgemm_mfma', 'linear_mfma', 'linear_generic',
           'colreduce4', 'colreduce')


def routes_for(cell):
    """Launches of the BACKWARD alone per hook group of COUNTED (fp32), from the steps of layer_api.hip:
      1 bwd_output_stage     pvs_node_out_bwd | k_node_mlp_bwd; own column sums of the node gate (t1: 4-wide, gl: one
                             column = the scalar kernel) and of the residual gate (tg)
      2 bwd_node_mlp_to_gy1  g_u product; own node_mlp.3 weight (tsgemm) and bias (column sum of g_o - g_h_out itself where
                             the plan says so, scalar kernel when that is off 16 bytes); pvs_node_tail_bwd1; GraphNorm:
                             column sums S1, S2 (S2 reads saved y1) and pvs_node_tail_bwd2
      3 bwd_gh_gm            one double-width product | g_h and gM products; own node_mlp.0 weight (two tsgemm) and bias
      5 bwd_weight_tail      the g_P / g_Q product unless folded (at H = 64 the folded one is a linear launch of
                             pvs_launch_node_wgrads); k_node_wgrads | own edge_mlp.0 weight (two tsgemm) and bias
    A linear launch is the MFMA kernel at hidden 32 / 64 with x and y on 16 bytes, two (four with two operands) 64-column
    MFMA chunks at hidden 128, the generic kernel otherwise."""
    assert cell['dtype'] == 'f32'
    H, p = cell['hid'], plan_for(cell)
    on16 = {name: name not in cell['offsets'] for name in OFFSET_NAMES}
    r = dict.fromkeys(COUNTED, 0)

    def linear(aligned, operands=1):
        if H in (32, 64) and aligned:
            r['linear_mfma'] += 1
        elif H == 128 and aligned:
            r['linear_mfma'] += 2 * operands
        else:
            r['linear_generic'] += 1

    def colsum(aligned=True):
        r['colreduce4' if aligned else 'colreduce'] += 1

    g_o_on16 = on16['g_h_out'] if p['g_o_is_g_h_out'] else True
    r['node_out_bwd'] = p['node_out_bwd']
    r['node_mlp_bwd'] = int(p['gh_gm'] == GHGM_CHAIN)
    if p['own_node_att_w']:
        colsum()
    if p['own_node_att_b']:
        colsum(False)
    if p['own_node_gate']:
        colsum()
    if p['gu_product']:
        linear(g_o_on16)
    tsgemm = p['own_node_w2'] + 2 * p['own_node_w1'] + 2 * p['own_edge_w1']
    if p['own_node_b2']:
        colsum(g_o_on16)
    r['node_tail'] = p['tail_bwd1'] + p['graphnorm']
    if p['graphnorm']:
        colsum()
        colsum(on16['saved'])
    if p['gh_gm'] == GHGM_ONE:
        linear(True)
    elif p['gh_gm'] == GHGM_TWO:
        linear(on16['g_h'])
        linear(True)
    if p['own_node_b1']:
        colsum()
    if not p['gh_folded']:
        linear(on16['g_h'], operands=2)
    elif H == 64:
        linear(True)
    r['node_wgrads'] = p['fused_wgrads']
    if p['own_edge_b1']:
        colsum()
    if H in (32, 64):
        r['tsgemm_mfma'] = tsgemm
    return {k: v for k, v in r.items() if v}


def forward_chain(cell):
    """node_mlp_forward (layer_api.hip): the folded chain k_node_mlp_fwd needs hidden 32 / 64, no GraphNorm, no rezero /
    gated residual, no PVS_EGNN_SPLIT_SMALL, and h, h_out and the saved pieces (Magg, y1, u, o) on 16 bytes."""
    F = layer_flags(cell['flags'])
    gates = bool(F & _lib.RESIDUAL) and bool(F & (_lib.REZERO | _lib.GATED_RESIDUAL))
    on16 = all(name not in cell['offsets'] for name in ('h', 'h_out', 'saved'))
    return (cell['hid'] in (32, 64) and not F & _lib.GRAPHNORM and not gates and on16
            and 'PVS_EGNN_SPLIT_SMALL' not in cell['env'])
