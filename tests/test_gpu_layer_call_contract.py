"""The documented contract of pvs_egnn_layer_bwd that the Python package never exercises: "grads: members may be NULL to
skip" (include/pvs_egnn.h), caller tensors that sit 4 bytes off a 16-byte boundary, and PVS_EGNN_SPLIT_WGRADS / _SMALL -
through the C entries directly (tests/_layer_call.py), over the cells of tests/_grad_subset_cases.py (pinned on the host by
tests/test_grad_subset_cases_host.py, which also says which launches each cell is there for).

Per cell: the returned keys are the requested ones; outputs, input gradients and every requested parameter gradient
pass the bound of tests/test_gpu_edge_classes.py Problem.check (assert_strict against the fp64 oracle with three fp32
oracle draws and grad_floor; the rho / class columns of edge_mlp.0.weight.grad on their own) - fp64 cells the bound of
tests/test_gpu_fp64.py; every guard element around every caller tensor is intact and no element of a written output still
holds the arena's fill pattern; where the cell's plan is the baseline's but for dropped writes, every returned tensor is
bit-identical to the baseline run; the launches recorded by the measurement hook are those the table states; offset,
unfused and switch cells run twice and agree bit for bit.

Alignment. What reads or writes a caller tensor (h, h_out, saved, g_h_out, g_h) with 8- or 16-byte accesses:
  gated by a host check, with a fallback that the offset cells take
    k_node_mlp_fwd / k_node_mlp_bwd     pvs_node_mlp_fused_supported + the `*_aligned` facts -> the separate launches
    k_linear_mfma (epilogues, side jobs) pvs_linear_epilogue_supported / aligned16 of pvs_launch_linear -> k_linear
    the g_h role of k_node_wgrads        gh_gpq_aligned -> the product as a launch of its own
    k_colreduce4                         vec4 of pvs_launch_colreduce (g_h_out as g_o, saved y1 for S2) -> k_colreduce
    P | Q with the forward's clears      node_pre_forward: side_ok (Magg) and the epilogue check (PQ) -> two launches
  gated by nothing: the edge kernels on `saved`
    edge_mfma_common.h gather_tile / gather_tile32 (float4 of P and Q rows; every MFMA edge forward and backward),
    edge_mfma_fwd.hip (float4 stores of the Magg rows by k_edge_fwd_mfma's flush, k_init_fwd's clears); m_prev, m_out and
    g_m_prev rows likewise (not offset here: rows of H floats from a 256-byte start). The generic edge kernels
    (edge_v0.hip) use float4 on LDS and on the workspace only
  element by element, any alignment: k_node_out_*, k_node_tail_*, k_tsgemm_mfma, k_tsgemm_tn, k_node_wgrads' operand
  loads, k_linear, k_reduce_slabs (the writer of every unfused weight gradient, at any ldo)
None of the ungated accesses needs 16 bytes to be correct: they are global-memory vector loads and stores, which gfx950
serves at any 4-byte-aligned address (no LDS access and no packed atomic is formed from a caller pointer), so a `saved`
that is 4 bytes off costs bandwidth, not correctness; the `saved` cells assert exactly that, value for value.
"""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import _grad_subset_cases as gsc
from tests import _layer_call as lc
from tests._golden import CaseLog, assert_strict

pytestmark = pytest.mark.gpu

DTYPES = {'f32': torch.float32, 'f64': torch.float64}
F32_CELLS = [c for c in gsc.CELLS if c['dtype'] == 'f32']
F64_CELLS = [c for c in gsc.CELLS if c['dtype'] == 'f64']


def _problem(cell):
    if cell['A'] != 3:
        from tests.test_gpu_edge_classes import problem
        p = problem(cell['A'], cell['hid'], cell['flags'])
    else:
        from tests.test_gpu_node_side import _problem as node_problem
        p = node_problem(cell['n'], cell['hid'], cell['flags'])
    assert p.g.n_nodes == cell['n'] and int(p.g.edge_index.shape[1]) <= 3200        # (6 N edges; the class graph: 3200)
    return p


def _run(cell, routes=False):
    """-> (values, guards_intact, untouched_outputs, forward routes, backward routes)."""
    p = _problem(cell)
    offsets = dict.fromkeys(cell['offsets'], 1)
    seen_f, seen_b = {}, {}
    if routes:
        with lc.recorded_routes(('node_mlp_fwd',)) as seen_f:
            fwd = lc.forward(p, offsets, cell['env'], DTYPES[cell['dtype']])
        with lc.recorded_routes(gsc.COUNTED) as seen_b:
            out = lc.backward(p, fwd, cell['skip'], offsets, cell['env'])
    else:
        fwd = lc.forward(p, offsets, cell['env'], DTYPES[cell['dtype']])
        out = lc.backward(p, fwd, cell['skip'], offsets, cell['env'])
    return out + (seen_f, seen_b)


@functools.lru_cache(maxsize=None)
def _baseline(tag):
    """The all-slots, aligned run of a (n, hid, flags, env): run once, shared, left unchanged."""
    values, guards, untouched, _, _ = _run(gsc.BY_TAG[tag])
    assert guards and not untouched
    return values


def _expected_keys(p, cell):
    keys = {k for k in p.ref64 if not k.startswith('grad ')}
    return keys | {'grad ' + lc.state_dict_name(slot) for slot in gsc.requested(cell)}


def _differing(a, b):
    assert set(a) == set(b)
    return sorted(k for k in a if a[k].tobytes() != b[k].tobytes())


def _check32(p, got, tag):
    """Problem.check for a reduced key set: assert_strict per key, gradients with the case's floor, the trailing columns
    of edge_mlp.0.weight.grad on their own."""
    log = CaseLog(tag)
    for key in sorted(got):
        floor = p.floor if key.startswith('g') else 0.0
        ref64, ref32 = p.ref64[key], [r[key] for r in p.ref32]
        assert got[key].dtype == np.float32, key
        value = got[key].reshape(ref64.shape)
        assert_strict(value, ref64, ref32, f'{tag} {key}', floor=floor, log=log)
        if key.endswith('edge_mlp.0.weight'):
            for label, c in p.class_columns(key):
                assert_strict(value[:, c], ref64[:, c], [r[:, c] for r in ref32], f'{tag} {key}[:, {label}]', floor=floor,
                              log=log)
    log.finish()


def _check64(p, got, tag):
    from tests.test_gpu_fp64 import _check
    g_max = max(float(np.abs(v).max()) for k, v in p.ref64.items() if k.startswith('grad '))
    for key in sorted(got):
        assert got[key].dtype == np.float64, key
        _check(got[key], p.ref64[key], f'{tag} {key}', g_max if key.startswith('g') else 0.0)
        if key.endswith('edge_mlp.0.weight'):
            for label, c in p.class_columns(key):
                _check(got[key].reshape(p.ref64[key].shape)[:, c], p.ref64[key][:, c], f'{tag} {key}[:, {label}]', g_max)


def _contract(cell, check):
    p = _problem(cell)
    got, guards, untouched, seen_f, seen_b = _run(cell, routes=cell['dtype'] == 'f32')
    assert set(got) == _expected_keys(p, cell), sorted(set(got) ^ _expected_keys(p, cell))
    failures = []
    if not guards:
        failures.append('a guard element around a caller tensor was overwritten')
    if untouched:
        failures.append(f'elements still holding the fill pattern: {untouched}')
    if cell['dtype'] == 'f32':
        want_f = {'node_mlp_fwd': 1} if gsc.forward_chain(cell) else {}
        print(f'{cell["tag"]}: forward {seen_f} backward {seen_b}')
        if seen_f != want_f:
            failures.append(f'forward route {seen_f}, the table says {want_f}')
        if seen_b != gsc.routes_for(cell):
            failures.append(f'backward routes {seen_b}, the table says {gsc.routes_for(cell)}')
    if gsc.same_launches_as_full(cell):
        base = _baseline(gsc.baseline_of(cell)['tag'])
        differing = [k for k in got if got[k].tobytes() != base[k].tobytes()]
        if differing:
            failures.append(f'not bit-identical to the all-slots run: {differing}')
    if cell['twice'] or cell['offsets'] or cell['env']:
        again = _run(cell)[0]
        if _differing(got, again):
            failures.append(f'two runs differ in {_differing(got, again)}')
    try:
        check(p, got, cell['tag'])
    except AssertionError as exc:
        failures.append(str(exc))
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('cell', F32_CELLS, ids=[c['tag'] for c in F32_CELLS])
def test_layer_call_contract(cell):
    _contract(cell, _check32)


@pytest.mark.parametrize('cell', F64_CELLS, ids=[c['tag'] for c in F64_CELLS])
def test_layer_call_contract_fp64(cell):
    """pvs_egnn_layer_bwd_f64 guards every gradient's own launches by its slot (csrc/layer_f64.hip)."""
    _contract(cell, _check64)


def test_the_helper_is_the_python_path():
    """The direct caller with every slot and nothing offset returns, bit for bit, what EGNNLayer.forward + autograd
    return: what the cells add is the NULL slots and the offsets, not another way of calling."""
    cell = gsc.BY_TAG['base-N33-H32-full-all']
    p = _problem(cell)
    via_python = p.gpu()
    assert _differing(_baseline(cell['tag']), via_python) == []


# ---- the one-call layer stack hands NULL members down per layer --------------------------------------------------------
@pytest.mark.parametrize('skipped', ['node_w2', 'every'])
@pytest.mark.parametrize('name', ['cfg3_like', 'test_kwargs'])
def test_stack_with_skipped_slots_equals_the_per_layer_calls(name, skipped, monkeypatch):
    """`dead_grads` decides the NULL slots of both paths (_EGNNLayerFn.backward, _GradLayout): with node_w2 - or every
    slot - added to what it returns, pvs_egnn_stack_bwd passes NULL members down per layer. Logits, every gradient and
    which gradients are None agree bit for bit with the per-layer path, and the skipped parameters get no gradient."""
    import pointvs_amd.functional as PF
    from pointvs_amd import _lib
    from tests.test_gpu_properties import make_model, random_graph
    from tests.test_gpu_stack import FLAG_SETS, _run as run_steps, _same
    real = PF.dead_grads
    extra = ('node_w2',) if skipped == 'node_w2' else _lib.PARAM_FIELDS

    def dead(flags, coords_fed, edge_res):
        return tuple(dict.fromkeys(real(flags, coords_fed, edge_res) + extra))
    monkeypatch.setattr(PF, 'dead_grads', dead)
    model, _ = make_model(seed=5, **FLAG_SETS[name])
    twin = copy.deepcopy(model)
    g = random_graph(300, 5000, seed=3).to('cuda')
    la, ga, _ = run_steps(model, g, monkeypatch, stack=False)
    assert model.__dict__.get('_stack_cache') is None
    lb, gb, _ = run_steps(twin, g, monkeypatch, stack=True)
    assert twin.__dict__.get('_stack_cache') is not None, 'the one-call stack did not run'
    _same(la[0], lb[0], 'logits')
    assert ga.keys() == gb.keys()
    for pname in ga:
        _same(ga[pname], gb[pname], f'grad {pname}')
    layer_names = [n for n in ga if n.startswith('layers.') and not n.startswith('layers.0.')]
    gone = [n for n in layer_names if skipped == 'every' or '.node_mlp.3.weight' in n]
    assert gone and all(ga[n] is None and gb[n] is None for n in gone)
    kept = [n for n in layer_names if n not in gone and '.coord_mlp.' not in n]
    assert all(ga[n] is not None for n in kept) and (skipped == 'every' or kept)
    # what lies before the layers still gets its gradient through them: the input gradients of every layer were computed
    first = [n for n in ga if n.startswith('layers.0.')]
    assert first and all(ga[n] is not None and bool(ga[n].abs().max() > 0) for n in first)
