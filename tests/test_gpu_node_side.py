"""The node side of EGNNLayer at every row-count edge, node flag kind and attention activation.

The edge-class and work-partition tests run one 96-node graph. What picks the node-level code is the node count (32-row
MFMA tiles, 128-row workgroups, the 256-row blocks of k_node_wgrads, the 512 rows of a tsgemm block, 64 / H nodes per
wave of k_node_out_*, the two column-to-wave maps and the 1280-block cap of k_node_gather, the 2048-block cap of the
generic edge kernels, ew_grid's 4096 blocks, rows_m = 256 from 32768 rows on), the node flag kind (GraphNorm, rezero,
gated residual - at or below a gate of 0 too -, node attention alone, no residual) and the attention activation.
Hidden 32 / 64 without GraphNorm and without a gate run the folded chain k_node_mlp_fwd / _bwd; everything else, and
every layer at hidden 16 and 65 ... 128, the separate tail and output stage (k_node_tail_*, k_node_out_*<H> / _wide<2>)
with unfused tsgemm weight gradients and per-gate column reductions; hidden 32 / 64 the fused weight-gradient pass
k_node_wgrads. test_node_routes reads the route each cell took from the library's measurement hook.

Arbiter and bound: those of tests/test_gpu_edge_classes.py, whose Problem this file reuses - autograd on the fp64
oracle layer, assert_strict with three fp32 oracle draws, per tensor; fp64 layers: the bound of tests/test_gpu_fp64.py.
Inputs: tests/_node_count_cases.py, pinned on the host by tests/test_node_count_cases_host.py.
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import _node_count_cases as ncc
from tests.test_gpu_dense_ops import NODE_ROUTE_NAMES, ROUTE_FIRST_ID, ROUTE_NAMES
from tests.test_gpu_edge_classes import FLAGS, Problem, _check64, _environment

pytestmark = pytest.mark.gpu

WIDTHS = (16, 32, 64, 128)
NODE_KINDS = ('nores', 'gn', 'natt-sigmoid', 'natt-tanh', 'natt-relu', 'natt-silu', 'rezero0', 'rezero', 'gated+',
              'gated0', 'gated-', 'eatt-tanh', 'eatt-relu', 'eatt-silu')
CLOSED_GATE = ('gated0', 'gated-')          # relu(gate) = 0: h_out = h, and relu cuts the gate's gradient
KIND_N = (129, 5121)
SMALL_N = 1000                              # problems up to this size are kept for the other tests of the session


def _cell(group, n, hid, flags, family='default', grad=True, edges=True, twice=False):
    tag = f'{group}-N{n}-H{hid}-{family}-{flags}-{"grad" if grad else "nograd"}'
    return pytest.param(dict(group=group, n=n, hid=hid, flags=flags, family=family, env={}, grad=grad, edges=edges,
                             twice=twice, tag=tag), id=tag)


def _cells():
    out = []
    # node counts x widths: plain (the folded chain) and full (separate tail and output stage) at H = 32 / 64, full at
    # H = 16 / 128; hidden 48 and 100 zero-padded to 64 and 128 at one row past a tile
    for n in ncc.NODE_COUNTS:
        twice = n in (257, 5121)
        for hid in WIDTHS:
            if ncc.ONLY_AT_WIDTH.get(n, hid) != hid:
                continue
            if hid in (32, 64):
                out.append(_cell('count', n, hid, 'plain', twice=twice))
            out.append(_cell('count', n, hid, 'full', twice=twice))
    for n in (33, 257):
        out += [_cell('count', n, hid, 'full', twice=n == 257) for hid in (48, 100)]
    # flag kinds x widths, at one row past a 128-row workgroup and past the gather's grid cap
    for n in KIND_N:
        for hid in WIDTHS:
            out += [_cell('kind', n, hid, flags, twice=flags.startswith(('natt-', 'gated'))) for flags in NODE_KINDS]
    # activations x families (H = 16 is generic whatever the family)
    for flags in ('eatt-tanh', 'eatt-relu', 'eatt-silu'):
        for hid, family in ((32, 'default'), (32, 'exact'), (64, 'default'), (64, 'exact'), (16, 'default'),
                            (128, 'default'), (128, 'exact')):
            out.append(_cell('act', 513, hid, flags, family))
    # no edges: one node, and 37 nodes without an edge; forward only, and forward with backward
    for n in (1, ncc.EDGELESS_N):
        for hid in WIDTHS:
            for flags in ('plain', 'full', 'soft', 'rezero'):
                out += [_cell('noedges', n, hid, flags, grad=grad, edges=False) for grad in (False, True)]
    return out


CELLS = _cells()
_BY_KEY = {(c.values[0]['group'], c.values[0]['n'], c.values[0]['hid'], c.values[0]['flags']) for c in CELLS}
for _hid in WIDTHS:      # the first N above every grid cap runs the separate tail and output stage at every width
    for _n in (5121, 8200) + tuple(n for n, h in ncc.ONLY_AT_WIDTH.items() if h == _hid):
        assert ('count', _n, _hid, 'full') in _BY_KEY, (_n, _hid)


def _build(n, hid, flags, edges):
    return Problem(ncc.N_CLASSES, hid, flags, graph=ncc.graph_for(n, edges))


_kept = functools.lru_cache(maxsize=None)(_build)


def _problem(n, hid, flags, edges=True):
    """Inputs and oracle references of one layer on the N-node graph, built once and left unchanged; the small ones
    are shared by the tests of the session (a 30,000-edge problem at 128 channels holds 100 MB: built where it is used)."""
    edges = edges and n > 1
    return _kept(n, hid, flags, edges) if n <= SMALL_N else _build(n, hid, flags, edges)


def _differing(first, second):
    assert set(first) == set(second)
    return [k for k in first if first[k].tobytes() != second[k].tobytes()]


ZERO_WITHOUT_EDGES = ('grad edge_mlp.', 'grad coord_mlp.', 'grad att_mlp.', 'grad edge_gate_parameter')


def _assert_without_edges(p, got, cell, failures):
    """No edge: no message, no coordinate update - x_out is x itself, and every gradient that the fp64 reference has
    identically zero (the edge, coordinate and attention MLPs, the edge gate) is 0.0, not a residue."""
    assert int(p.g.edge_index.shape[1]) == 0 and got['m'].size == 0
    if got['x_out'].tobytes() != p.g.pos.numpy().tobytes():
        failures.append('x_out is not x bit for bit')
    if not cell['grad']:
        return
    dead = [k for k in p.ref64 if k.startswith(ZERO_WITHOUT_EDGES)]
    want = 7 + (2 if p.flags.get('edge_attention') else 0) + (1 if p.flags.get('edge_residual') else 0)
    assert len(dead) == want, dead
    for k in dead:
        assert not p.ref64[k].any(), k
        if got[k].any() or not np.isfinite(got[k]).all():
            failures.append(f'{k} is not 0.0 on a graph without edges (max |.| = {np.abs(got[k]).max():.3e})')


def _assert_closed_gate(p, got, cell, failures):
    """relu(gate) = 0: h_out = 0 * o + 1 * h is h itself, relu cuts the gate's gradient to exactly 0, and the residual
    hands the whole upstream gradient to g_h. The last one is read off a second run whose loss leaves h_out out: with a
    closed gate nothing of g_h_out reaches the node MLP, so the two g_h differ by g_h_out = wh itself, up to the
    rounding of the at most 2 H + 4 fp32 additions between the residual's part and the finished g_h."""
    if got['h_out'].tobytes() != p.h0.numpy().tobytes():
        failures.append('h_out is not h bit for bit under a closed gate')
    gate = float(got['grad node_gate_parameter'].reshape(-1)[0])
    if gate != 0.0:
        failures.append(f'node_gate_parameter.grad = {gate:.3e}, not 0.0, at gate <= 0')
    for k in ('grad node_mlp.0.weight', 'grad node_mlp.0.bias', 'grad node_mlp.3.weight', 'grad node_mlp.3.bias'):
        if got[k].any():
            failures.append(f'{k} is not 0.0 under a closed gate')
    q = copy.copy(p)
    q.wh = torch.zeros_like(p.wh)
    with _environment(cell):
        without = q.gpu()['g_h']
    wh = p.wh.numpy().astype(np.float64)
    err = float(np.abs(got['g_h'].astype(np.float64) - without.astype(np.float64) - wh).max())
    scale = max(float(np.abs(got['g_h']).max()), float(np.abs(wh).max()))
    bound = (2 * cell['hid'] + 4) * 2.0 ** -24 * scale
    print(f'{cell["tag"]}: g_h - g_h(no h_out in the loss) - wh: {err:.3e} (bound {bound:.3e})')
    if not err <= bound:
        failures.append(f'g_h does not carry the full upstream gradient: {err:.3e} > {bound:.3e}')


@pytest.mark.parametrize('cell', CELLS)
def test_node_side_matches_the_fp64_oracle(cell):
    """Outputs (h, coord, messages, att_val / node_att_val), input gradients and every parameter gradient of one
    EGNNLayer.forward (+ backward) under the strict bound. Cells marked `twice` (N = 257 and 5121 of every width, every
    natt-* / gated* cell) run a second time and must agree bit for bit. Without edges and under a closed gate, the
    exact statements of _assert_without_edges / _assert_closed_gate on top."""
    p = _problem(cell['n'], cell['hid'], cell['flags'], cell['edges'])
    assert p.g.n_nodes == cell['n']
    with _environment(cell):
        got = p.gpu(grad=cell['grad'])
        again = p.gpu(grad=cell['grad']) if cell['twice'] else None
    failures = []
    if again is not None:
        differing = _differing(got, again)
        if differing:
            failures.append(f'two runs differ in {differing}')
    if not cell['edges'] or cell['n'] == 1:
        _assert_without_edges(p, got, cell, failures)
    if cell['flags'] in CLOSED_GATE and cell['grad']:
        _assert_closed_gate(p, got, cell, failures)
    try:
        p.check(got, cell['tag'], grad=cell['grad'])
    except AssertionError as exc:
        failures.append(str(exc))
    assert not failures, '\n'.join(failures)


@pytest.mark.parametrize('flags', ['full', 'rezero', 'gated-'])
@pytest.mark.parametrize('n', [1, 33, 257])
def test_fp64_node_tail(n, flags):
    """The fp64 node tail (csrc/layer_f64.hip) on one node without an edge, one row past a tile and past a row block."""
    p = _problem(n, 32, flags)
    got = p.gpu(dtype=torch.float64)
    _check64(p, got, f'fp64-N{n}-H32-{flags}')
    if flags in CLOSED_GATE:
        assert got['h_out'].tobytes() == p.h0.double().numpy().tobytes()
        assert float(got['grad node_gate_parameter'].reshape(-1)[0]) == 0.0
    if n == 1:
        assert got['x_out'].tobytes() == p.g.pos.double().numpy().tobytes()
        for k in (k for k in p.ref64 if k.startswith(ZERO_WITHOUT_EDGES)):
            assert not p.ref64[k].any() and not got[k].any(), k


# ---- the route a cell took ----------------------------------------------------------------------------------------------
TSGEMM_NAMES = tuple(name for name in ROUTE_NAMES if name.startswith('tsgemm'))
RECORDED = NODE_ROUTE_NAMES + ('colreduce4', 'colreduce', 'colreduce_chunk') + TSGEMM_NAMES


def expected_routes(hid, flags):
    """Launches of one forward and one backward with every gradient, written from node_mlp_forward and
    pvs_egnn_layer_bwd (csrc/layer_api.hip).
    Hidden 32 / 64 (the MFMA linear takes the layer's products with an epilogue, pvs_node_mlp_fused_supported):
      no GraphNorm, no gate   k_node_mlp_fwd and k_node_mlp_bwd, nothing else of the node side
      otherwise               forward: k_node_tail_fwd under GraphNorm (else SiLU rides on the first product),
                              k_node_out_fwd with node attention or a gate (else the residual rides on the second);
                              backward: k_node_out_bwd, and k_node_tail_bwd1 / _bwd2 under GraphNorm
      always                  k_node_wgrads: every weight gradient, the bias sums and the node gate's two sums
    Hidden 16 / 128 (no epilogue, no folded chain, no fused weight gradients): k_node_tail_fwd, k_node_out_fwd,
    k_node_tail_bwd1 always, k_node_out_bwd unless the layer has neither residual nor node attention (g_o = g_h_out),
    five tsgemm products (node_mlp.3, two halves of node_mlp.0, two of edge_mlp.0), three bias column sums, two more for
    node attention (the bias's over a one-column array: the scalar kernel).
    Column sums on top: one for a node gate parameter, four for GraphNorm (mean, variance; S1, S2)."""
    f = FLAGS[flags]
    res, natt, gn = f.get('residual', True), bool(f.get('node_attention')), bool(f.get('graphnorm'))
    gate = res and bool(f.get('rezero') or f.get('gated_residual'))
    want = {}
    if hid in (32, 64):
        if not gn and not gate:
            want.update(node_mlp_fwd=1, node_mlp_bwd=1)
        else:
            want['node_tail'] = 3 if gn else 0
            want['node_out_fwd'] = 1 if (natt or gate) else 0
            want['node_out_bwd'] = 1 if (res or natt) else 0
        want['node_wgrads'] = 1
        want['colreduce4'] = (1 if gate else 0) + (4 if gn else 0)
    else:
        want['node_tail'] = 3 if gn else 2
        want['node_out_fwd'] = 1
        want['node_out_bwd'] = 1 if (res or natt) else 0
        want['colreduce4'] = 3 + (1 if natt else 0) + (1 if gate else 0) + (4 if gn else 0)
        want['colreduce'] = 1 if natt else 0
        want['tsgemm_tn8' if hid == 16 else 'tsgemm_wide'] = 5
    return {k: v for k, v in want.items() if v}


@pytest.mark.parametrize('flags', ('plain', 'full') + NODE_KINDS)
@pytest.mark.parametrize('hid', WIDTHS)
def test_node_routes(hid, flags):
    """One cell per (width class, flag kind): the node-level launchers of its forward and backward, and the column
    reductions and tsgemm products beside them, as the measurement hook recorded them - the folded chain where the
    table says folded, the separate stages where it says separate, the fused weight-gradient pass at 32 / 64 only."""
    from pointvs_amd import _lib
    lib = _lib.lib()
    p = _problem(129, hid, flags)
    first = ROUTE_FIRST_ID + len(ROUTE_NAMES)
    mask = sum(1 << (ROUTE_FIRST_ID + ROUTE_NAMES.index(name) + 1) for name in RECORDED if name in ROUTE_NAMES)
    mask += sum(1 << (first + k + 1) for k in range(len(NODE_ROUTE_NAMES)))
    lib.pvs_profile_reset()
    lib.pvs_profile_enable(mask)
    try:
        p.gpu()
    finally:
        lib.pvs_profile_enable(0)
    seen = {}
    for name in RECORDED:
        ms, cnt = C.c_double(0.0), C.c_int64(0)
        assert lib.pvs_profile_read(name.encode(), C.byref(ms), C.byref(cnt)) == 0, name
        if cnt.value:
            seen[name] = cnt.value
    lib.pvs_profile_reset()
    assert seen == expected_routes(hid, flags)
