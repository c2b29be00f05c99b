"""The partial first layer of the screens for softmax-attention layers, per row, against the fp64 oracle:
pvs_egnn_layer_edge_stats_softmax and pvs_egnn_layer_fwd_partial_softmax (k_pack_base_rows, k_combine_partial_softmax,
k_scale_att_rows behind the softmax MFMA edge forward), called through pointvs_amd._lib as screening.py calls them.

Arbiter: oracle.egnn_oracle.egnn_layer in fp64 on the union graph. Bound: tests/_golden.py assert_strict with three fp32
oracle draws, on each tensor as a whole and on the rows of each kind as tensors of their own. Inputs and references:
tests/_softmax_partial_cases.py, pinned on the host by tests/test_softmax_partial_cases_host.py (which also shows that
a dropped base, attention left normalised over the partial set, a merge without the shift to the common maximum and a
sigmoid on the node attention each move the oracle by more than 100 x this bound).

The base rows of every cell come from two sources: (a) the fp64 reference statistics rounded to fp32 - the partial entry
alone - and (b) pvs_egnn_layer_edge_stats_softmax over the base edges - what the screens run; (b)'s rows are held to the
reference statistics.
"""
import ctypes as C
import re

import numpy as np
import pytest
import torch

from tests import _partial_cases as pc
from tests import _softmax_partial_cases as spc
from tests._golden import CaseLog, strict_margin
from tests.test_gpu_edge_classes import FLAGS, _new_layer
from tests.test_gpu_partial_layer import (ONE_BLOCK, PAD_ROWS, ROOM, Device, _assert_refused, _environment, _same_bits,
                                          _sentinel)

pytestmark = pytest.mark.gpu


def _cell(A, hid, flags, family='default', ends='base', env=None):
    tag = f'softpartial-A{A}-H{hid}-{family}-{flags}-ends_{ends}'
    if env:
        tag += '-' + '-'.join(f'{k}={v}' for k, v in env.items())
    return pytest.param(dict(A=A, hid=hid, flags=flags, family=family, ends=ends, env=env or {}, tag=tag), id=tag)


def _cells():
    names = tuple(spc.flag_sets())
    out = [_cell(3, hid, flags) for hid in (32, 64, 128) for flags in names]
    out += [_cell(A, hid, flags) for A in (0, 5) for hid in (32, 64) for flags in ('soft', 'soft-full')]
    out += [_cell(3, hid, flags, ends='partial') for hid in (32, 64) for flags in ('soft', 'soft-full')]
    out += [_cell(3, hid, flags, 'exact') for hid in (32, 64) for flags in ('soft', 'soft-full')]
    out += [_cell(3, hid, 'soft-full', env=env) for hid in (32, 64) for env in ({'PVS_CHUNK_EDGES': '256'}, ONE_BLOCK)]
    return out


CELLS = _cells()


class SoftDevice(Device):
    """tests/test_gpu_partial_layer.Device with the two softmax entries (workspace mode 3)."""

    def workspace(self, n_edges):
        size = self.lib.pvs_egnn_layer_workspace_bytes(C.byref(self.desc), self.n, n_edges, 3)
        return torch.empty(size, dtype=torch.uint8, device='cuda'), size

    def reference_bases(self, p):
        rows = torch.as_tensor(p.reference_base_rows())
        return (self._rows(rows),) + tuple(self._rows(p.ref64[k]) for k in ('base_xsum', 'base_deg'))

    def edge_stats(self, pg, ws_bytes=None):
        ptr = self._lib.ptr
        ws, size = self.workspace(pg.c.n_edges)
        out = dict(rows=_sentinel(self.n, self.hid + 4), xsum=_sentinel(self.n, 3))
        rc = self.lib.pvs_egnn_layer_edge_stats_softmax(
            C.byref(self.desc), C.byref(pg.c), C.byref(self.pstruct), ptr(self.h), ptr(self.x), ptr(out['rows']),
            ptr(out['xsum']), ptr(ws), size if ws_bytes is None else ws_bytes, self._lib.stream(self.h.device))
        torch.cuda.synchronize()
        return rc, out

    def stat_bases(self, base_pg):
        rc, out = self.edge_stats(base_pg)
        assert rc == 0, self.error()
        rowptr = base_pg.t['rowptr']
        return out['rows'], out['xsum'], (rowptr[1:] - rowptr[:-1]).float().contiguous()

    def partial(self, pg, bases, att=False, ws_bytes=None, alias_x=False):
        """pvs_egnn_layer_fwd_partial_softmax (att: with an att_out of the graph's room + 5, else NULL) into outputs that
        hold the sentinel -> (return code, {h_out, x_out, natt, att})."""
        ptr = self._lib.ptr
        room = pg.c.n_edges
        ws, size = self.workspace(room)
        saved = torch.empty(self.lib.pvs_egnn_layer_saved_floats(C.byref(self.desc), self.n, room), device='cuda')
        out = dict(h_out=_sentinel(self.n, self.hid), x_out=self.x if alias_x else _sentinel(self.n, 3))
        if self.natt:
            out['natt'] = _sentinel(self.n)
        if att:
            out['att'] = _sentinel(room + 5)
        args = [C.byref(self.desc), C.byref(pg.c), C.byref(self.pstruct), ptr(self.h), ptr(self.x)]
        args += [ptr(b) for b in bases] + [ptr(out['h_out']), ptr(out['x_out']), ptr(out.get('natt')), ptr(out.get('att'))]
        args += [ptr(saved), ptr(ws), size if ws_bytes is None else ws_bytes, self._lib.stream(self.h.device)]
        rc = self.lib.pvs_egnn_layer_fwd_partial_softmax(*args)
        torch.cuda.synchronize()
        return rc, out


def _device(p, pad=0):
    return SoftDevice(p.case, p.new_layer(), p.h0, pad)


def _expected_keys(p):
    return {'h_out', 'x_out', 'att'} | ({'natt'} if p.kw['node_attention'] else set())


def _check_stats(p, d, bases, tag, log):
    """(b)'s base rows and xsum against the reference statistics; rows without base edges are all zero."""
    rows = bases[0].cpu().numpy()
    H = p.hid
    got = {'base_A': rows[:, :H], 'base_mu': rows[:, H], 'base_S': rows[:, H + 1], 'base_xsum': bases[1].cpu().numpy()}
    p.check({k: np.ascontiguousarray(v) for k, v in got.items()}, tag, log, n_rows=p.case.n_nodes)
    empty = np.flatnonzero(np.concatenate([p.ref64['base_deg'], np.zeros(d.pad)]) == 0)
    assert len(empty) >= 30 + d.pad
    if rows[empty].any() or got['base_xsum'][empty].any():
        log.failures.append(f'{tag}: a row without base edges is not all zero')
    if rows[:, H + 2:].any():
        log.failures.append(f'{tag}: the two trailing floats of a base row are not 0.0')
    filled = np.setdiff1d(np.arange(p.case.n_nodes), empty)
    if not (rows[filled, H + 1] >= 1).all():
        log.failures.append(f'{tag}: S < 1 on a row with base edges')
    assert np.array_equal(bases[2].cpu().numpy()[:p.case.n_nodes], p.ref64['base_deg'])
    if not p.kw['update_coords'] and got['base_xsum'].any():
        log.failures.append(f'{tag} base_xsum: not 0.0 without update_coords')


def _run_cell(p, d, pg, tag, log, n_rows=None):
    """Both sources of the base rows through the partial entry, every tensor under the strict bound."""
    stat = d.stat_bases(d.base_graph())
    _check_stats(p, d, stat, f'{tag} edge_stats', log)
    for source, bases in (('a', d.reference_bases(p)), ('b', stat)):
        got = d.layer_outputs(pg, bases)
        assert set(got) == _expected_keys(p)
        p.check(got, f'{tag} ({source})', log, n_rows=n_rows)
        if not p.kw['update_coords']:
            assert got['x_out'].tobytes() == d.x.cpu().numpy().tobytes(), 'x_out is not x without update_coords'


@pytest.mark.parametrize('cell', CELLS)
def test_softmax_partial_layer_matches_the_fp64_oracle(cell):
    """h_out, x_out, node_att_out and att_out (normalised over ALL edges of a row) of one softmax first layer through the
    partial entry, with the base rows from the reference (a) and from pvs_egnn_layer_edge_stats_softmax (b); (b)'s rows
    themselves. The entry with and without att_out gives the same bits, and att_out behind the edge count keeps its
    sentinel (Device.layer_outputs)."""
    p = spc.problem(cell['A'], cell['hid'], cell['flags'], cell['ends'])
    log = CaseLog(cell['tag'])
    with _environment(cell['family'], cell['env']):
        d = _device(p)
        _run_cell(p, d, d.partial_graph(), cell['tag'], log)
    log.finish()


def _union_forward(p, d):
    """pvs_egnn_layer_fwd, the existing single-pass forward, on the union graph -> h_out, x_out, natt, att over the
    partial list."""
    from pointvs_amd.graph import prepare_graph
    ei, ea = pc.union(p.case)
    pg = prepare_graph(ei.cuda(), None if ea is None else ea.cuda(), d.n, need_backward=False)
    pg.check_status()
    with torch.no_grad():
        h, x, _ = d.layer.forward_prepared(pg, d.h, d.x, None, need_m=False, need_coords=True)
    out = dict(h_out=h, x_out=x)
    if d.natt:
        out['natt'] = d.layer._natt_src().reshape(-1)
    out['att'] = d.layer._att_src().reshape(-1)[p.n_base:]      # (input order: the base list, then the partial list)
    return {k: v.detach().float().cpu().numpy() for k, v in out.items()}


def _worst(p, got):
    """Largest err / bound over the tensors of `got`, each as a whole and per row kind."""
    worst = 0.0
    for key, value in got.items():
        value = np.asarray(value).reshape(p.ref64[key].shape)
        for _, idx in [('all', slice(None))] + p.subsets(key):
            if isinstance(idx, np.ndarray) and idx.size == 0:
                continue
            err, bound = strict_margin(value[idx], p.ref64[key][idx], [r[key][idx] for r in p.ref32])
            worst = max(worst, err / bound if bound > 0 else (0.0 if err == 0 else float('inf')))
    return worst


@pytest.mark.parametrize('flags', ['soft', 'soft-full'])
def test_wide_spread_of_the_two_maxima(flags):
    """att_mlp.0.weight x gain at H = 32: mu_b - mu_g tens of units apart over the mixed rows, one row whose base weight and
    one whose partial weight underflow to 0. The yardstick is the existing single-pass forward on the union graph: the
    largest gain of 60, 20, 6 at which IT holds the strict bound is the gain at which the merged path must hold it."""
    log = CaseLog(f'softpartial-wide-H32-{flags}')
    chosen = None
    with _environment():
        for gain in spc.GAINS:
            p = spc.problem(3, 32, flags, 'base', gain)
            d = _device(p)
            single = _worst(p, _union_forward(p, d))
            print(f'wide {flags} gain {gain}: single-pass forward uses {single:.3f} of the bound')
            log.append((f'{log.case} single-pass gain{gain} used-of-bound', 1.0, single, 1.0))
            if single <= 1.0:
                chosen = gain
                break
        assert chosen is not None, 'the single-pass forward misses the bound at every gain'
        print(f'wide {flags}: gain {chosen}')
        _run_cell(p, d, d.partial_graph(), f'{log.case} gain{chosen}', log)
    log.finish()


@pytest.mark.parametrize('hid,flags', [(32, 'soft'), (32, 'soft-full'), (64, 'soft-full'), (128, 'soft-full')])
def test_device_side_edge_count_gives_the_host_count_bits(hid, flags):
    """n_edges = a capacity of E + 777, the count in n_edges_dev, the slots behind it full of edges of the hub row: every
    output has the bits of the host-count call, and att_out behind the count keeps its sentinel (layer_outputs)."""
    p = spc.problem(3, hid, flags)
    with _environment():
        d = _device(p)
        bases = d.reference_bases(p)
        host = d.layer_outputs(d.partial_graph(), bases)
        dev = d.layer_outputs(d.partial_graph(room=ROOM), bases)
        rc_h, stats_h = d.edge_stats(d.partial_graph())
        rc_d, stats_d = d.edge_stats(d.partial_graph(room=ROOM))
    assert rc_h == 0 and rc_d == 0
    _same_bits(host, dev)
    _same_bits({k: v.cpu().numpy() for k, v in stats_h.items()}, {k: v.cpu().numpy() for k, v in stats_d.items()})


@pytest.mark.parametrize('hid', [32, 64])
def test_graphnorm_over_a_device_row_count(hid):
    """40 trailing rows without edges as padding, n_norm_rows_dev = N - 40: the leading rows are the layer on the
    (N - 40)-row problem."""
    p = spc.problem(3, hid, 'soft-full')
    tag = f'softpartial-A3-H{hid}-default-soft-full-norm_rows'
    log = CaseLog(tag)
    with _environment():
        d = _device(p, pad=PAD_ROWS)
        assert d.n == p.case.n_nodes + 40 and p.kw['graphnorm']
        _run_cell(p, d, d.partial_graph(norm_rows=p.case.n_nodes), tag, log, n_rows=p.case.n_nodes)
    log.finish()


@pytest.mark.parametrize('cell', [_cell(3, 32, 'soft-full'), _cell(3, 64, 'soft-full'), _cell(5, 64, 'soft'),
                                  _cell(3, 128, 'soft-full'), _cell(3, 32, 'soft-full', 'exact'),
                                  _cell(3, 32, 'soft-full', env=ONE_BLOCK)])
def test_both_entries_are_bitwise_reproducible(cell):
    p = spc.problem(cell['A'], cell['hid'], cell['flags'])
    with _environment(cell['family'], cell['env']):
        d = _device(p)
        base_pg, pg, bases = d.base_graph(), d.partial_graph(), d.reference_bases(p)
        for run in (lambda: d.edge_stats(base_pg), lambda: d.partial(pg, bases), lambda: d.partial(pg, bases, att=True)):
            (rc1, first), (rc2, second) = run(), run()
            assert rc1 == 0 and rc2 == 0, d.error()
            _same_bits({k: v.cpu().numpy() for k, v in first.items()}, {k: v.cpu().numpy() for k, v in second.items()})


# ---- refusals -----------------------------------------------------------------------------------------------------------
ENTRIES = ('edge_stats', 'fwd_partial', 'fwd_partial_att')
ONLY = 'for layers with edge attention and softmax attention only'
REFUSALS = {
    # kind -> (layer flags or None for the good layer, hidden, environment, message)
    'sigmoid': (dict(edge_attention=True, residual=True), 32, {}, ONLY),
    'no_attention': (FLAGS['plain'], 32, {}, ONLY),
    'edge_residual': (dict(FLAGS['soft'], edge_residual=True), 32, {}, 'edge_residual layers are not supported'),
    'h16': (FLAGS['soft'], 16, {}, 'needs the MFMA edge kernel'),
    'generic': (None, 32, {'PVS_EGNN_KERNELS': 'generic'}, 'needs the MFMA edge kernel'),
    'alias': (None, 32, {}, 'x_out must not alias x'),
    'workspace': (None, 32, {}, 'workspace too small'),
}
GOOD = (3, 32, 'soft-full')


def _call(d, entry, pg_base, pg, bases, **kw):
    if entry == 'edge_stats':
        return d.edge_stats(pg_base, **{k: v for k, v in kw.items() if k == 'ws_bytes'})
    return d.partial(pg, bases, att=entry == 'fwd_partial_att', **kw)


@pytest.mark.parametrize('kind,entry', [(k, e) for k in REFUSALS for e in ENTRIES
                                        if (k, e) != ('alias', 'edge_stats')])      # (that entry has no x_out)
def test_refusals_leave_the_outputs_and_the_next_call_alone(kind, entry):
    """Non-zero return, pvs_last_error() set, every output at its sentinel, and the valid call after it gives the bits of
    the valid call before it."""
    flags, hid, env, message = REFUSALS[kind]
    p = spc.problem(*GOOD)
    with _environment():
        good = _device(p)
        base_pg, pg, bases = good.base_graph(), good.partial_graph(), good.reference_bases(p)
        rc, before = _call(good, entry, base_pg, pg, bases)
        assert rc == 0, good.error()
        if flags is None:
            bad, bad_bases = good, bases
        else:
            h0 = torch.randn((p.case.n_nodes, hid), generator=torch.Generator().manual_seed(3))
            bad = SoftDevice(p.case, _new_layer(3, hid, flags, pc.LAYER_SEED), h0)
            bad_bases = (torch.zeros((bad.n, hid + 4), device='cuda'),) + tuple(bases[1:])
        x_before = bad.x.clone()
        with _environment(env=env):
            if kind == 'workspace':
                # what the entry needs is what it says it needs: one byte less is refused, exactly that much is enough
                rc, out = _call(bad, entry, base_pg, pg, bad_bases, ws_bytes=0)
                _assert_refused(bad, rc, out, message)
                need = int(re.search(r'workspace too small \(0 < (\d+)\)', bad.error()).group(1))
                n_edges = (base_pg if entry == 'edge_stats' else pg).c.n_edges
                assert 0 < need <= bad.workspace(n_edges)[1]
                rc, out = _call(bad, entry, base_pg, pg, bad_bases, ws_bytes=need - 1)
                _assert_refused(bad, rc, out, message)
                assert f'({need - 1} < {need})' in bad.error()
                rc, after = _call(good, entry, base_pg, pg, bases, ws_bytes=need)
            else:
                rc, out = _call(bad, entry, base_pg, pg, bad_bases, **({'alias_x': True} if kind == 'alias' else {}))
                _assert_refused(bad, rc, out, message, x_before)
        if kind != 'workspace':
            rc, after = _call(good, entry, base_pg, pg, bases)
    assert rc == 0, good.error()
    _same_bits({k: v.cpu().numpy() for k, v in before.items()}, {k: v.cpu().numpy() for k, v in after.items()})


def test_workspace_mode_3_is_mode_2_plus_a_float_per_node():
    """(What modes 0 to 2 return is pinned by the tests of the entries they size.)"""
    p = spc.problem(*GOOD)
    d = _device(p)
    n, e = d.n, d.n_part
    mode2, mode3 = (d.lib.pvs_egnn_layer_workspace_bytes(C.byref(d.desc), n, e, mode) for mode in (2, 3))
    assert mode2 + 4 * n <= mode3 <= mode2 + 4 * n + 512
