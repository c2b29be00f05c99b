"""The partial first layer of the screens, per row, against the fp64 oracle: pvs_egnn_layer_edge_sums,
pvs_egnn_layer_fwd_partial / _partial_att (k_combine_partial, the raw-xsum branch of the MFMA edge forward) and
pvs_graph_filter_ligand_edges, called through pointvs_amd._lib as screening.py calls them - not through a screen object,
which gates away configurations the entries accept.

Arbiter: oracle.egnn_oracle.egnn_layer in fp64 on the union graph. Bound: tests/_golden.py assert_strict with three fp32
oracle draws (one in list order, two under edge permutations), on each tensor as a whole and on the rows of each kind
(no edges / base only / partial only / both) as tensors of their own. Inputs and references: tests/_partial_cases.py,
pinned on the host by tests/test_partial_cases_host.py (which also shows that a dropped base sum, a partial-only degree
and an early clamp each move the oracle by more than 100 x this bound).

The bases of every cell come from two sources: (a) the fp64 reference sums rounded to fp32 - the partial entry alone -
and (b) pvs_egnn_layer_edge_sums over the base edges - what the screens run; (b)'s sums are held to the reference sums.
"""
import contextlib
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest
import torch

from tests import _partial_cases as pc
from tests._golden import CaseLog
from tests.test_gpu_edge_classes import FAMILY_ENV, FLAGS, _new_layer

pytestmark = pytest.mark.gpu

SENTINEL = -7250.0
ROOM = 777            # edge slots behind the count of a graph whose count lives on the device
PAD_ROWS = 40         # trailing rows outside GraphNorm's statistics
PARTITION_ENV = ('PVS_CHUNK_EDGES', 'PVS_EDGES_PER_WAVE')
ONE_BLOCK = {'PVS_EDGES_PER_WAVE': '4096', 'PVS_CHUNK_EDGES': '256'}      # chunks of 256 edges in earnest: one workgroup


def _cell(A, hid, flags, family='default', ends='base', env=None):
    tag = f'partial-A{A}-H{hid}-{family}-{flags}-ends_{ends}'
    if env:
        tag += '-' + '-'.join(f'{k}={v}' for k, v in env.items())
    return pytest.param(dict(A=A, hid=hid, flags=flags, family=family, ends=ends, env=env or {}, tag=tag), id=tag)


THREE = ('plain', 'full-', 'gated-')


def _cells():
    out = [_cell(3, 32, flags) for flags in pc.flag_sets()]
    out += [_cell(3, 64, flags) for flags in THREE]
    out += [_cell(3, hid, flags, 'exact') for hid in (32, 64) for flags in THREE]
    out += [_cell(A, 32, flags) for A in (0, 2) for flags in ('plain', 'full-')]
    out += [_cell(5, hid, flags) for hid in (32, 64) for flags in ('plain', 'full-')]      # H = 64: the 512-thread forward
    # the first and the last node partial-only: rows the base launch never flushes at either end of the range
    out += [_cell(3, hid, flags, ends='partial') for hid in (32, 64) for flags in ('plain', 'full-')]
    # the chunk loop: a nominal cut inside the hub row (pinned on the host)
    out += [_cell(3, hid, 'full-', env=env) for hid in (32, 64) for env in ({'PVS_CHUNK_EDGES': '256'}, ONE_BLOCK)]
    # the wide family (two launches of the edge forward, the messages handed over through the workspace)
    out += [_cell(3, 128, flags) for flags in ('plain', 'full-')]
    return out


CELLS = _cells()


@contextlib.contextmanager
def _environment(family='default', env=None):
    """The family and partition switches are read by the library at every call (edge_dispatch.h); whatever the cell does
    not set is unset."""
    want = dict(FAMILY_ENV[family], **(env or {}))
    names = set(want) | set(PARTITION_ENV) | {k for f in FAMILY_ENV.values() for k in f}
    old = {k: os.environ.pop(k, None) for k in names}
    os.environ.update(want)
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).cuda().contiguous()


def _sentinel(*shape):
    return torch.full(shape, SENTINEL, dtype=torch.float32, device='cuda')


def _untouched(t):
    return bool((t == SENTINEL).all())


class Device:
    """A layer, node inputs and a case's two graphs on the device, `pad` rows without edges appended."""

    def __init__(self, case, layer, h0, pad=0):
        from pointvs_amd import _lib
        self._lib, self.lib = _lib, _lib.lib()
        self.case, self.pad, self.n = case, pad, case.n_nodes + pad
        self.layer = layer.cuda()
        self.hid, self.A = layer.hidden_nf, layer.edges_in_d
        self.desc = _lib.PvsLayerDesc(*self.layer._desc())
        self.params = [None if t is None else t.detach().float().contiguous() for t in self.layer._params()]
        self.pstruct = _lib.PvsLayerParams(*[_lib.ptr(t) for t in self.params])
        gen = torch.Generator().manual_seed(99)
        self.h = torch.cat([h0, torch.randn((pad, self.hid), generator=gen)]).cuda().contiguous()
        self.x = torch.cat([case.pos, torch.randn((pad, 3), generator=gen)]).cuda().contiguous()
        self.n_part = int(case.part_index.shape[1])
        self.eatt, self.natt = bool(self.layer.edge_attention), bool(self.layer.node_attention)

    # ---- graphs ----
    def base_graph(self):
        from pointvs_amd.graph import prepare_graph
        c = self.case
        pg = prepare_graph(c.base_index.cuda(), None if c.base_attr is None else c.base_attr.cuda(), self.n,
                           need_backward=False)
        pg.check_status()
        return pg

    def partial_graph(self, room=0, norm_rows=None):
        """The case's partial list as it stands (it is CSR-sorted). room > 0: the count on the device and `room` further
        edge slots, filled with in-range edges of the hub row; norm_rows: PvsGraph.n_norm_rows_dev."""
        from pointvs_amd.graph import PreparedGraph
        c, e = self.case, self.n_part
        row, col = c.part_index[0].numpy(), c.part_index[1].numpy()
        et = None if c.part_etype is None else c.part_etype.numpy()
        rowptr = np.searchsorted(row, np.arange(self.n + 1))
        if room:
            ligand = np.flatnonzero(c.bp.numpy() == 0)
            row = np.concatenate([row, np.full(room, pc.HUB)])
            col = np.concatenate([col, ligand[np.arange(room) % ligand.size]])
            et = None if et is None else np.concatenate([et, np.arange(room) % c.A])
        t = dict(rowptr=_i32(rowptr), row=_i32(row), col=_i32(col), inv_deg=torch.ones(self.n, device='cuda'))
        if et is not None:
            t['etype'] = torch.as_tensor(et, dtype=torch.uint8).cuda()
        word = None
        if room:
            word = t['count'] = _i32([e])
        pg = PreparedGraph.over_buffers(self.n, e + room, t, word, n_edge_attr=c.A)
        if norm_rows is not None:
            t['norm_rows'] = _i32([norm_rows])
            pg.c.n_norm_rows_dev = t['norm_rows'].data_ptr()
        return pg

    # ---- bases ----
    def _rows(self, a):
        a = torch.as_tensor(a, dtype=torch.float32)
        return torch.cat([a, a.new_zeros((self.pad,) + tuple(a.shape[1:]))]).cuda().contiguous()

    def reference_bases(self, p):
        """(a): the fp64 reference sums over the base list, rounded to fp32."""
        return tuple(self._rows(p.ref64[k]) for k in ('base_magg', 'base_xsum', 'base_deg'))

    def summed_bases(self, base_pg):
        """(b): pvs_egnn_layer_edge_sums over the base graph, the degrees from its rowptr (screening.py)."""
        rc, out = self.edge_sums(base_pg)
        assert rc == 0, self.error()
        rowptr = base_pg.t['rowptr']
        return out['magg'], out['xsum'], (rowptr[1:] - rowptr[:-1]).float().contiguous()

    # ---- the three entries ----
    def error(self):
        return self.lib.pvs_last_error().decode(errors='replace')

    def workspace(self, n_edges):
        size = self.lib.pvs_egnn_layer_workspace_bytes(C.byref(self.desc), self.n, n_edges, 2)
        return torch.empty(size, dtype=torch.uint8, device='cuda'), size

    def edge_sums(self, pg, ws_bytes=None):
        ptr = self._lib.ptr
        ws, size = self.workspace(pg.c.n_edges)
        out = dict(magg=_sentinel(self.n, self.hid), xsum=_sentinel(self.n, 3))
        rc = self.lib.pvs_egnn_layer_edge_sums(
            C.byref(self.desc), C.byref(pg.c), C.byref(self.pstruct), ptr(self.h), ptr(self.x), ptr(out['magg']),
            ptr(out['xsum']), ptr(ws), size if ws_bytes is None else ws_bytes, self._lib.stream(self.h.device))
        torch.cuda.synchronize()
        return rc, out

    def partial(self, pg, bases, att=False, ws_bytes=None, alias_x=False):
        """pvs_egnn_layer_fwd_partial (att: _partial_att with an att_out of the graph's room + 5) into outputs that hold
        the sentinel -> (return code, {h_out, x_out, natt, att})."""
        ptr = self._lib.ptr
        room = pg.c.n_edges
        ws, size = self.workspace(room)
        saved = torch.empty(self.lib.pvs_egnn_layer_saved_floats(C.byref(self.desc), self.n, room), device='cuda')
        out = dict(h_out=_sentinel(self.n, self.hid), x_out=self.x if alias_x else _sentinel(self.n, 3))
        if self.natt:       # (NULL without node attention, as the screens pass it)
            out['natt'] = _sentinel(self.n)
        args = [C.byref(self.desc), C.byref(pg.c), C.byref(self.pstruct), ptr(self.h), ptr(self.x)]
        args += [ptr(b) for b in bases] + [ptr(out['h_out']), ptr(out['x_out']), ptr(out.get('natt'))]
        name = 'pvs_egnn_layer_fwd_partial'
        if att:
            out['att'] = _sentinel(room + 5)
            args.append(ptr(out['att']))
            name += '_att'
        args += [ptr(saved), ptr(ws), size if ws_bytes is None else ws_bytes, self._lib.stream(self.h.device)]
        rc = getattr(self.lib, name)(*args)
        torch.cuda.synchronize()
        return rc, out

    def layer_outputs(self, pg, bases):
        """The layer through the partial entries, as numpy: h_out, x_out, natt (node attention), att over the first
        n_part edges (edge attention; the _att entry, whose h_out / x_out / natt must be the plain entry's bits)."""
        rc, out = self.partial(pg, bases)
        assert rc == 0, self.error()
        if self.eatt:
            rc, with_att = self.partial(pg, bases, att=True)
            assert rc == 0, self.error()
            att = with_att.pop('att')
            assert _untouched(att[self.n_part:]), 'att_out written behind the edge count'
            for k in out:
                assert torch.equal(out[k], with_att[k]), f'{k} differs between the entry with and without att_out'
            out['att'] = att[:self.n_part]
        return {k: v.cpu().numpy() for k, v in out.items()}


def _device(p, pad=0):
    return Device(p.case, p.new_layer(), p.h0, pad)


def _same_bits(a, b):
    assert set(a) == set(b)
    differing = [k for k in a if np.asarray(a[k]).tobytes() != np.asarray(b[k]).tobytes()]
    assert not differing, differing


def _expected_keys(p):
    return {'h_out', 'x_out'} | ({'natt'} if p.kw['node_attention'] else set()) | ({'att'} if p.kw['edge_attention'] else set())


def _check_sums(p, d, sums, tag, log):
    """(b)'s magg and xsum against the reference sums; rows without base edges hold exactly 0."""
    got = {'base_magg': sums[0].cpu().numpy(), 'base_xsum': sums[1].cpu().numpy()}
    p.check(got, tag, log, n_rows=p.case.n_nodes)
    empty = np.flatnonzero(np.concatenate([p.ref64['base_deg'], np.zeros(d.pad)]) == 0)
    assert len(empty) >= 30 + d.pad
    for k, v in got.items():
        if v[empty].any():
            log.failures.append(f'{tag} {k}: a row without base edges is not 0.0')
    assert np.array_equal(sums[2].cpu().numpy()[:p.case.n_nodes], p.ref64['base_deg'])
    if not p.kw['update_coords'] and got['base_xsum'].any():
        log.failures.append(f'{tag} base_xsum: not 0.0 without update_coords')


def _run_cell(p, d, pg, tag, log, n_rows=None):
    """Both sources of the bases through the partial entries, every tensor under the strict bound -> source (a)'s outputs."""
    sums = d.summed_bases(d.base_graph())
    _check_sums(p, d, sums, f'{tag} edge_sums', log)
    first = None
    for source, bases in (('a', d.reference_bases(p)), ('b', sums)):
        got = d.layer_outputs(pg, bases)
        assert set(got) == _expected_keys(p)
        p.check(got, f'{tag} ({source})', log, n_rows=n_rows)
        if not p.kw['update_coords']:
            assert got['x_out'].tobytes() == d.x.cpu().numpy().tobytes(), 'x_out is not x without update_coords'
        first = got if first is None else first
    return first


@pytest.mark.parametrize('cell', CELLS)
def test_partial_layer_matches_the_fp64_oracle(cell):
    """h_out, x_out, node_att_out and att_out over the partial graph of one first layer through the partial entries, with
    the bases from the reference (a) and from pvs_egnn_layer_edge_sums (b); (b)'s magg / xsum themselves."""
    p = pc.problem(cell['A'], cell['hid'], cell['flags'], cell['ends'])
    log = CaseLog(cell['tag'])
    with _environment(cell['family'], cell['env']):
        d = _device(p)
        _run_cell(p, d, d.partial_graph(), cell['tag'], log)
    log.finish()


@pytest.mark.parametrize('hid,flags', [(32, 'plain'), (32, 'full-'), (64, 'full-'), (128, 'full-')])
def test_device_side_edge_count_gives_the_host_count_bits(hid, flags):
    """n_edges = a capacity of E + 777, the count in n_edges_dev, the slots behind it full of edges of the hub row: the
    chunk plan is remade from the count (edge_dispatch.h), so every output has the bits of the host-count call, and
    att_out behind the count keeps its sentinel (checked in layer_outputs)."""
    p = pc.problem(3, hid, flags)
    with _environment():
        d = _device(p)
        bases = d.reference_bases(p)
        host = d.layer_outputs(d.partial_graph(), bases)
        dev = d.layer_outputs(d.partial_graph(room=ROOM), bases)
        # the same for the sums: the partial list as a graph of its own
        rc_h, sums_h = d.edge_sums(d.partial_graph())
        rc_d, sums_d = d.edge_sums(d.partial_graph(room=ROOM))
    assert rc_h == 0 and rc_d == 0
    _same_bits(host, dev)
    _same_bits({k: v.cpu().numpy() for k, v in sums_h.items()}, {k: v.cpu().numpy() for k, v in sums_d.items()})


@pytest.mark.parametrize('hid,flags', [(32, 'gn'), (64, 'full-')])
def test_graphnorm_over_a_device_row_count(hid, flags):
    """40 trailing rows without edges as padding, n_norm_rows_dev = N - 40: the leading rows are the layer on the
    (N - 40)-row problem."""
    p = pc.problem(3, hid, flags)
    tag = f'partial-A3-H{hid}-default-{flags}-norm_rows'
    log = CaseLog(tag)
    with _environment():
        d = _device(p, pad=PAD_ROWS)
        assert d.n == p.case.n_nodes + 40 and p.kw['graphnorm']
        _run_cell(p, d, d.partial_graph(norm_rows=p.case.n_nodes), tag, log, n_rows=p.case.n_nodes)
    log.finish()


@pytest.mark.parametrize('cell', [_cell(3, 32, 'full-'), _cell(3, 64, 'full-'), _cell(5, 64, 'plain'), _cell(3, 128, 'full-'),
                                  _cell(3, 32, 'full-', 'exact'), _cell(3, 32, 'full-', env=ONE_BLOCK)])
def test_the_three_entries_are_bitwise_reproducible(cell):
    p = pc.problem(cell['A'], cell['hid'], cell['flags'])
    with _environment(cell['family'], cell['env']):
        d = _device(p)
        base_pg, pg, bases = d.base_graph(), d.partial_graph(), d.reference_bases(p)
        for run in (lambda: d.edge_sums(base_pg), lambda: d.partial(pg, bases), lambda: d.partial(pg, bases, att=True)):
            (rc1, first), (rc2, second) = run(), run()
            assert rc1 == 0 and rc2 == 0, d.error()
            _same_bits({k: v.cpu().numpy() for k, v in first.items()}, {k: v.cpu().numpy() for k, v in second.items()})


# ---- refusals -----------------------------------------------------------------------------------------------------------
ENTRIES = ('edge_sums', 'fwd_partial', 'fwd_partial_att')
REFUSALS = {
    # kind -> (layer flags or None for the good layer, hidden, environment, message)
    'softmax': (FLAGS['soft'], 32, {}, 'softmax attention is not supported'),
    'edge_residual': (FLAGS['full'], 32, {}, 'edge_residual layers are not supported'),
    'h16': ({}, 16, {}, 'needs the MFMA edge kernel'),
    'generic': (None, 32, {'PVS_EGNN_KERNELS': 'generic'}, 'needs the MFMA edge kernel'),
    'alias': (None, 32, {}, 'x_out must not alias x'),
    'workspace': (None, 32, {}, 'workspace too small'),
}
GOOD = (3, 32, 'full-')


def _call(d, entry, pg_base, pg, bases, **kw):
    if entry == 'edge_sums':
        return d.edge_sums(pg_base, **{k: v for k, v in kw.items() if k == 'ws_bytes'})
    return d.partial(pg, bases, att=entry == 'fwd_partial_att', **kw)


def _assert_refused(d, rc, out, message, x_before=None):
    assert rc != 0, 'the call was accepted'
    assert message in d.error(), d.error()
    for k, v in out.items():
        if v is d.x:
            assert torch.equal(v, x_before), 'x changed by a refused call'
        else:
            assert _untouched(v), f'{k} written by a refused call'


@pytest.mark.parametrize('kind,entry', [(k, e) for k in REFUSALS for e in ENTRIES
                                        if (k, e) != ('alias', 'edge_sums')])      # (that entry has no x_out)
def test_refusals_leave_the_outputs_and_the_next_call_alone(kind, entry):
    """Non-zero return, pvs_last_error() set, every output at its sentinel, and the valid call after it gives the bits of
    the valid call before it (which is held to the oracle by the cells above)."""
    flags, hid, env, message = REFUSALS[kind]
    p = pc.problem(*GOOD)
    with _environment():
        good = _device(p)
        base_pg, pg, bases = good.base_graph(), good.partial_graph(), good.reference_bases(p)
        rc, before = _call(good, entry, base_pg, pg, bases)
        assert rc == 0, good.error()
        if flags is None:
            bad, bad_bases = good, bases
        else:
            h0 = torch.randn((p.case.n_nodes, hid), generator=torch.Generator().manual_seed(3))
            bad = Device(p.case, _new_layer(3, hid, flags, pc.LAYER_SEED), h0)
            bad_bases = (torch.zeros((bad.n, hid), device='cuda'),) + tuple(bases[1:])
        x_before = bad.x.clone()
        with _environment(env=env):
            if kind == 'workspace':
                # what the entry needs is what it says it needs: one byte less is refused, exactly that much is enough
                rc, out = _call(bad, entry, base_pg, pg, bad_bases, ws_bytes=0)
                _assert_refused(bad, rc, out, message)
                need = int(re.search(r'workspace too small \(0 < (\d+)\)', bad.error()).group(1))
                n_edges = (base_pg if entry == 'edge_sums' else pg).c.n_edges
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


# ---- pvs_graph_filter_ligand_edges ----------------------------------------------------------------------------------------
FILTER_DEGREES = (0, 1, 63, 64, 65, 130)
N_LIGAND = 12
# receptor rows whose only ligand contact sits at this position of the row (the kernel: one wave per row, 64 edges a step)
CONTACT_AT = {'lane 0': 0, 'lane 63': 63, 'second step': 64, 'no contact': None}
CANARY = -99


@functools.lru_cache(maxsize=None)
def _filter_case(n, A=3, seed=77):
    """A row-sorted edge list over n nodes (the first 12 ligand atoms) -> (row, col, etype or None, special) as numpy;
    special: [(row id, degree, edges the filter keeps)] of the rows built on purpose, the others have 0 ... 20 random
    edges."""
    rng = np.random.default_rng(seed)
    ligand, receptor = np.arange(N_LIGAND), np.arange(N_LIGAND, n)
    plan = {i: (d, 'ligand') for i, d in enumerate(FILTER_DEGREES)}
    node = N_LIGAND
    for what, at in CONTACT_AT.items():
        for d in FILTER_DEGREES:
            if at is None or at < d:
                plan[node] = (d, what)
                node += 1
    assert node == N_LIGAND + 16 and node < n
    rows, cols, special = [], [], []
    for i in range(n):
        if i in plan:
            d, what = plan[i]
            c = rng.choice(receptor[receptor != i], size=d)
            if what == 'ligand':
                c = rng.choice(np.arange(n)[np.arange(n) != i], size=d)
            elif CONTACT_AT[what] is not None:
                c[CONTACT_AT[what]] = rng.choice(ligand)
            special.append((i, d, d if what == 'ligand' else int(CONTACT_AT[what] is not None)))
        else:
            c = rng.choice(np.arange(n)[np.arange(n) != i], size=int(rng.integers(0, 21)))
        rows.append(np.full(c.size, i))
        cols.append(c)
    row, col = np.concatenate(rows), np.concatenate(cols)
    et = rng.integers(0, A, size=row.size) if A else None
    return row.astype(np.int64), col.astype(np.int64), et, special


def _prepared(row, col, et, n, A):
    from pointvs_amd.graph import prepare_graph
    ei = torch.as_tensor(np.vstack([row, col])).cuda()
    ea = None if et is None else torch.nn.functional.one_hot(torch.as_tensor(et), A).cuda()
    pg = prepare_graph(ei, ea, n, need_backward=False)
    pg.check_status()
    assert np.array_equal(pg.t['col'].cpu().numpy()[:row.size], col), 'a row-sorted list is its own CSR'
    return pg


def _filter(pg, bp, capacity, with_etype=True):
    """-> (return code, status, rowptr_out, row, col, etype) with canaries in the three edge arrays (3 slots more than
    the capacity)."""
    from pointvs_amd import _lib
    lib, n = _lib.lib(), pg.n_nodes
    room = max(capacity, 0) + 3
    rowptr = torch.full((n + 1,), CANARY, dtype=torch.int32, device='cuda')
    row, col = (torch.full((room,), CANARY, dtype=torch.int32, device='cuda') for _ in range(2))
    etype = torch.full((room,), 0xEE, dtype=torch.uint8, device='cuda')
    status = torch.full((1,), CANARY, dtype=torch.int32, device='cuda')
    size = lib.pvs_graph_filter_workspace_bytes(n)
    ws = torch.empty(size, dtype=torch.uint8, device='cuda')
    bp = torch.as_tensor(bp, dtype=torch.uint8).cuda().contiguous()
    rc = lib.pvs_graph_filter_ligand_edges(
        C.byref(pg.c), _lib.ptr(bp), capacity, _lib.ptr(rowptr), _lib.ptr(row), _lib.ptr(col),
        _lib.ptr(etype) if with_etype else None, _lib.ptr(status), _lib.ptr(ws), size, _lib.stream(bp.device))
    torch.cuda.synchronize()
    return rc, int(status.item()), rowptr.cpu().numpy(), row.cpu().numpy(), col.cpu().numpy(), etype.cpu().numpy()


def _numpy_filter(row, col, et, bp, n):
    keep = (bp[row] == 0) | (bp[col] == 0)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(row[keep], minlength=n))])
    return rowptr, row[keep], col[keep], (None if et is None else et[keep])


def _ligand_marks(which, n):
    bp = np.ones(n, dtype=np.uint8)
    if which == 'mixed':
        bp[:N_LIGAND] = 0
    elif which == 'all ligand':
        bp[:] = 0
    return bp


@pytest.mark.parametrize('which', ['mixed', 'no ligand', 'all ligand'])
@pytest.mark.parametrize('n', [148, 150, 151])
def test_ligand_filter_equals_the_numpy_filter(n, which):
    """rowptr_out, row, col and etype of pvs_graph_filter_ligand_edges, exact, at a capacity equal to the count (status
    0, nothing behind the count written), with and without etype_out; four rows per block, so n = 150 and 151 end in a
    block that is not full."""
    row, col, et, special = _filter_case(n)
    bp = _ligand_marks(which, n)
    pg = _prepared(row, col, et, n, 3)
    want_ptr, want_row, want_col, want_et = _numpy_filter(row, col, et, bp, n)
    count = int(want_ptr[-1])
    if which == 'mixed':
        degree = np.bincount(row, minlength=n)
        assert [(i, int(degree[i]), int(want_ptr[i + 1] - want_ptr[i])) for i, _, _ in special] == special
        assert sorted({d for _, d, _ in special}) == list(FILTER_DEGREES) and len(special) == 22
    assert count == {'mixed': count, 'no ligand': 0, 'all ligand': row.size}[which] and (which != 'mixed' or 0 < count < row.size)
    for with_etype in (True, False):
        rc, status, rowptr, r, c, t = _filter(pg, bp, count, with_etype)
        assert rc == 0 and status == 0
        assert np.array_equal(rowptr, want_ptr)
        assert np.array_equal(r[:count], want_row) and np.array_equal(c[:count], want_col)
        assert (r[count:] == CANARY).all() and (c[count:] == CANARY).all()
        if with_etype:
            assert np.array_equal(t[:count], want_et) and (t[count:] == 0xEE).all()
        else:
            assert (t == 0xEE).all()


def test_ligand_filter_reports_a_capacity_one_edge_short():
    n = 150
    row, col, et, _ = _filter_case(n)
    bp = _ligand_marks('mixed', n)
    want_ptr = _numpy_filter(row, col, et, bp, n)[0]
    count = int(want_ptr[-1])
    rc, status, rowptr, r, c, t = _filter(_prepared(row, col, et, n, 3), bp, count - 1)
    assert rc == 0 and status == 4, 'status bit 2: the edges do not fit'
    assert np.array_equal(rowptr, want_ptr), 'rowptr_out keeps the true counts'
    assert (r == CANARY).all() and (c == CANARY).all() and (t == 0xEE).all(), 'nothing is written'


def test_ligand_filter_refuses_edge_classes_of_a_graph_without_them():
    from pointvs_amd import _lib
    n = 150
    row, col, _, _ = _filter_case(n, A=0)
    pg = _prepared(row, col, None, n, 0)
    bp = _ligand_marks('mixed', n)
    rc, status, rowptr, r, c, t = _filter(pg, bp, row.size)
    assert rc != 0 and 'graph has no edge classes' in _lib.lib().pvs_last_error().decode()
    assert status == CANARY and (rowptr == CANARY).all() and (r == CANARY).all() and (t == 0xEE).all()
    want_ptr, want_row, want_col, _ = _numpy_filter(row, col, None, bp, n)
    rc, status, rowptr, r, c, t = _filter(pg, bp, row.size, with_etype=False)
    count = int(want_ptr[-1])
    assert rc == 0 and status == 0 and np.array_equal(rowptr, want_ptr)
    assert np.array_equal(r[:count], want_row) and np.array_equal(c[:count], want_col)


@pytest.mark.parametrize('hid,flags', [(32, 'plain'), (64, 'full-')])
def test_filtered_union_graph_reproduces_the_partial_cell(hid, flags):
    """The case's split is the filter's: the ligand-touching edges of the prepared union graph are the partial list, and
    the filter's arrays, handed to the partial entries with n_edges_dev = rowptr_out + N, give the bits of the cell that
    was handed the list itself."""
    from pointvs_amd import _lib
    from pointvs_amd.graph import PreparedGraph, prepare_graph
    p = pc.problem(3, hid, flags)
    c, n = p.case, p.case.n_nodes
    ei, ea = pc.union(c)
    with _environment():
        d = _device(p)
        full = prepare_graph(ei.cuda(), ea.cuda(), n, need_backward=False)
        full.check_status()
        capacity = d.n_part + ROOM
        lib = _lib.lib()
        t = dict(rowptr=torch.zeros(n + 1, dtype=torch.int32, device='cuda'), inv_deg=torch.ones(n, device='cuda'),
                 row=torch.zeros(capacity, dtype=torch.int32, device='cuda'),
                 col=torch.zeros(capacity, dtype=torch.int32, device='cuda'),
                 etype=torch.zeros(capacity, dtype=torch.uint8, device='cuda'),
                 status=torch.zeros(1, dtype=torch.int32, device='cuda'))
        size = lib.pvs_graph_filter_workspace_bytes(n)
        ws = torch.empty(size, dtype=torch.uint8, device='cuda')
        bp = c.bp.cuda().contiguous()
        _lib.check(lib.pvs_graph_filter_ligand_edges(
            C.byref(full.c), _lib.ptr(bp), capacity, _lib.ptr(t['rowptr']), _lib.ptr(t['row']), _lib.ptr(t['col']),
            _lib.ptr(t['etype']), _lib.ptr(t['status']), _lib.ptr(ws), size, _lib.stream(bp.device)),
            'pvs_graph_filter_ligand_edges')
        torch.cuda.synchronize()
        e = d.n_part
        assert int(t['status'].item()) == 0 and int(t['rowptr'][n].item()) == e
        assert np.array_equal(t['row'].cpu().numpy()[:e], c.part_index[0].numpy())
        assert np.array_equal(t['col'].cpu().numpy()[:e], c.part_index[1].numpy())
        assert np.array_equal(t['etype'].cpu().numpy()[:e], c.part_etype.numpy())
        filtered = PreparedGraph.over_buffers(n, capacity, t, t['rowptr'][n:], n_edge_attr=3)
        bases = d.reference_bases(p)
        _same_bits(d.layer_outputs(d.partial_graph(), bases), d.layer_outputs(filtered, bases))
