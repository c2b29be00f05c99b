"""GraphNorm per node segment (the layer flag PVS_GRAPHNORM_SEGMENTS, PreparedGraph.set_norm_segments), on the GPU.

Operator level (PF.graphnorm_stats_segments -> pvs_graphnorm_stats_segments): every segment's [2H] statistics equal, bit
for bit, PF.graphnorm_stats (pvs_graphnorm_stats_rows) on that segment's rows alone - at every edge of the row partition
(0, 1, 2, 127 ... 257 rows, and 65,537 rows where the block count clamps), on the float4 and on the scalar route, with NaN
in the rows that belong to no segment, with table entries outside [0, N_cap], and twice in a row.

Layer level (EGNNLayer.forward_prepared, the one-call stack and one partial-layer entry on a PreparedGraph with
set_norm_segments): a batch of four leave-out copies of the 207-node graph of tests/test_gpu_graphnorm_rows.py, an empty
segment among them and 40 padding rows behind; every copy's rows against the fp64 oracle ON THAT COPY ALONE at the strict
parity bound (tests/_golden.assert_strict) - which the same batch under whole-batch statistics (set_norm_rows) must miss.
Then: the table is read when the kernels run (one captured forward, three tables), and what is refused.
"""
import ctypes as C
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from tests._golden import CaseLog, assert_strict, edge_permutations, strict_margin
from tests.test_gpu_edge_classes import _new_layer
from tests.test_gpu_graphnorm_rows import LAYER_FLAGS, N_REAL, _graph207

pytestmark = pytest.mark.gpu

WIDTHS = (16, 32, 64, 128, 30)          # 30: the scalar route (C % 4 != 0)
LENGTHS = (0, 1, 2, 127, 128, 129, 255, 256, 257)
FRONT, BEHIND = 5, 7                    # rows of no segment in front of the first and behind the last one
LONG = 65537                            # ceil(65537 / 128) = 513 blocks: clamped to 512


def _bits(t):
    return t.detach().cpu().numpy().view(np.uint32)


def _table(values):
    return torch.tensor(values, dtype=torch.int32, device='cuda')


@functools.lru_cache(maxsize=None)
def _base(hidden):
    """(values [LONG + 3, H] on the device, mean_scale): standard normal columns around per-column offsets; built once
    per width, never written."""
    gen = torch.Generator().manual_seed(177 + hidden)
    y = torch.randn(LONG + 3, hidden, generator=gen) + 0.5 * torch.randn(hidden, generator=gen)
    return y.cuda(), (0.5 + torch.rand(hidden, generator=gen)).cuda()


def _edges_table():
    ptr = [FRONT]
    for n in LENGTHS:
        ptr.append(ptr[-1] + n)
    return ptr, ptr[-1] + BEHIND


def _alone(y, ms, start, n):
    """What pvs_graphnorm_stats_rows gives on the rows [start, start + n) alone (n = 0: zeros)."""
    from pointvs_amd import functional as PF
    if n == 0:
        return torch.zeros(2 * y.shape[1], device='cuda')
    return PF.graphnorm_stats(y[start:start + n], ms)


# ---- the operator ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('hidden', WIDTHS)
def test_every_segment_has_the_bits_of_the_rows_operator_on_its_rows_alone(hidden):
    from pointvs_amd import functional as PF
    y_all, ms = _base(hidden)
    ptr, n_cap = _edges_table()
    y = y_all[:n_cap].clone()
    y[:FRONT] = float('nan')
    y[n_cap - BEHIND:] = float('nan')
    stats = PF.graphnorm_stats_segments(y, ms, _table(ptr))
    assert stats.shape == (len(LENGTHS), 2 * hidden) and stats.dtype == torch.float32
    assert torch.isfinite(stats).all()
    for s, n in enumerate(LENGTHS):
        assert np.array_equal(_bits(stats[s]), _bits(_alone(y, ms, ptr[s], n))), (hidden, s, n)
    assert not _bits(stats[0]).any()          # the empty segment: +0.0, nothing divided by 0
    # the same call again, into a poisoned output: the same bits
    out = torch.full_like(stats, float('nan'))
    assert PF.graphnorm_stats_segments(y, ms, _table(ptr), out=out) is out
    assert np.array_equal(_bits(out), _bits(stats))


@pytest.mark.parametrize('hidden', WIDTHS)
def test_one_long_segment_where_the_block_count_clamps(hidden):
    from pointvs_amd import functional as PF
    y_all, ms = _base(hidden)
    y = y_all.clone()
    y[LONG:] = float('nan')
    stats = PF.graphnorm_stats_segments(y, ms, _table([0, LONG]))
    assert torch.isfinite(stats).all()
    assert np.array_equal(_bits(stats[0]), _bits(_alone(y, ms, 0, LONG))), hidden
    assert np.array_equal(_bits(PF.graphnorm_stats_segments(y, ms, _table([0, LONG]))), _bits(stats))


@pytest.mark.parametrize('hidden', [32, 30])
def test_table_entries_outside_the_rows_are_clamped(hidden):
    """Entries above N_cap and below 0 (the table itself is valid device memory): clamped to [0, N_cap], a segment that
    ends in front of its start has length 0."""
    from pointvs_amd import functional as PF
    y_all, ms = _base(hidden)
    n_cap = 700
    y = y_all[:n_cap].contiguous()
    for ptr, want in (([-7, 129, 129, n_cap + 1000], [(0, 129), (129, 0), (129, n_cap - 129)]),
                      ([-2 ** 31, -1, 300, 2 ** 31 - 1], [(0, 0), (0, 300), (300, n_cap - 300)]),
                      ([n_cap + 5, n_cap + 9, 2 ** 30], [(n_cap, 0), (n_cap, 0)]),
                      ([300, 100, 500], [(300, 0), (100, 400)])):
        stats = PF.graphnorm_stats_segments(y, ms, _table(ptr))
        assert torch.isfinite(stats).all()
        for s, (a, n) in enumerate(want):
            assert np.array_equal(_bits(stats[s]), _bits(_alone(y, ms, a, n))), (hidden, ptr, s)


def test_the_operator_refuses_what_it_cannot_take():
    from pointvs_amd import functional as PF
    y_all, ms = _base(32)
    y = y_all[:64]
    with pytest.raises(ValueError, match='seg_ptr'):
        PF.graphnorm_stats_segments(y, ms, torch.zeros(3, dtype=torch.int64, device='cuda'))
    with pytest.raises(ValueError, match='seg_ptr'):
        PF.graphnorm_stats_segments(y, ms, _table([0]))
    with pytest.raises(TypeError):
        PF.graphnorm_stats_segments(y.double(), ms, _table([0, 64]))
    with pytest.raises(ValueError, match='out must be'):
        PF.graphnorm_stats_segments(y, ms, _table([0, 64]), out=torch.empty(64, device='cuda'))


# ---- the layer -------------------------------------------------------------------------------------------------------
DROPS = (1, 2, 30, 100)          # atoms each leave-out copy lacks: four copies of different sizes
PADDING = 40
DEPTH = 3                        # layers of the stack case


@functools.lru_cache(maxsize=None)
def _copies():
    """The four copies of the 207-node graph (induced subgraphs, nodes renumbered), their union with the copies' rows one
    behind the other and PADDING rows without edges behind them, and the segment table with an EMPTY segment between the
    second and the third copy."""
    g = _graph207()
    gen = torch.Generator().manual_seed(20261021)
    parts, ptr, eis, eas, at = [], [0], [], [], 0
    for k, n_drop in enumerate(DROPS):
        keep = torch.ones(N_REAL, dtype=torch.bool)
        keep[torch.randperm(N_REAL, generator=gen)[:n_drop]] = False
        new_id = torch.cumsum(keep.long(), 0) - 1
        live = keep[g.edge_index[0]] & keep[g.edge_index[1]]
        ei = new_id[g.edge_index[:, live]]
        parts.append(SimpleNamespace(keep=keep, edge_index=ei, edge_attr=g.edge_attr[live], n=int(keep.sum())))
        eis.append(ei + at)
        eas.append(g.edge_attr[live])
        at += parts[-1].n
        ptr.append(at)
        if k == 1:
            ptr.append(at)          # the empty segment
    return SimpleNamespace(parts=parts, ptr=ptr, n_real=at, n_cap=at + PADDING, edge_index=torch.cat(eis, 1),
                           edge_attr=torch.cat(eas, 0), spans=[(ptr[s], ptr[s + 1] - ptr[s]) for s in (0, 1, 3, 4)])


def _oracle_kwargs(flags):
    from oracle import egnn_oracle as orc
    kw = dict(orc.BUILD_NET_DEFAULTS, residual=True, normalize=False, tanh=False, graphnorm=False)  # EGNNLayer's defaults
    kw.update(flags)
    kw['edge_attention_here'], kw['node_attention_here'] = kw['edge_attention'], kw['node_attention']
    return kw


class _Case:
    """Inputs and per-copy oracle references (fp64, and three fp32 evaluations: the edge list as it is and in two other
    orders) of `depth` GraphNorm layers on the copies: built once per (hid, natt, depth), never written."""

    def __init__(self, hid, natt, depth):
        from oracle import egnn_oracle as orc
        self.hid, self.flags, self.depth = hid, LAYER_FLAGS[natt], depth
        c = _copies()
        g = _graph207()
        self.sds = [{k: v.detach().clone() for k, v in _new_layer(3, hid, self.flags, 11 + 7 * d).state_dict().items()}
                    for d in range(depth)]
        gen = torch.Generator().manual_seed(5 + hid)
        h207 = torch.randn(N_REAL, hid, generator=gen)
        self.h0 = torch.cat([h207[p.keep] for p in c.parts] + [torch.randn(PADDING, hid, generator=gen)])
        self.x0 = torch.cat([g.pos[p.keep] for p in c.parts] + [torch.randn(PADDING, 3, generator=gen)])
        kw = _oracle_kwargs(self.flags)

        def alone(part, a, dtype, perm=None):
            ei, ea = part.edge_index, part.edge_attr
            if perm is not None:
                ei, ea = ei[:, perm], ea[perm]
            h, x = self.h0[a:a + part.n].to(dtype), self.x0[a:a + part.n].to(dtype)
            with torch.no_grad():
                for sd in self.sds:
                    h, x, _, _, _ = orc.egnn_layer({k: v.to(dtype) for k, v in sd.items()}, '', kw, h, ei, x, ea, None)
            return dict(h_out=h.numpy(), x_out=x.numpy())

        self.ref64, self.ref32 = [], []
        for part, (a, n) in zip(c.parts, c.spans):
            assert n == part.n
            self.ref64.append(alone(part, a, torch.float64))
            perms = [None] + edge_permutations(int(part.edge_index.shape[1]), count=2)
            self.ref32.append([alone(part, a, torch.float32, perm) for perm in perms])

    def layers(self):
        out = []
        for d, sd in enumerate(self.sds):
            layer = _new_layer(3, self.hid, self.flags, 11 + 7 * d)
            layer.load_state_dict(sd)
            out.append(layer.cuda())
        return out

    def margins(self, h, x):
        """[(copy, key, err, bound)] of the copies' rows of h [N_cap, H] / x [N_cap, 3] against the oracle on each copy
        alone, by the strict rule."""
        h, x = h.detach().cpu().numpy(), x.detach().cpu().numpy()
        rows = []
        for k, (a, n) in enumerate(_copies().spans):
            for key, value in (('h_out', h[a:a + n]), ('x_out', x[a:a + n])):
                err, bound = strict_margin(value, self.ref64[k][key], [r[key] for r in self.ref32[k]])
                rows.append((k, key, err, bound))
        return rows

    def check(self, h, x, tag):
        log = CaseLog(tag)
        h_np, x_np = h.detach().cpu().numpy(), x.detach().cpu().numpy()
        for k, (a, n) in enumerate(_copies().spans):
            for key, value in (('h_out', h_np[a:a + n]), ('x_out', x_np[a:a + n])):
                assert_strict(value, self.ref64[k][key], [r[key] for r in self.ref32[k]], f'{tag} copy{k} {key}', log=log)
        log.finish()
        pad = h_np[_copies().n_real:]
        assert pad.shape[0] == PADDING and np.all(np.isfinite(pad)), tag      # the padding rows: mean = var = 0, finite


@functools.lru_cache(maxsize=None)
def _case(hid, natt, depth=1):
    return _Case(hid, natt, depth)


def _prepared(norm):
    """The union graph at N_cap rows; norm: 'segments' (the copies' table), 'rows' (whole-batch statistics over the real
    rows, the existing route) or None."""
    from pointvs_amd.graph import prepare_graph
    c = _copies()
    pg = prepare_graph(c.edge_index.cuda(), c.edge_attr.cuda(), c.n_cap, need_backward=False)
    if norm == 'segments':
        table = _table(c.ptr)
        pg.set_norm_segments(table)
        assert pg.norm_segments is table and pg.c.n_norm_rows_dev == table.data_ptr() and pg.c.n_graphs == len(c.ptr) - 1
    elif norm == 'rows':
        pg.set_norm_rows(_table([c.n_real]))
    return pg


def _layer_forward(case, pg):
    with torch.no_grad():
        h, x = case.h0.cuda(), case.x0.cuda()
        for layer in case.layers():
            h, x, _ = layer.forward_prepared(pg, h, x, None, need_m=False)
    torch.cuda.synchronize()
    return h, x


def _stack_forward(case, pg):
    from pointvs_amd import _lib
    from pointvs_amd import functional as PF
    layers = case.layers()
    descs, params, pstructs = [], [], []
    for layer in layers:
        d = layer._desc()
        if pg.norm_segments is not None:
            d = (d[0], d[1], d[2] | _lib.GRAPHNORM_SEGMENTS, d[3])
        p, ps = layer._params_cached()
        descs.append(d)
        params.append(p)
        pstructs.append(ps)
    with torch.no_grad():
        h, x, *_ = PF.egnn_stack(case.h0.cuda(), case.x0.cuda(), pg, PF.StackPlan(descs, params, pstructs))
    torch.cuda.synchronize()
    return h, x


def _partial_forward(case, pg, flags_extra):
    """pvs_egnn_layer_fwd_partial over ALL edges of pg on top of a zero base: the whole layer through the partial-layer
    host path."""
    from pointvs_amd import _lib
    lib = _lib.lib()
    (layer,) = case.layers()
    d = layer._desc()
    desc = _lib.PvsLayerDesc(d[0], d[1], d[2] | flags_extra, d[3])
    params, pstruct = layer._params_cached()
    n, e, hid = pg.n_nodes, pg.n_edges, case.hid
    f32 = dict(dtype=torch.float32, device='cuda')
    h, x = case.h0.cuda().contiguous(), case.x0.cuda().contiguous()
    h_out, x_out = torch.empty_like(h), torch.empty_like(x)
    natt = torch.empty(n, **f32)
    zeros = [torch.zeros((n, hid), **f32), torch.zeros((n, 3), **f32), torch.zeros(n, **f32)]
    saved = torch.empty(lib.pvs_egnn_layer_saved_floats(C.byref(desc), n, e), **f32)
    ws_bytes = lib.pvs_egnn_layer_workspace_bytes(C.byref(desc), n, e, 2)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    rc = lib.pvs_egnn_layer_fwd_partial(C.byref(desc), C.byref(pg.c), C.byref(pstruct), _lib.ptr(h), _lib.ptr(x),
                                        *[_lib.ptr(z) for z in zeros], _lib.ptr(h_out), _lib.ptr(x_out), _lib.ptr(natt),
                                        _lib.ptr(saved), _lib.ptr(ws), ws_bytes, _lib.stream(h.device))
    torch.cuda.synchronize()
    return rc, h_out, x_out


@pytest.mark.parametrize('natt', [False, True], ids=['gn', 'gn-natt'])
@pytest.mark.parametrize('hid', [32, 64, 128])
def test_layer_normalises_every_copy_as_if_it_ran_alone(hid, natt):
    case = _case(hid, natt)
    h, x = _layer_forward(case, _prepared('segments'))
    case.check(h, x, f'graphnorm-segments-layer-H{hid}-{"natt" if natt else "plain"}')


@pytest.mark.parametrize('natt', [False, True], ids=['gn', 'gn-natt'])
@pytest.mark.parametrize('hid', [32, 64, 128])
def test_stack_of_three_layers_normalises_every_copy_as_if_it_ran_alone(hid, natt):
    case = _case(hid, natt, DEPTH)
    pg = _prepared('segments')
    h, x = _stack_forward(case, pg)
    case.check(h, x, f'graphnorm-segments-stack-H{hid}-{"natt" if natt else "plain"}')
    # the per-layer calls launch the same kernels: the same bits
    h2, x2 = _layer_forward(case, pg)
    assert np.array_equal(_bits(h), _bits(h2)) and np.array_equal(_bits(x), _bits(x2))


@pytest.mark.parametrize('natt', [False, True], ids=['gn', 'gn-natt'])
@pytest.mark.parametrize('hid', [32, 64, 128])
def test_partial_layer_entry_normalises_every_copy_as_if_it_ran_alone(hid, natt):
    from pointvs_amd import _lib
    case = _case(hid, natt)
    rc, h, x = _partial_forward(case, _prepared('segments'), _lib.GRAPHNORM_SEGMENTS)
    assert rc == 0, _lib.lib().pvs_last_error()
    case.check(h, x, f'graphnorm-segments-partial-H{hid}-{"natt" if natt else "plain"}')


@pytest.mark.parametrize('hid', [32, 64, 128])
def test_whole_batch_statistics_miss_the_bound_on_these_inputs(hid):
    """The inputs show the coupling: the same batch normalised by the statistics of all real rows (set_norm_rows, the
    existing route) is outside the strict bound on at least one copy."""
    case = _case(hid, False)
    h, x = _layer_forward(case, _prepared('rows'))
    rows = case.margins(h, x)
    assert any(err > bound for _, key, err, bound in rows if key == 'h_out'), rows


def test_the_table_is_read_when_the_kernels_run():
    """One captured layer forward, replayed with three tables written into the same device tensor."""
    from pointvs_amd.nowait import capture_fixed_step
    case = _case(32, True)
    c = _copies()
    pg = _prepared('segments')
    table = pg.norm_segments
    (layer,) = case.layers()
    h0, x0 = case.h0.cuda(), case.x0.cuda()

    def step():
        with torch.no_grad():
            h, x, _ = layer.forward_prepared(pg, h0, x0, None, need_m=False)
        return h

    graph, static_h = capture_fixed_step(step, h0.device, lambda: None)
    whole = [0, c.n_real, c.n_real, c.n_real, c.n_real, c.n_real]          # one segment over every real row
    halves = [0, 100, 100, 300, c.n_real, c.n_cap]                         # other segments, the padding rows owned
    seen = []
    for ptr in (c.ptr, whole, halves):
        table.copy_(_table(ptr))
        graph.replay()
        torch.cuda.synchronize()
        got = static_h.clone()
        seen.append(got)
        fresh = _prepared(None)
        fresh.set_norm_segments(_table(ptr))
        assert np.array_equal(_bits(got), _bits(_layer_forward(case, fresh)[0])), ptr      # the eager call on that table
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    case.check(seen[0], _layer_forward(case, _prepared('segments'))[1], 'graphnorm-segments-captured-H32-natt')


# ---- refusals --------------------------------------------------------------------------------------------------------
def test_the_layers_refuse_what_the_segment_kernels_cannot_do():
    c = _copies()
    pg = _prepared('segments')
    x = torch.randn(c.n_cap, 3, device='cuda')
    layer = _new_layer(3, 32, LAYER_FLAGS[False], 11).cuda()
    h = torch.randn(c.n_cap, 32, device='cuda')
    with pytest.raises(NotImplementedError, match='autograd is recording'):          # parameters that require grad
        layer.forward_prepared(pg, h, x)
    with torch.no_grad():
        layer64 = _new_layer(3, 32, LAYER_FLAGS[False], 11).double().cuda()
        with pytest.raises(NotImplementedError, match='fp64'):
            layer64.forward_prepared(pg, h.double(), x.double())
        wide = _new_layer(3, 160, LAYER_FLAGS[False], 11).cuda()
        with pytest.raises(NotImplementedError, match='hidden sizes up to 128'):
            wide.forward_prepared(pg, torch.randn(c.n_cap, 160, device='cuda'), x)
        # a layer without GraphNorm does not look at the table
        plain = _new_layer(3, 32, dict(), 11).cuda()
        with_table = plain.forward_prepared(pg, h, x)[0]
        assert np.array_equal(_bits(with_table), _bits(plain.forward_prepared(_prepared(None), h, x)[0]))
        # cleared, every layer runs; set_norm_rows replaces the table and the other way round
        pg.set_norm_segments(None)
        assert pg.norm_segments is None and not pg.c.n_norm_rows_dev and pg.c.n_graphs == 0
        assert torch.isfinite(wide.forward_prepared(pg, torch.randn(c.n_cap, 160, device='cuda'), x)[0]).all()
        word, table = _table([c.n_real]), _table(c.ptr)
        pg.set_norm_segments(table)
        pg.set_norm_rows(word)
        assert pg.norm_segments is None and pg.t['norm_rows'] is word and pg.c.n_norm_rows_dev == word.data_ptr()
        pg.set_norm_segments(table)
        assert 'norm_rows' not in pg.t and pg.c.n_norm_rows_dev == table.data_ptr()
    for bad in (torch.zeros(1, dtype=torch.int32, device='cuda'), torch.zeros(3, dtype=torch.int64, device='cuda'),
                torch.zeros(3, dtype=torch.int32), torch.zeros(c.n_cap + 2, dtype=torch.int32, device='cuda')):
        with pytest.raises(ValueError, match='set_norm_segments'):
            pg.set_norm_segments(bad)


def test_the_c_entries_refuse_by_name():
    from pointvs_amd import _lib
    lib = _lib.lib()
    case = _case(32, False)
    c = _copies()
    SEG = _lib.GRAPHNORM_SEGMENTS

    def last():
        return lib.pvs_last_error().decode()

    # the flag without a table, with n_graphs < 1, and without PVS_GRAPHNORM: the forward entries
    rc, _, _ = _partial_forward(case, _prepared(None), SEG)
    assert rc != 0 and 'PVS_GRAPHNORM_SEGMENTS' in last() and 'NULL' in last()
    pg = _prepared('segments')
    pg.c.n_graphs = 0
    rc, _, _ = _partial_forward(case, pg, SEG)
    assert rc != 0 and 'PVS_GRAPHNORM_SEGMENTS' in last() and 'n_graphs' in last()
    pg = _prepared('segments')
    (layer,) = case.layers()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match='PVS_GRAPHNORM_SEGMENTS is valid only together with PVS_GRAPHNORM'):
            d = layer._desc()
            from pointvs_amd import functional as PF
            PF.egnn_layer(case.h0.cuda(), case.x0.cuda(), None, pg, (d[0], d[1], (d[2] & ~_lib.GRAPHNORM) | SEG, d[3]), False,
                          *layer._params_cached())
    # the backward entries and the fp64 entries: NULL tensors are never reached, the descriptor is refused first
    d = layer._desc()
    desc = _lib.PvsLayerDesc(d[0], d[1], d[2] | SEG, d[3])
    params, pstruct = layer._params_cached()
    grads = _lib.PvsLayerGrads()
    rc = lib.pvs_egnn_layer_bwd(C.byref(desc), C.byref(pg.c), C.byref(pstruct), None, None, None, None, None, None, None,
                                None, None, None, None, C.byref(grads), None, 0, _lib.stream(torch.device('cuda', 0)))
    assert rc != 0 and 'PVS_GRAPHNORM_SEGMENTS is forward-only' in last()
    descs = (_lib.PvsLayerDesc * 1)(desc)
    pstructs = (_lib.PvsLayerParams * 1)(pstruct)
    n, e = pg.n_nodes, pg.n_edges
    saved = lib.pvs_egnn_layer_saved_floats(C.byref(desc), n, e)
    from pointvs_amd.functional import _align
    strides = _lib.PvsStackStrides(_align(n * 32), _align(3 * n), _align(max(e, 1)), _align(n), _align(saved))
    rc = lib.pvs_egnn_stack_bwd(descs, pstructs, 1, C.byref(pg.c), C.byref(strides), *([None] * 10), C.byref(grads), None, 0,
                                _lib.stream(torch.device('cuda', 0)))
    assert rc != 0 and 'PVS_GRAPHNORM_SEGMENTS' in last() and 'forward-only' in last()
    p64 = _lib.PvsLayerParamsF64()
    rc = lib.pvs_egnn_layer_fwd_f64(C.byref(desc), C.byref(pg.c), C.byref(p64), *([None] * 9), None, 0,
                                    _lib.stream(torch.device('cuda', 0)))
    assert rc != 0 and 'PVS_GRAPHNORM_SEGMENTS' in last() and 'fp32 only' in last()
