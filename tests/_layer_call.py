"""A direct caller of pvs_egnn_layer_fwd / _bwd (and the fp64 pair) for tests: helper, not a test.

Modelled line for line on pointvs_amd/functional.py `_EGNNLayerFn.forward / .backward`, with two differences that no
caller of the Python package can make: any gradient slot can be passed as NULL (`skip`, on top of `dead_grads`), and every
tensor the caller owns lies in an arena, at a chosen 0 or 4 bytes from a 256-byte boundary, between guards.

Arena: one tensor of the call's dtype, pre-filled with one NaN bit pattern; each tensor carved out of it has GUARD
elements before and after it that belong to nobody. After a call every element outside the carved tensors must still
hold the pattern (`guards_intact`), and no element of an output that the contract says is written may
(`untouched_outputs`). The workspace stays as the allocator gives it.

Works on a `Problem` of tests/test_gpu_edge_classes.py (one layer): edge tensors go in and come out in the caller's edge
order through rows_to_sorted_order / rows_to_input_order, as EGNNLayer.forward does, so `Problem.ref64` applies
unchanged; the result is the numpy dict that `Problem.check` takes, with only the requested gradients.
"""
import contextlib
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import torch

GUARD = 64                                   # elements before and after every carved tensor
ALIGN_BYTES = 256
FILL32, FILL64 = 0x7FC5A5A5, 0x7FF8A5A5A5A5A5A5      # quiet NaNs no kernel computes
FORWARD_TENSORS = ('h', 'x', 'm_prev', 'h_out', 'x_out', 'm_out', 'att', 'node_att', 'saved')
BACKWARD_TENSORS = ('g_h_out', 'g_x_out', 'g_m_out', 'g_h', 'g_x', 'g_m_prev')


class Arena:
    """`spec`: [(name, shape)]; `offsets`: name -> elements of 4 bytes added to the tensor's 256-byte-aligned start."""

    def __init__(self, spec, offsets, dtype, device='cuda'):
        item = torch.empty((), dtype=dtype).element_size()
        bits = {4: torch.int32, 8: torch.int64}[item]
        self.fill = {4: FILL32, 8: FILL64}[item]
        per_align = ALIGN_BYTES // item
        assert not offsets or item == 4, 'a 4-byte offset misaligns the values of an fp64 tensor themselves'
        starts, pos = {}, 0
        for name, shape in spec:
            pos = -(-(pos + GUARD) // per_align) * per_align
            starts[name] = pos + int(offsets.get(name, 0))
            pos = starts[name] + int(np.prod(shape))
        total = pos + GUARD
        raw = torch.empty(total + per_align, dtype=dtype, device=device)
        lead = (-raw.data_ptr() % ALIGN_BYTES) // item
        self.flat = raw[lead:lead + total]
        assert self.flat.data_ptr() % ALIGN_BYTES == 0
        self.bits = self.flat.view(bits)
        self.bits.fill_(self.fill)
        self.owned = torch.zeros(total, dtype=torch.bool, device=device)
        self.t = {}
        for name, shape in spec:
            n = int(np.prod(shape))
            self.t[name] = self.flat[starts[name]:starts[name] + n].view(shape)
            self.owned[starts[name]:starts[name] + n] = True
            assert self.t[name].data_ptr() % ALIGN_BYTES == 4 * int(offsets.get(name, 0)) and self.t[name].is_contiguous()

    def guards_intact(self):
        return bool((self.bits[~self.owned] == self.fill).all())

    def untouched(self, name):
        t = self.t[name]
        return int((t.reshape(-1).view(self.bits.dtype) == self.fill).sum())


@contextlib.contextmanager
def environment(env):
    """The layer-level switches are read by the library at every call (csrc/layer_plan.h)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def state_dict_name(slot):
    """'node_w2' -> 'node_mlp.3.weight': the key of Problem.ref64 ('grad ' + this)."""
    from pointvs_amd import _lib
    from pointvs_amd.egnn_satorras import EGNNLayer
    cont, idx, name = EGNNLayer._SLOTS[_lib.PARAM_FIELDS.index(slot)]
    return name if cont is None else f'{cont}.{idx}.{name}'


def forward(problem, offsets=None, env=None, dtype=torch.float32):
    """pvs_egnn_layer_fwd on the problem's graph and layer. -> namespace for `backward` (tensors in `.arena.t`)."""
    from pointvs_amd import _lib
    from pointvs_amd import functional as PF
    from pointvs_amd.graph import prepare_graph
    from tests.test_gpu_edge_classes import _new_layer
    assert problem.depth == 1
    offsets, env = dict(offsets or {}), dict(env or {})
    kind = PF.KINDS[dtype]
    layer = _new_layer(problem.A, problem.hid, problem.flags, 11)
    layer.load_state_dict(problem.sds[0])
    layer = layer.to(dtype).cuda()
    params = tuple(None if p is None else p.detach() for p in layer._params())
    pstruct = kind.params_t(*[_lib.ptr(p) for p in params])
    g = problem.g
    ea = None if g.edge_attr is None else g.edge_attr.cuda()
    pg = prepare_graph(g.edge_index.cuda(), ea, g.n_nodes, need_backward=True)
    pg.check_status()
    hidden, n_attr, flags, act = desc_tuple = layer._desc()
    n, e = pg.n_nodes, pg.n_edges
    assert e > 0 and n_attr == pg.n_edge_attr
    desc = _lib.PvsLayerDesc(hidden, n_attr, flags, act)
    eatt = bool(flags & _lib.EDGE_ATTENTION)
    natt = bool(flags & _lib.NODE_ATTENTION)
    eres = bool(flags & _lib.EDGE_RESIDUAL)
    n_saved = kind.layer_saved(C.byref(desc), n, e)
    spec = [('h', (n, hidden)), ('x', (n, 3))] + ([('m_prev', (e, hidden))] if eres else [])
    spec += [('h_out', (n, hidden)), ('x_out', (n, 3)), ('m_out', (e, hidden))]
    spec += ([('att', (e,))] if eatt else []) + ([('node_att', (n,))] if natt else []) + [('saved', (n_saved,))]
    arena = Arena(spec, {k: v for k, v in offsets.items() if k in FORWARD_TENSORS}, dtype)
    t = arena.t
    t['h'].copy_(problem.h0.to(dtype))
    t['x'].copy_(g.pos.to(dtype))
    if eres:
        t['m_prev'].copy_(PF.rows_to_sorted_order(problem.m0.to(dtype).cuda(), pg))
    dev = t['h'].device
    ws_bytes = kind.layer_ws(C.byref(desc), n, e, 0)
    ws = PF._ws(ws_bytes, dev)
    with environment(env):
        rc = kind.layer_fwd(
            C.byref(desc), C.byref(pg.c), C.byref(pstruct), _lib.ptr(t['h']), _lib.ptr(t['x']), _lib.ptr(t.get('m_prev')),
            _lib.ptr(t['h_out']), _lib.ptr(t['x_out']), _lib.ptr(t['m_out']), _lib.ptr(t.get('att')),
            _lib.ptr(t.get('node_att')), _lib.ptr(t['saved']), _lib.ptr(ws), ws_bytes, PF._stream(dev))
        kind.check(rc, 'layer_fwd')
        torch.cuda.synchronize()
    return SimpleNamespace(arena=arena, layer=layer, params=params, pstruct=pstruct, pg=pg, desc_tuple=desc_tuple,
                           kind=kind, dtype=dtype, eres=eres, eatt=eatt, natt=natt, offsets=offsets)


def backward(problem, fwd, skip=(), offsets=None, env=None):
    """pvs_egnn_layer_bwd for the loss of Problem (sum h_out wh + sum x_out wx + sum m wm), the slots of `skip` (names of
    _lib.PARAM_FIELDS, or 'ALL') passed as NULL on top of `dead_grads`.
    -> (values, guards_intact, untouched_outputs): the numpy dict of Problem.check with the requested gradients only;
    whether every guard element of both arenas still holds the fill pattern; {output: elements still holding it}."""
    from pointvs_amd import _lib
    from pointvs_amd import functional as PF
    offsets, env = dict(fwd.offsets if offsets is None else offsets), dict(env or {})
    assert {k: v for k, v in offsets.items() if k in FORWARD_TENSORS} == \
        {k: v for k, v in fwd.offsets.items() if k in FORWARD_TENSORS}, 'forward and backward see the same tensors'
    kind, dtype, pg, ft = fwd.kind, fwd.dtype, fwd.pg, fwd.arena.t
    hidden, n_attr, flags, act = fwd.desc_tuple
    n, e = pg.n_nodes, pg.n_edges
    desc = _lib.PvsLayerDesc(hidden, n_attr, flags, act)
    dead = PF.dead_grads(flags, True, fwd.eres)
    wanted = [name for name, p in zip(_lib.PARAM_FIELDS, fwd.params)
              if p is not None and name not in dead and skip != 'ALL' and name not in skip]
    spec = [('g_h_out', (n, hidden)), ('g_x_out', (n, 3)), ('g_m_out', (e, hidden)), ('g_h', (n, hidden)), ('g_x', (n, 3))]
    spec += [('g_m_prev', (e, hidden))] if fwd.eres else []
    shapes = dict(zip(_lib.PARAM_FIELDS, (None if p is None else tuple(p.shape) for p in fwd.params)))
    spec += [('grad ' + name, shapes[name]) for name in wanted]
    arena = Arena(spec, {k: v for k, v in offsets.items() if k in BACKWARD_TENSORS}, dtype)
    t = arena.t
    t['g_h_out'].copy_(problem.wh.to(dtype))
    t['g_x_out'].copy_(problem.wx.to(dtype))
    t['g_m_out'].copy_(PF.rows_to_sorted_order(problem.wm.to(dtype).cuda(), pg))
    gstruct = kind.grads_t(*[_lib.ptr(t.get('grad ' + name)) for name in _lib.PARAM_FIELDS])
    dev = t['g_h'].device
    ws_bytes = kind.layer_ws(C.byref(desc), n, e, 1)
    ws = PF._ws(ws_bytes, dev)
    with environment(env):
        rc = kind.layer_bwd(
            C.byref(desc), C.byref(pg.c), C.byref(fwd.pstruct), _lib.ptr(ft['h']), _lib.ptr(ft['x']),
            _lib.ptr(ft.get('m_prev')), _lib.ptr(ft.get('att')), _lib.ptr(ft['saved']), _lib.ptr(t['g_h_out']),
            _lib.ptr(t['g_x_out']), _lib.ptr(t['g_m_out']), _lib.ptr(t['g_h']), _lib.ptr(t['g_x']),
            _lib.ptr(t.get('g_m_prev')), C.byref(gstruct), _lib.ptr(ws), ws_bytes, PF._stream(dev))
        kind.check(rc, 'layer_bwd')
        torch.cuda.synchronize()

    def input_order(rows):
        return PF.rows_to_input_order(rows.clone(), pg)
    res = dict(h_out=ft['h_out'], x_out=ft['x_out'], m=input_order(ft['m_out']), g_h=t['g_h'], g_x=t['g_x'])
    if fwd.eatt:
        res['att'] = input_order(ft['att'].reshape(-1, 1))
    if fwd.natt:
        res['natt'] = ft['node_att'].reshape(-1, 1)
    if fwd.eres:
        res['g_m_prev'] = input_order(t['g_m_prev'])
    for name in wanted:
        res['grad ' + state_dict_name(name)] = t['grad ' + name]
    values = {k: v.detach().cpu().numpy().copy() for k, v in res.items()}
    written_fwd = [k for k in ('h_out', 'x_out', 'm_out', 'att', 'node_att') if k in ft]
    written_bwd = [k for k in t if k not in ('g_h_out', 'g_x_out', 'g_m_out')]
    untouched = {k: fwd.arena.untouched(k) for k in written_fwd}
    untouched.update({k: arena.untouched(k) for k in written_bwd})
    guards = fwd.arena.guards_intact() and arena.guards_intact()
    return values, guards, {k: v for k, v in untouched.items() if v}


# ---- the route a call took ---------------------------------------------------------------------------------------------
@contextlib.contextmanager
def recorded_routes(names):
    """Launch counts per group of the library's measurement hook, read as tests/test_gpu_node_side.py test_node_routes
    does: `with recorded_routes(names) as seen:` fills `seen` (name -> count, non-zero only) when the block ends."""
    from pointvs_amd import _lib
    from tests.test_gpu_dense_ops import NODE_ROUTE_NAMES, ROUTE_FIRST_ID, ROUTE_NAMES
    lib = _lib.lib()
    known = ROUTE_NAMES + NODE_ROUTE_NAMES
    assert set(names) <= set(known)
    mask = sum(1 << (ROUTE_FIRST_ID + known.index(name) + 1) for name in names)
    seen = {}
    lib.pvs_profile_reset()
    lib.pvs_profile_enable(mask)
    try:
        yield seen
        torch.cuda.synchronize()
    finally:
        lib.pvs_profile_enable(0)
        for name in names:
            ms, cnt = C.c_double(0.0), C.c_int64(0)
            assert lib.pvs_profile_read(name.encode(), C.byref(ms), C.byref(cnt)) == 0, name
            if cnt.value:
                seen[name] = cnt.value
        lib.pvs_profile_reset()
