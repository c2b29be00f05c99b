"""torch.autograd.Function wrappers over the C ABI (include/pvs_egnn.h).

PyTorch supplies device memory, the current stream and the autograd tape; every arithmetic step
of the path runs in libpvs_egnn.so.
"""
import ctypes as C
import math

import torch

from . import _lib
from .nowait import LateQueue


def _stream(dev):
    return _lib.stream(dev)


def _ws(nbytes, dev):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=dev)


_F32, _F64 = torch.float32, torch.float64


class _Kind:
    """What distinguishes the fp32 and the fp64 family of this binding, said once: the torch dtype, the parameter and
    gradient struct classes of the layer, the 32-bit words per value (the row permutation is a bit copy) and, per
    operator, the C entry point. Every wrapper below has ONE body and reads these from the kind of its call.
    The entry points become attributes (bound ctypes functions) the first time one of them is asked for: the library is
    loaded by then and not at import, and a call pays a plain attribute look-up."""

    def __init__(self, dtype, params_t, grads_t, words, **entry):
        self.dtype, self.params_t, self.grads_t, self.words, self.entry = dtype, params_t, grads_t, words, entry

    def __getattr__(self, op):      # (reached only while the entry points are unbound: binds them all)
        entry = self.__dict__.get('entry')      # (absent on an instance made without __init__: copy / pickle probes)
        if entry is None or op not in entry:
            raise AttributeError(op)
        lib = _lib.lib()
        # (the one write after __init__: from here on the record is only read)
        self.__dict__.update({name: getattr(lib, symbol) for name, symbol in self.entry.items()})
        return self.__dict__[op]

    def check(self, rc, op):
        if rc != 0:
            _lib.check(rc, self.entry[op])


KINDS = {
    _F32: _Kind(_F32, _lib.PvsLayerParams, _lib.PvsLayerGrads, 1,
                rows_to_input='pvs_rows_to_input_order', rows_to_sorted='pvs_rows_to_sorted_order',
                layer_saved='pvs_egnn_layer_saved_floats', layer_ws='pvs_egnn_layer_workspace_bytes',
                layer_fwd='pvs_egnn_layer_fwd', layer_bwd='pvs_egnn_layer_bwd',
                linear_fwd='pvs_linear_fwd', linear_bwd_ws='pvs_linear_bwd_workspace_bytes', linear_bwd='pvs_linear_bwd',
                mean_pool_fwd='pvs_mean_pool_fwd', mean_pool_bwd='pvs_mean_pool_bwd',
                segment_ws='pvs_segment_workspace_bytes', segment_fwd='pvs_segment_reduce_fwd',
                segment_bwd='pvs_segment_reduce_bwd'),
    # (the row permutation has no fp64 entry: the fp32 one moves 2 x width words per row)
    _F64: _Kind(_F64, _lib.PvsLayerParamsF64, _lib.PvsLayerGradsF64, 2,
                rows_to_input='pvs_rows_to_input_order', rows_to_sorted='pvs_rows_to_sorted_order',
                layer_saved='pvs_egnn_layer_saved_doubles_f64', layer_ws='pvs_egnn_layer_workspace_bytes_f64',
                layer_fwd='pvs_egnn_layer_fwd_f64', layer_bwd='pvs_egnn_layer_bwd_f64',
                linear_fwd='pvs_linear_fwd_f64', linear_bwd_ws='pvs_linear_bwd_workspace_bytes_f64',
                linear_bwd='pvs_linear_bwd_f64',
                mean_pool_fwd='pvs_mean_pool_fwd_f64', mean_pool_bwd='pvs_mean_pool_bwd_f64',
                segment_ws='pvs_segment_workspace_bytes_f64', segment_fwd='pvs_segment_reduce_fwd_f64',
                segment_bwd='pvs_segment_reduce_bwd_f64'),
}
_K32, _K64 = KINDS[_F32], KINDS[_F64]
STACK_KIND = _K32        # the one-call layer stack (pvs_egnn_stack_fwd / _bwd) is built for fp32 only


def _kind_of(what, t):
    kind = KINDS.get(t.dtype)
    if kind is None:
        raise TypeError(f'{what}: pointvs_amd kernels are float32 or float64 (got {t.dtype})')
    return kind


def _c(t, dtype, note=''):
    """`t` contiguous, checked to be of `dtype` (the dtype of the call): the kernels never cast."""
    if t is None:
        return None
    if t.dtype != dtype:
        raise TypeError(f'pointvs_amd: a {t.dtype} tensor in a {dtype} call (mixed dtypes are not cast){note}')
    return t.contiguous()


_FP32_ONLY = ': this op is fp32 only, fp64 runs per-layer ops'


def _call_dtype(what, primary, **others):
    """The dtype of a call: its primary input's, fp32 or fp64. Any other floating tensor of another dtype is a
    TypeError that names them all (fp64 parameters with fp32 features, say): never cast silently."""
    dtype = _kind_of(what, primary).dtype
    bad = [f'{k}: {t.dtype}' for k, t in others.items() if t is not None and t.dtype != dtype]
    if bad:
        raise TypeError(f'{what}: mixed dtypes - the primary input is {dtype}, but ' + ', '.join(bad) +
                        ' (convert the model and its inputs to one dtype: model.double() / .float())')
    return dtype


class _PermuteRows(torch.autograd.Function):
    """Rows between input edge order and CSR-sorted order (and back in the backward)."""

    @staticmethod
    def forward(ctx, src, perm, to_input):
        kind = _kind_of('rows_to_input_order / rows_to_sorted_order', src)
        src = src.contiguous()
        _lib.require_hip(src)
        ctx.perm, ctx.to_input, ctx.dtype = perm, to_input, kind.dtype
        width = (src.shape[1] if src.dim() > 1 else 1) * kind.words
        dst = torch.empty_like(src)
        fn = kind.rows_to_input if to_input else kind.rows_to_sorted
        kind.check(fn(_lib.ptr(src), _lib.ptr(dst), _lib.ptr(perm), src.shape[0], width, _stream(src.device)),
                   'rows_to_input' if to_input else 'rows_to_sorted')
        return dst

    @staticmethod
    def backward(ctx, g):
        return _PermuteRows.apply(_c(g, ctx.dtype), ctx.perm, not ctx.to_input), None, None


def rows_to_input_order(src_sorted, pg):
    return _PermuteRows.apply(src_sorted, pg.perm, True)


def rows_to_sorted_order(src_input, pg):
    return _PermuteRows.apply(src_input, pg.perm, False)


_COORD_MLP = ('coord_w1', 'coord_b1', 'coord_w2')


def dead_grads(flags, coords_fed, edge_res):
    """The slots of `_lib.PARAM_FIELDS` that get NO gradient in a layer's backward (every other parameter the layer has
    gets one): the coord MLP unless the layer updates coordinates and a gradient arrived for them (`coords_fed`), the
    edge gate unless messages came from the layer before (`edge_res`) through a rezero / gated residual."""
    dead = () if flags & _lib.UPDATE_COORDS and coords_fed else _COORD_MLP
    if not (edge_res and flags & (_lib.REZERO | _lib.GATED_RESIDUAL)):
        dead += ('edge_gate',)
    return dead


class _EGNNLayerFn(torch.autograd.Function):
    """One EGNNLayer.forward (egnn_satorras.py:189-206) and its backward, sorted edge order, in the dtype of `kind`."""

    @staticmethod
    def forward(ctx, kind, h, x, m_prev, pg, desc_tuple, need_m, pstruct, *params):
        # pstruct: the layer's parameter struct built ONCE for these very parameter tensors (EGNNLayer._params_cached:
        # of the kind's dtype, contiguous, on the device - checked when it was built), or None (padded / ad-hoc
        # parameter tensors). Host time matters here: at the reference's default shape (32 graphs of 500 atoms) a
        # training step is ~70 launches of a few microseconds and the step is bound by this Python
        # (tools/host_profile.py).
        hidden, n_attr, flags, act = desc_tuple
        dtype = kind.dtype
        h, x, m_prev = _c(h, dtype), _c(x, dtype), _c(m_prev, dtype)
        if pstruct is None:
            params = tuple(_c(p, dtype) for p in params)
            _lib.require_hip(h, x, m_prev, *params)
            pstruct = kind.params_t(*[_lib.ptr(p) for p in params])
        else:
            _lib.require_hip(h, x, m_prev)
        dev = h.device
        n, e = pg.n_nodes, pg.n_edges
        if h.shape != (n, hidden) or x.shape != (n, 3):
            raise ValueError(f'h {tuple(h.shape)} / coord {tuple(x.shape)} do not match N={n}, '
                             f'H={hidden}')
        if n_attr != pg.n_edge_attr:
            raise ValueError(f'layer built with edges_in_d={n_attr} but edge_attr has '
                             f'{pg.n_edge_attr} columns')
        desc = _lib.PvsLayerDesc(hidden, n_attr, flags, act)
        eatt = bool(flags & _lib.EDGE_ATTENTION)
        natt = bool(flags & _lib.NODE_ATTENTION)
        eres = bool(flags & _lib.EDGE_RESIDUAL) and m_prev is not None
        h_out = torch.empty_like(h)
        x_out = torch.empty_like(x)
        m_out = torch.empty((max(e, 0), hidden), dtype=dtype, device=dev) if need_m else None
        att = torch.empty((max(e, 1),), dtype=dtype, device=dev) if eatt else None
        node_att = torch.empty((n,), dtype=dtype, device=dev) if natt else None
        saved = torch.empty(kind.layer_saved(C.byref(desc), n, e), dtype=dtype, device=dev)
        ws_bytes = kind.layer_ws(C.byref(desc), n, e, 0)
        ws = _ws(ws_bytes, dev)
        rc = kind.layer_fwd(
            C.byref(desc), C.byref(pg.c), C.byref(pstruct), _lib.ptr(h), _lib.ptr(x),
            _lib.ptr(m_prev if eres else None), _lib.ptr(h_out), _lib.ptr(x_out), _lib.ptr(m_out),
            _lib.ptr(att), _lib.ptr(node_att), _lib.ptr(saved), _lib.ptr(ws), ws_bytes, _stream(dev))
        kind.check(rc, 'layer_fwd')
        ctx.pg, ctx.desc_tuple, ctx.eres, ctx.kind = pg, desc_tuple, eres, kind
        ctx.pstruct = pstruct      # (the backward reads the same parameter tensors: saved below, so they cannot have moved)
        ctx.save_for_backward(h, x, m_prev if eres else None, att, saved, *params)
        ctx.set_materialize_grads(False)
        # absent outputs are None, not empty tensors (h.new_empty(0) cost 22 us apiece on the host: 0.4 ms per step of a
        # 6-layer model)
        if att is not None or node_att is not None:       # (one call: a second call replaces the first one's list)
            ctx.mark_non_differentiable(*[t for t in (att, node_att) if t is not None])
        return h_out, x_out, m_out, att, node_att

    @staticmethod
    def backward(ctx, g_h_out, g_x_out, g_m_out, _g_att, _g_natt):
        h, x, m_prev, att, saved, *params = ctx.saved_tensors
        pg, kind = ctx.pg, ctx.kind
        hidden, n_attr, flags, act = ctx.desc_tuple
        dev, dtype = h.device, kind.dtype
        n, e = pg.n_nodes, pg.n_edges
        desc = _lib.PvsLayerDesc(hidden, n_attr, flags, act)
        pstruct = ctx.pstruct
        g_h_out = torch.zeros_like(h) if g_h_out is None else _c(g_h_out, dtype)
        g_x_out = _c(g_x_out, dtype)       # None => the caller never used x_out (last layer)
        g_m_out = _c(g_m_out, dtype) if (g_m_out is not None and g_m_out.numel()) else None
        need = ctx.needs_input_grad
        g_h = torch.empty_like(h)
        g_x = torch.empty_like(x) if need[2] else None
        g_m_prev = torch.empty_like(m_prev) if ctx.eres else None
        dead = dead_grads(flags, g_x_out is not None, ctx.eres)
        grads = [None if (p is None or name in dead) else torch.empty_like(p)
                 for name, p in zip(_lib.PARAM_FIELDS, params)]
        gstruct = kind.grads_t(*[_lib.ptr(g) for g in grads])
        ws_bytes = kind.layer_ws(C.byref(desc), n, e, 1)
        ws = _ws(ws_bytes, dev)
        rc = kind.layer_bwd(
            C.byref(desc), C.byref(pg.c), C.byref(pstruct), _lib.ptr(h), _lib.ptr(x),
            _lib.ptr(m_prev), _lib.ptr(att), _lib.ptr(saved), _lib.ptr(g_h_out), _lib.ptr(g_x_out),
            _lib.ptr(g_m_out), _lib.ptr(g_h), _lib.ptr(g_x), _lib.ptr(g_m_prev), C.byref(gstruct),
            _lib.ptr(ws), ws_bytes, _stream(dev))
        kind.check(rc, 'layer_bwd')
        return (None, g_h, g_x, g_m_prev, None, None, None, None, *grads)


def egnn_layer(h, x, m_prev_sorted, pg, desc_tuple, need_m, params, pstruct=None):
    """Returns (h_out, x_out, m_sorted|None, att_sorted|None, node_att|None). pstruct: see _EGNNLayerFn.forward.
    fp64 (h float64, or a layer whose cached parameter struct is fp64) runs the fp64 kernels; mixed dtypes raise."""
    kind = _K32
    if h.dtype == _F64 or isinstance(pstruct, _K64.params_t):
        kind = _K64
        _call_dtype('EGNNLayer', h, coord=x, edge_messages=m_prev_sorted,
                    **{name: p for name, p in zip(_lib.PARAM_FIELDS, params)})
        if pg.c.n_edges_dev:
            raise NotImplementedError('fp64 layers need a graph with a host-known edge count')
    elif pstruct is None and params and params[0] is not None and params[0].dtype == _F64:
        _call_dtype('EGNNLayer', h, coord=x, **{name: p for name, p in zip(_lib.PARAM_FIELDS, params)})
    return _EGNNLayerFn.apply(kind, h, x, m_prev_sorted, pg, desc_tuple, need_m, pstruct, *params)


def _align(count, to=64):
    return (int(count) + to - 1) // to * to


class StackPlan:
    """What the one-call layer stack (`pvs_egnn_stack_fwd/bwd`) needs about a model's EGNN layers, built once and kept
    while the layers' parameter structs stay the same objects: the C arrays of descriptors and parameter structs, the flat
    tuple of parameter tensors handed to autograd and, for each of them, (layer, slot of `_lib.PARAM_FIELDS`).
    `pstructs` are the layers' own cached PvsLayerParams (EGNNLayer._params_cached): held here, so `is` against a layer's
    current struct says whether any parameter has moved since."""

    def __init__(self, desc_tuples, param_tuples, pstructs):
        n = len(desc_tuples)
        self.n_layers, self.hidden = n, desc_tuples[0][0]
        self.desc_tuples, self.pstructs = tuple(desc_tuples), tuple(pstructs)
        self.descs = (_lib.PvsLayerDesc * n)(*[_lib.PvsLayerDesc(*d) for d in desc_tuples])
        self.params_c = (STACK_KIND.params_t * n)(*pstructs)       # (copies of the structs: plain pointers)
        self.any_eatt = any(d[2] & _lib.EDGE_ATTENTION for d in desc_tuples)
        self.any_natt = any(d[2] & _lib.NODE_ATTENTION for d in desc_tuples)
        self.index, flat = [], []
        for layer, params in enumerate(param_tuples):
            for slot, p in enumerate(params):
                if p is not None:
                    self.index.append((layer, slot))
                    flat.append(p)
        self.params = tuple(flat)
        self._sizes, self._layouts = {}, {}

    def grad_layout(self, last_coords_live):
        """Where every parameter gradient of a backward sits in ONE flat buffer. Which gradients exist is `dead_grads`, as
        in _EGNNLayerFn.backward: a layer's coordinates fed something in every layer but the last, and in the last one
        when a gradient arrives for x_L; a stack has no edge residual."""
        got = self._layouts.get(last_coords_live)
        if got is None:
            got = self._layouts[last_coords_live] = _GradLayout(self, last_coords_live)
        return got

    def sizes(self, n, e):
        """(strides struct, forward workspace bytes, backward workspace bytes) for a graph of n nodes and e edges."""
        got = self._sizes.get((n, e))
        if got is None:
            lib = _lib.lib()
            saved = STACK_KIND.layer_saved(self.descs, n, e)
            st = _lib.PvsStackStrides(_align(n * self.hidden), _align(3 * n), _align(max(e, 1)), _align(n), _align(saved))
            got = (st, lib.pvs_egnn_stack_workspace_bytes(self.descs, self.n_layers, n, e, 0),
                   lib.pvs_egnn_stack_workspace_bytes(self.descs, self.n_layers, n, e, 1))
            if len(self._sizes) > 64:
                self._sizes.clear()
            self._sizes[(n, e)] = got
        return got


class _GradLayout:
    """`sizes`: the split of the flat buffer (gradients and the pads that keep each one 16-byte aligned); `take`: per
    parameter of `plan.params` (index into the split or -1 = no gradient, shape to view it as or None for 1-D);
    `structs(base)`: the PvsLayerGrads array for a flat buffer at address `base` (kept per address: the caching allocator
    alternates between a few)."""

    def __init__(self, plan, last_coords_live):
        fields, nl = _lib.PARAM_FIELDS, plan.n_layers
        self.sizes, self.take, self._offsets, self._by_base = [], [], [], {}
        off = 0
        dead = [dead_grads(d[2], layer < nl - 1 or last_coords_live, False) for layer, d in enumerate(plan.desc_tuples)]
        for (layer, slot), p in zip(plan.index, plan.params):
            if fields[slot] in dead[layer]:
                self.take.append((-1, None))
                continue
            k = p.numel()
            self.take.append((len(self.sizes), None if p.dim() == 1 else tuple(p.shape)))
            self.sizes.append(k)
            self._offsets.append((layer, slot, 4 * off))
            off += k
            if k % 4:
                self.sizes.append(4 - k % 4)
                off += 4 - k % 4
        self.total, self.n_layers, self.n_fields = off, nl, len(fields)

    def structs(self, base):
        got = self._by_base.get(base)
        if got is None:
            rows = [[None] * self.n_fields for _ in range(self.n_layers)]
            for layer, slot, byte_off in self._offsets:
                rows[layer][slot] = base + byte_off
            got = (STACK_KIND.grads_t * self.n_layers)(*[STACK_KIND.grads_t(*r) for r in rows])
            if len(self._by_base) > 32:
                self._by_base.clear()
            self._by_base[base] = got
        return got


class _EGNNStackFn(torch.autograd.Function):
    """All EGNN layers of a model (the loop of SartorrasEGNN.get_embeddings, egnn_satorras.py:325-328) as ONE autograd
    node over `pvs_egnn_stack_fwd/bwd`: the same launches as one `_EGNNLayerFn` per layer, bit for bit the same values
    (tests/test_gpu_stack.py), a sixth of the host time for six layers. No edge residual (per-layer path)."""

    @staticmethod
    def forward(ctx, h0, x0, pg, plan, *params):
        lib = _lib.lib()
        h0, x0 = _c(h0, _F32, _FP32_ONLY), _c(x0, _F32, _FP32_ONLY)
        _lib.require_hip(h0, x0)
        n, e, hidden, nl = pg.n_nodes, pg.n_edges, plan.hidden, plan.n_layers
        if h0.shape != (n, hidden) or x0.shape != (n, 3):
            raise ValueError(f'h {tuple(h0.shape)} / coord {tuple(x0.shape)} do not match N={n}, H={hidden}')
        if plan.desc_tuples[0][1] != pg.n_edge_attr:
            raise ValueError(f'layers built with edges_in_d={plan.desc_tuples[0][1]} but edge_attr has '
                             f'{pg.n_edge_attr} columns')
        dev = h0.device
        st, ws_bytes, _ = plan.sizes(n, e)
        f32 = torch.float32
        h_out, x_out = torch.empty_like(h0), torch.empty_like(x0)
        h_mid = torch.empty((nl - 1, st.h_mid), dtype=f32, device=dev) if nl > 1 else None
        x_mid = torch.empty((nl - 1, st.x_mid), dtype=f32, device=dev) if nl > 1 else None
        att = torch.empty((nl, st.att), dtype=f32, device=dev) if plan.any_eatt else None
        natt = torch.empty((nl, st.node_att), dtype=f32, device=dev) if plan.any_natt else None
        saved = torch.empty((nl, st.saved), dtype=f32, device=dev)
        ws = _ws(ws_bytes, dev)
        rc = lib.pvs_egnn_stack_fwd(plan.descs, plan.params_c, nl, C.byref(pg.c), C.byref(st), _lib.ptr(h0), _lib.ptr(x0),
                                    _lib.ptr(h_mid), _lib.ptr(x_mid), _lib.ptr(h_out), _lib.ptr(x_out), _lib.ptr(att),
                                    _lib.ptr(natt), _lib.ptr(saved), _lib.ptr(ws), ws_bytes, _stream(dev))
        _lib.check(rc, 'pvs_egnn_stack_fwd')
        ctx.pg, ctx.plan = pg, plan
        ctx.save_for_backward(h0, x0, h_mid, x_mid, att, saved, *params)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable(*[t for t in (h_mid, x_mid, att, natt) if t is not None])
        return h_out, x_out, h_mid, x_mid, att, natt

    @staticmethod
    def backward(ctx, g_h_out, g_x_out, *_unused):
        lib = _lib.lib()
        h0, x0, h_mid, x_mid, att, saved, *params = ctx.saved_tensors
        pg, plan = ctx.pg, ctx.plan
        n, e, nl = pg.n_nodes, pg.n_edges, plan.n_layers
        dev = h0.device
        g_h_out = torch.zeros_like(h0) if g_h_out is None else _c(g_h_out, _F32, _FP32_ONLY)
        g_x_out = _c(g_x_out, _F32, _FP32_ONLY)        # None => nothing read the last layer's coordinates
        g_h0 = torch.empty_like(h0)
        g_x0 = torch.empty_like(x0) if ctx.needs_input_grad[1] else None
        # ONE allocation for all parameter gradients, handed out as views (16-byte aligned): 78 allocations less per step
        # of a 6-layer model, and the optimiser finds its pointer table again by one address instead of 78 that the
        # caching allocator shuffles from step to step (FusedClipAdam._recent)
        lay = plan.grad_layout(g_x_out is not None)
        flat = torch.empty((lay.total,), dtype=torch.float32, device=dev)
        parts = flat.split_with_sizes(lay.sizes)
        grads = [None if k < 0 else (parts[k] if shape is None else parts[k].view(shape)) for k, shape in lay.take]
        gstructs = lay.structs(flat.data_ptr())
        st, _, ws_bytes = plan.sizes(n, e)
        ws = _ws(ws_bytes, dev)
        rc = lib.pvs_egnn_stack_bwd(plan.descs, plan.params_c, nl, C.byref(pg.c), C.byref(st), _lib.ptr(h0), _lib.ptr(x0),
                                    _lib.ptr(h_mid), _lib.ptr(x_mid), _lib.ptr(att), _lib.ptr(saved), _lib.ptr(g_h_out),
                                    _lib.ptr(g_x_out), _lib.ptr(g_h0), _lib.ptr(g_x0), gstructs, _lib.ptr(ws), ws_bytes,
                                    _stream(dev))
        _lib.check(rc, 'pvs_egnn_stack_bwd')
        return (g_h0, g_x0, None, None, *grads)


def egnn_stack(h0, x0, pg, plan):
    """Returns (h_L, x_L, h_mid, x_mid, att, node_att): the last layer's outputs and the per-layer buffers (rows of
    `plan.sizes(n, e)[0]` strides; None where no layer needs them) the side attributes are read from."""
    return _EGNNStackFn.apply(h0, x0, pg, plan, *plan.params)


class _LinearFn(torch.autograd.Function):
    """y = x W^T + b  (PygLinearPass / head Linear; pnn_geometric_base.py:83-94)."""

    @staticmethod
    def forward(ctx, x, w, b):
        kind = _kind_of('linear', x)
        dtype = kind.dtype
        x, w, b = _c(x, dtype), _c(w, dtype), _c(b, dtype)
        _lib.require_hip(x, w, b)
        n, k = x.shape
        c = w.shape[0]
        y = torch.empty((n, c), dtype=dtype, device=x.device)
        kind.check(kind.linear_fwd(_lib.ptr(x), _lib.ptr(w), _lib.ptr(b), _lib.ptr(y), n, k, c, _stream(x.device)),
                   'linear_fwd')
        ctx.save_for_backward(x, w)
        ctx.has_bias, ctx.kind = b is not None, kind
        return y

    @staticmethod
    def backward(ctx, g_y):
        x, w = ctx.saved_tensors
        kind = ctx.kind
        g_y = _c(g_y, kind.dtype)
        n, k = x.shape
        c = w.shape[0]
        g_x = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        g_w = torch.empty_like(w)
        g_b = torch.empty((c,), dtype=kind.dtype, device=x.device) if ctx.has_bias else None
        ws_bytes = kind.linear_bwd_ws(n, k, c)
        ws = _ws(ws_bytes, x.device)
        kind.check(kind.linear_bwd(_lib.ptr(x), _lib.ptr(w), _lib.ptr(g_y), _lib.ptr(g_x), _lib.ptr(g_w), _lib.ptr(g_b),
                                   n, k, c, _lib.ptr(ws), ws_bytes, _stream(x.device)), 'linear_bwd')
        return g_x, g_w, g_b


def linear(x, weight, bias=None):
    squeeze = x.dim() == 1
    y = _LinearFn.apply(x.reshape(1, -1) if squeeze else x, weight, bias)
    return y.reshape(-1) if squeeze else y


def graphnorm_stats(y1, mean_scale, n_rows=None, out=None):
    """GraphNorm's statistics of y1 [N_cap, H] (fp32, H <= 256) as the layers compute them: a [2 H] tensor, the column
    means in front, behind them the column means of (y1 - mean_scale * mean)^2. n_rows None: over all rows (N_cap >= 1).
    n_rows a device int32 tensor with one element: over the first clamp(n_rows, 0, N_cap) rows, the count read on the
    device (PvsGraph.n_norm_rows_dev: rows behind it are never read, 0 gives zeros, n >= 1 the bits of the call on
    y1[:n]). No gradient: the layers' backward has its own kernels."""
    if y1.dim() != 2 or y1.dtype != _F32:
        raise TypeError(f'graphnorm_stats: y1 must be a float32 [N, H] tensor (got {y1.dtype}, {tuple(y1.shape)})')
    y1, mean_scale = y1.contiguous(), _c(mean_scale, _F32)
    _lib.require_hip(y1, mean_scale, n_rows)
    n_cap, hidden = int(y1.shape[0]), int(y1.shape[1])
    if mean_scale.numel() != hidden:
        raise ValueError(f'graphnorm_stats: mean_scale has {mean_scale.numel()} entries, y1 {hidden} columns')
    if n_rows is not None and not (n_rows.dtype == torch.int32 and n_rows.numel() == 1 and n_rows.is_contiguous()):
        raise ValueError('graphnorm_stats: n_rows must be a device int32 tensor with one element')
    lib = _lib.lib()
    dev = y1.device
    stats = torch.empty(2 * hidden, dtype=_F32, device=dev) if out is None else out
    ws_bytes = lib.pvs_graphnorm_stats_rows_workspace_bytes(n_cap, hidden)
    ws = _ws(ws_bytes, dev)
    _lib.check(lib.pvs_graphnorm_stats_rows(_lib.ptr(y1), _lib.ptr(mean_scale), n_cap, hidden, _lib.ptr(n_rows),
                                            _lib.ptr(stats), _lib.ptr(ws), ws_bytes, _stream(dev)),
               'pvs_graphnorm_stats_rows')
    return stats


def graphnorm_stats_segments(y1, mean_scale, seg_ptr, out=None):
    """GraphNorm's statistics of every row segment of y1 [N_cap, H] (fp32, H <= 256) as the layers compute them under
    `_lib.GRAPHNORM_SEGMENTS`: a [S, 2 H] tensor, row s the pair `graphnorm_stats` gives on y1[seg_ptr[s]:seg_ptr[s + 1]]
    alone, bit for bit. seg_ptr: a device int32 tensor [S + 1] (a node offset table), read on the device when the kernels
    run; every entry is clamped to [0, N_cap], a segment that ends in front of its start has length 0, and a segment of
    length 0 gives zeros. Rows outside every segment are never read. No gradient."""
    if y1.dim() != 2 or y1.dtype != _F32:
        raise TypeError(f'graphnorm_stats_segments: y1 must be a float32 [N, H] tensor (got {y1.dtype}, {tuple(y1.shape)})')
    y1, mean_scale = y1.contiguous(), _c(mean_scale, _F32)
    _lib.require_hip(y1, mean_scale, seg_ptr)
    n_cap, hidden = int(y1.shape[0]), int(y1.shape[1])
    if mean_scale.numel() != hidden:
        raise ValueError(f'graphnorm_stats_segments: mean_scale has {mean_scale.numel()} entries, y1 {hidden} columns')
    if not (torch.is_tensor(seg_ptr) and seg_ptr.dtype == torch.int32 and seg_ptr.dim() == 1 and seg_ptr.numel() >= 2
            and seg_ptr.is_contiguous()):
        raise ValueError('graphnorm_stats_segments: seg_ptr must be a contiguous device int32 tensor [S + 1], S >= 1')
    n_segs = int(seg_ptr.numel()) - 1
    lib = _lib.lib()
    dev = y1.device
    stats = torch.empty((n_segs, 2 * hidden), dtype=_F32, device=dev) if out is None else out
    if stats.shape != (n_segs, 2 * hidden) or stats.dtype != _F32 or not stats.is_contiguous() or stats.device != dev:
        raise ValueError(f'graphnorm_stats_segments: out must be a contiguous float32 [{n_segs}, {2 * hidden}] tensor on {dev}')
    ws_bytes = lib.pvs_graphnorm_stats_segments_workspace_bytes(n_cap, n_segs, hidden)
    ws = _ws(ws_bytes, dev)
    _lib.check(lib.pvs_graphnorm_stats_segments(_lib.ptr(y1), _lib.ptr(mean_scale), n_cap, hidden, _lib.ptr(seg_ptr), n_segs,
                                                _lib.ptr(stats), _lib.ptr(ws), ws_bytes, _stream(dev)),
               'pvs_graphnorm_stats_segments')
    return stats


class _MeanPoolFn(torch.autograd.Function):
    """global_mean_pool over contiguous per-graph node ranges (pnn_geometric_base.py:29-33)."""

    @staticmethod
    def forward(ctx, h, graph_ptr):
        kind = _kind_of('mean_pool', h)
        h = h.contiguous()
        _lib.require_hip(h, graph_ptr)
        b = graph_ptr.numel() - 1
        pooled = torch.empty((b, h.shape[1]), dtype=kind.dtype, device=h.device)
        kind.check(kind.mean_pool_fwd(_lib.ptr(h), _lib.ptr(graph_ptr), _lib.ptr(pooled), b, h.shape[1],
                                      _stream(h.device)), 'mean_pool_fwd')
        ctx.graph_ptr, ctx.n, ctx.kind = graph_ptr, h.shape[0], kind
        return pooled

    @staticmethod
    def backward(ctx, g):
        kind = ctx.kind
        g = _c(g, kind.dtype)
        b, width = g.shape
        g_h = torch.empty((ctx.n, width), dtype=kind.dtype, device=g.device)
        kind.check(kind.mean_pool_bwd(_lib.ptr(g), _lib.ptr(ctx.graph_ptr), _lib.ptr(g_h), b, ctx.n, width,
                                      _stream(g.device)), 'mean_pool_bwd')
        return g_h, None


def mean_pool(h, graph_ptr):
    """Mean of the rows [graph_ptr[g], graph_ptr[g + 1]) per graph (an empty graph gives zeros); a row outside
    [graph_ptr[0], graph_ptr[-1]) belongs to no graph: the forward ignores it, the backward gives it a zero gradient."""
    return _MeanPoolFn.apply(h, graph_ptr)


class _PoolHeadFn(torch.autograd.Function):
    """global_mean_pool + the head's first Linear in one launch, their backward in one launch
    (pnn_geometric_base.py:29-36, egnn_multitask.py:158-166)."""

    @staticmethod
    def forward(ctx, h, graph_ptr, w, b):
        h, w, b = _c(h, _F32, _FP32_ONLY), _c(w, _F32, _FP32_ONLY), _c(b, _F32, _FP32_ONLY)
        _lib.require_hip(h, graph_ptr, w, b)
        n_graphs, width, n_out = graph_ptr.numel() - 1, h.shape[1], w.shape[0]
        pooled = torch.empty((n_graphs, width), dtype=torch.float32, device=h.device)
        y = torch.empty((n_graphs, n_out), dtype=torch.float32, device=h.device)
        _lib.check(_lib.lib().pvs_pool_head_fwd(_lib.ptr(h), _lib.ptr(graph_ptr), _lib.ptr(w), _lib.ptr(b),
                                                _lib.ptr(pooled), _lib.ptr(y), n_graphs, width, n_out,
                                                _stream(h.device)), 'pvs_pool_head_fwd')
        ctx.save_for_backward(pooled, w)
        ctx.graph_ptr, ctx.n, ctx.has_bias = graph_ptr, h.shape[0], b is not None
        return y

    @staticmethod
    def backward(ctx, g_y):
        pooled, w = ctx.saved_tensors
        g_y = _c(g_y, _F32, _FP32_ONLY)
        n_graphs, width = pooled.shape
        n_out = w.shape[0]
        dev = g_y.device
        g_h = torch.empty((ctx.n, width), dtype=torch.float32, device=dev) if ctx.needs_input_grad[0] else None
        g_w = torch.empty_like(w)
        g_b = torch.empty((n_out,), dtype=torch.float32, device=dev) if ctx.has_bias else None
        _lib.check(_lib.lib().pvs_pool_head_bwd(_lib.ptr(g_y), _lib.ptr(pooled), _lib.ptr(w), _lib.ptr(ctx.graph_ptr),
                                                _lib.ptr(g_h), _lib.ptr(g_w), _lib.ptr(g_b), n_graphs, ctx.n, width,
                                                n_out, _stream(dev)), 'pvs_pool_head_bwd')
        return g_h, None, g_w, g_b


POOL_HEAD_MAX_WIDTH = 1024


def pool_head(h, graph_ptr, weight, bias=None):
    """linear(mean_pool(h, graph_ptr), weight, bias) as one op (hidden widths up to POOL_HEAD_MAX_WIDTH)."""
    return _PoolHeadFn.apply(h, graph_ptr, weight, bias)


MAX_POOL_HEADS = _lib.MAX_POOL_HEADS
HEAD_ACTS = {None: _lib.HEAD_NONE, 'relu': _lib.HEAD_RELU, 'softplus': _lib.HEAD_SOFTPLUS}


def _head_table(what, h, heads):
    """(h contiguous, the PvsHead table of `heads`, the tensors it points at, the columns they write in all) of
    `pool_heads` / `node_heads`; their refusals, worded with `what`."""
    heads = [(w, b, act) for w, b, act in heads]
    tensors = [h] + [t for w, b, _ in heads for t in (w, b) if t is not None]
    if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
        raise RuntimeError(f'{what} is forward only: call it under torch.no_grad() (training takes pool_head)')
    h = _c(h, _F32, _FP32_ONLY)
    _lib.require_hip(*tensors)
    width = h.shape[1]
    table, keep, col = (_lib.PvsHead * max(len(heads), 1))(), [], 0
    for i, (w, b, act) in enumerate(heads):
        if act not in HEAD_ACTS:
            raise ValueError(f'{what}: activation {act!r} (one of {sorted(k for k in HEAD_ACTS if k)} or None)')
        w, b = _c(w.detach(), _F32, _FP32_ONLY), _c(None if b is None else b.detach(), _F32, _FP32_ONLY)
        if w.dim() != 2 or w.shape[1] != width or (b is not None and b.numel() != w.shape[0]):
            raise ValueError(f'{what}: head {i}: weight {tuple(w.shape)} / bias on features of width {width}')
        keep += [w, b]
        table[i] = _lib.PvsHead(_lib.ptr(w), _lib.ptr(b), w.shape[0], HEAD_ACTS[act], col)
        col += w.shape[0]
    return h, table, len(heads), keep, col


def pool_heads(h, graph_ptr, heads, return_pooled=False):
    """Several heads on ONE pooled row per graph, in one launch, forward only (screening a two-headed model):
    heads = [(weight [C_i, width], bias [C_i] or None, act), ...], act None, 'relu' or 'softplus' (nn.Softplus()
    with its defaults). Returns y [B, sum C_i], the heads' columns side by side in the order given (and the pooled rows
    [B, width] with return_pooled). With act None a head's columns are bit for bit pool_head(h, graph_ptr, weight,
    bias). fp32 only; raises when autograd is recording and an input requires grad (there is no backward)."""
    h, table, n_heads, keep, col = _head_table('pool_heads', h, heads)
    _lib.require_hip(graph_ptr)
    n_graphs, width = graph_ptr.numel() - 1, h.shape[1]
    y = torch.empty((n_graphs, col), dtype=torch.float32, device=h.device)
    pooled = torch.empty((n_graphs, width), dtype=torch.float32, device=h.device) if return_pooled else None
    _lib.check(_lib.lib().pvs_pool_heads_fwd(_lib.ptr(h), _lib.ptr(graph_ptr), table, n_heads, _lib.ptr(pooled),
                                             _lib.ptr(y), n_graphs, width, col, _stream(h.device)),
               'pvs_pool_heads_fwd')
    return (y, pooled) if return_pooled else y


def node_heads(h, heads, out=None):
    """The heads of `pool_heads` on EVERY row of h [n, width] (pvs_node_heads_fwd; the class-activation map: the head
    applied to each node's final embedding): y [n, sum C_i], y[r] bit for bit what pool_heads gives for a graph that
    is row r alone. Same argument forms and refusals as pool_heads. `out`: an fp32 tensor [>= n, sum C_i] to write the
    first n rows of (a static buffer of a captured step). One launch, forward only, fp32 only."""
    h, table, n_heads, keep, col = _head_table('node_heads', h, heads)
    n, width = h.shape
    if out is None:
        out = torch.empty((n, col), dtype=torch.float32, device=h.device)
    _lib.require_hip(out)
    if out.dtype != torch.float32 or out.dim() != 2 or out.shape[0] < n or out.shape[1] != col:
        raise ValueError(f'node_heads: out = an fp32 tensor [>= {n}, {col}]')
    _lib.check(_lib.lib().pvs_node_heads_fwd(_lib.ptr(h), table, n_heads, _lib.ptr(out), n, width, col,
                                             _stream(h.device)), 'pvs_node_heads_fwd')
    return out[:n]


def segment_argmax(scores, seg_ptr, column=0):
    """The best row of every segment: scores [P, C] fp32, seg_ptr [L + 1] int32 on the device (ascending, inside
    [0, P]). Returns (best int32 [L], rows [L, C]): best[s] = the row of segment s, counted from its first, with the
    largest scores[:, column] (equal values: the lower row; a NaN never beats a number; -inf is a score), rows[s] =
    that row of scores; best = -1 and a row of NaNs for a segment without rows or with NaNs only. One launch, no
    atomics: the same bits every time."""
    scores = _c(scores, _F32, _FP32_ONLY)
    if scores.dim() != 2 or seg_ptr.dtype != torch.int32 or seg_ptr.dim() != 1 or seg_ptr.numel() < 1:
        raise ValueError('segment_argmax: scores [P, C] and an int32 seg_ptr [L + 1]')
    _lib.require_hip(scores, seg_ptr)
    n_cols, n_seg = scores.shape[1], seg_ptr.numel() - 1
    if scores.shape[0] == 0:        # (no rows: every segment is empty, the kernel reads none - but wants a pointer)
        scores = scores.new_zeros((1, n_cols))
    best = torch.empty(n_seg, dtype=torch.int32, device=scores.device)
    rows = torch.empty((n_seg, n_cols), dtype=torch.float32, device=scores.device)
    _lib.check(_lib.lib().pvs_segment_argmax(_lib.ptr(scores), n_cols, int(column), _lib.ptr(seg_ptr.contiguous()), n_seg,
                                             _lib.ptr(best), _lib.ptr(rows), _stream(scores.device)),
               'pvs_segment_argmax')
    return best, rows


def leave_out_ligand_pack(lig_pos, lig_feats, lig_ptr, first_copy, n_slots, slot_cap, out=None):
    """Leave-one-atom-out copies of a set of ligands as the slots of a pose batch (pvs_leave_out_ligand_pack).
    lig_pos [L, 3], lig_feats [L, F] fp32, lig_ptr [S + 1] int32, first_copy: one int32, all on the device. Ligand s owns
    the copies lig_ptr[s] + s ..: the whole ligand, then the ligand without atom 0, 1, ...; slot k of the batch holds
    copy first_copy + k (nothing past the last copy). Returns (out_pos [n_slots * slot_cap, 3], out_feats [.., F],
    out_ptr [n_slots + 1] int32, status [1] int32): the rows [out_ptr[k], out_ptr[k + 1]) are slot k's atoms, the rows
    from out_ptr[n_slots] on are not written. `out`: those four tensors to write into (at least that large). status:
    8 when lig_ptr does not ascend from 0 inside L or a ligand has more than slot_cap atoms (out_ptr all zeros, no
    row written). One launch, no atomics, no host synchronisation."""
    lig_pos, lig_feats = _c(lig_pos, _F32, _FP32_ONLY), _c(lig_feats, _F32, _FP32_ONLY)
    n_slots, slot_cap = int(n_slots), int(slot_cap)
    if (lig_pos.dim() != 2 or lig_pos.shape[1] != 3 or lig_feats.dim() != 2 or lig_feats.shape[0] != lig_pos.shape[0]
            or lig_feats.shape[1] < 1):
        raise ValueError('leave_out_ligand_pack: lig_pos [L, 3] and lig_feats [L, F] of the same L')
    if lig_ptr.dtype != torch.int32 or lig_ptr.dim() != 1 or lig_ptr.numel() < 1:
        raise ValueError('leave_out_ligand_pack: an int32 lig_ptr [S + 1]')
    if first_copy.dtype != torch.int32 or first_copy.numel() < 1:
        raise ValueError('leave_out_ligand_pack: first_copy is one int32 on the device')
    if n_slots < 1 or slot_cap < 1:
        raise ValueError(f'leave_out_ligand_pack: {n_slots} slots of up to {slot_cap} atoms')
    _lib.require_hip(lig_pos, lig_feats, lig_ptr, first_copy)
    dev, n_feats, rows = lig_pos.device, lig_feats.shape[1], n_slots * slot_cap
    if out is None:
        out = (torch.empty((rows, 3), dtype=torch.float32, device=dev),
               torch.empty((rows, n_feats), dtype=torch.float32, device=dev),
               torch.empty(n_slots + 1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    out_pos, out_feats, out_ptr, status = out
    _lib.require_hip(*out)
    if (out_pos.dtype != torch.float32 or out_feats.dtype != torch.float32 or out_pos.dim() != 2 or out_feats.dim() != 2
            or out_pos.shape[0] < rows or out_pos.shape[1] != 3 or out_feats.shape[0] < rows
            or out_feats.shape[1] != n_feats or out_ptr.dtype != torch.int32 or out_ptr.numel() != n_slots + 1
            or status.dtype != torch.int32 or status.numel() < 1):
        raise ValueError(f'leave_out_ligand_pack: out = (pos [>= {rows}, 3], feats [>= {rows}, {n_feats}], int32 ptr '
                         f'[{n_slots + 1}], int32 status [1])')
    _lib.check(_lib.lib().pvs_leave_out_ligand_pack(
        _lib.ptr(lig_pos), _lib.ptr(lig_feats), _lib.ptr(lig_ptr), lig_ptr.numel() - 1, lig_pos.shape[0], n_feats,
        _lib.ptr(first_copy), n_slots, slot_cap, _lib.ptr(out_pos), _lib.ptr(out_feats), _lib.ptr(out_ptr),
        _lib.ptr(status), _stream(dev)), 'pvs_leave_out_ligand_pack')
    return out_pos, out_feats, out_ptr, status


def contact_pairs(lig_pos, lig_ptr, rec_pos, radius, host_ptr=False):
    """The ligand-receptor contacts of packed hits (pvs_contact_pairs_count / _fill): lig_pos [L, 3] fp32, lig_ptr
    [S + 1] int32 (hit s: the rows lig_ptr[s] .. lig_ptr[s + 1]) and rec_pos [n_rec, 3] fp32, all on the device. A pair
    (a, r) - ligand atom a counted inside its hit, receptor atom r - is a contact exactly when the pose-batch builders
    write a class-1 edge for it at inter radius `radius` (the same fp64 distance and compares). Returns (pairs [K, 2]
    int32, pair_ptr [S + 1] int32): the rows pair_ptr[s] .. pair_ptr[s + 1] are hit s's contacts, sorted by a then r.
    K = pair_ptr[S] is read back once (the call's one wait for the device); ValueError when lig_ptr does not ascend
    from 0 inside L. host_ptr: that one copy brings the whole pair_ptr, returned third (a host int32 tensor)."""
    lig_pos, rec_pos = _c(lig_pos, _F32, _FP32_ONLY), _c(rec_pos, _F32, _FP32_ONLY)
    if lig_pos.dim() != 2 or lig_pos.shape[1] != 3 or rec_pos.dim() != 2 or rec_pos.shape[1] != 3 or rec_pos.shape[0] < 1:
        raise ValueError('contact_pairs: lig_pos [L, 3] and rec_pos [n_rec >= 1, 3]')
    if lig_ptr.dtype != torch.int32 or lig_ptr.dim() != 1 or lig_ptr.numel() < 1:
        raise ValueError('contact_pairs: an int32 lig_ptr [S + 1]')
    if not float(radius) > 0:
        raise ValueError(f'contact_pairs: radius must be positive (got {radius})')
    if lig_pos.shape[0] * rec_pos.shape[0] >= 2 ** 31:
        raise ValueError('contact_pairs: L * n_rec passes 2^31')
    _lib.require_hip(lig_pos, lig_ptr, rec_pos)
    dev, n_hits = lig_pos.device, lig_ptr.numel() - 1
    lig_ptr = lig_ptr.contiguous()
    pair_ptr = torch.empty(n_hits + 1, dtype=torch.int32, device=dev)
    args = (_lib.ptr(lig_pos), _lib.ptr(lig_ptr), n_hits, lig_pos.shape[0], _lib.ptr(rec_pos), rec_pos.shape[0],
            float(radius), _lib.ptr(pair_ptr))
    _lib.check(_lib.lib().pvs_contact_pairs_count(*args, _stream(dev)), 'pvs_contact_pairs_count')
    on_host = pair_ptr.cpu() if host_ptr else pair_ptr[n_hits:].cpu()
    n_pairs = int(on_host[-1])
    if n_pairs < 0:
        raise ValueError('contact_pairs: lig_ptr is not an ascending table from 0 inside lig_pos')
    pairs = torch.empty((n_pairs, 2), dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().pvs_contact_pairs_fill(*args, n_pairs, _lib.ptr(pairs), _stream(dev)),
               'pvs_contact_pairs_fill')
    return (pairs, pair_ptr, on_host) if host_ptr else (pairs, pair_ptr)


def leave_out_pair_pack(lig_pos, lig_feats, lig_ptr, pairs, pair_ptr, n_rec, first_copy, n_slots, slot_cap, out=None):
    """Copies of a set of hits that leave out one ligand-receptor pair each, as the slots of a struck pose batch
    (pvs_leave_out_pair_pack). lig_pos [L, 3], lig_feats [L, F] fp32, lig_ptr [S + 1] int32, pairs [K, 2] int32 (ligand
    atom a counted inside its hit or -1, receptor atom r or -1), pair_ptr [S + 1] int32 (hit s: the rows pair_ptr[s] ..
    pair_ptr[s + 1] of pairs), first_copy: one int32, all on the device. Hit s owns the copies pair_ptr[s] + s ..: the
    whole ligand, then one per row of its pairs; slot k of the batch holds copy first_copy + k (nothing past the last
    copy). Returns (out_pos [n_slots * slot_cap, 3], out_feats [.., F], out_ptr [n_slots + 1] int32, rec_drop [n_slots]
    int32, status [1] int32): the hit's rows without atom a, and rec_drop[k] = r (-1: the whole receptor). `out`: those
    five tensors to write into. status: 8 when lig_ptr or pair_ptr does not ascend from 0 inside L / K, a ligand has
    more than slot_cap atoms or a pair of one of the batch's copies is outside its hit or the receptor (out_ptr all
    zeros, rec_drop all -1, no row written). One launch, no atomics, no host synchronisation."""
    lig_pos, lig_feats = _c(lig_pos, _F32, _FP32_ONLY), _c(lig_feats, _F32, _FP32_ONLY)
    n_slots, slot_cap, n_rec = int(n_slots), int(slot_cap), int(n_rec)
    if (lig_pos.dim() != 2 or lig_pos.shape[1] != 3 or lig_feats.dim() != 2 or lig_feats.shape[0] != lig_pos.shape[0]
            or lig_feats.shape[1] < 1):
        raise ValueError('leave_out_pair_pack: lig_pos [L, 3] and lig_feats [L, F] of the same L')
    if lig_ptr.dtype != torch.int32 or lig_ptr.dim() != 1 or lig_ptr.numel() < 1:
        raise ValueError('leave_out_pair_pack: an int32 lig_ptr [S + 1]')
    if pair_ptr.dtype != torch.int32 or pair_ptr.dim() != 1 or pair_ptr.numel() != lig_ptr.numel():
        raise ValueError('leave_out_pair_pack: an int32 pair_ptr [S + 1], as long as lig_ptr')
    if pairs.dtype != torch.int32 or pairs.dim() != 2 or pairs.shape[1] != 2 or not pairs.is_contiguous():
        raise ValueError('leave_out_pair_pack: contiguous int32 pairs [K, 2]')
    if first_copy.dtype != torch.int32 or first_copy.numel() < 1:
        raise ValueError('leave_out_pair_pack: first_copy is one int32 on the device')
    if n_slots < 1 or slot_cap < 1 or n_rec < 1:
        raise ValueError(f'leave_out_pair_pack: {n_slots} slots of up to {slot_cap} atoms against {n_rec} receptor atoms')
    _lib.require_hip(lig_pos, lig_feats, lig_ptr, pairs, pair_ptr, first_copy)
    dev, n_feats, rows = lig_pos.device, lig_feats.shape[1], n_slots * slot_cap
    if out is None:
        out = (torch.empty((rows, 3), dtype=torch.float32, device=dev),
               torch.empty((rows, n_feats), dtype=torch.float32, device=dev),
               torch.empty(n_slots + 1, dtype=torch.int32, device=dev),
               torch.empty(n_slots, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    out_pos, out_feats, out_ptr, rec_drop, status = out
    _lib.require_hip(*out)
    if (out_pos.dtype != torch.float32 or out_feats.dtype != torch.float32 or out_pos.dim() != 2 or out_feats.dim() != 2
            or out_pos.shape[0] < rows or out_pos.shape[1] != 3 or out_feats.shape[0] < rows
            or out_feats.shape[1] != n_feats or out_ptr.dtype != torch.int32 or out_ptr.numel() != n_slots + 1
            or rec_drop.dtype != torch.int32 or rec_drop.numel() != n_slots
            or status.dtype != torch.int32 or status.numel() < 1):
        raise ValueError(f'leave_out_pair_pack: out = (pos [>= {rows}, 3], feats [>= {rows}, {n_feats}], int32 ptr '
                         f'[{n_slots + 1}], int32 rec_drop [{n_slots}], int32 status [1])')
    _lib.check(_lib.lib().pvs_leave_out_pair_pack(
        _lib.ptr(lig_pos), _lib.ptr(lig_feats), _lib.ptr(lig_ptr), _lib.ptr(pairs), _lib.ptr(pair_ptr),
        lig_ptr.numel() - 1, lig_pos.shape[0], pairs.shape[0], n_feats, n_rec, _lib.ptr(first_copy), n_slots, slot_cap,
        _lib.ptr(out_pos), _lib.ptr(out_feats), _lib.ptr(out_ptr), _lib.ptr(rec_drop), _lib.ptr(status), _stream(dev)),
        'pvs_leave_out_pair_pack')
    return out_pos, out_feats, out_ptr, rec_drop, status


def leave_out_parent_pack(lig_pos, lig_ptr, copy_ptr, first_copy, n_slots, slot_cap, out=None):
    """The PARENTS' atoms for the slots of a leave-out batch (pvs_leave_out_parent_pack): what the slots of a cropped
    copies batch are cropped around. lig_pos [L, 3] fp32, lig_ptr [S + 1] int32, copy_ptr [S + 1] int32 (hit s owns the
    copies copy_ptr[s] + s .. copy_ptr[s + 1] + s: lig_ptr itself for leave_out_ligand_pack's copies, pair_ptr for
    leave_out_pair_pack's), first_copy: one int32, all on the device. Slot k holds copy first_copy + k and gets the WHOLE
    hit's atoms (nothing past the last copy). Returns (out_pos [n_slots * slot_cap, 3], out_ptr [n_slots + 1] int32,
    status [1] int32); `out`: those three tensors to write into. status: 8 when lig_ptr or copy_ptr does not ascend from
    0 (lig_ptr inside L) or a hit has more than slot_cap atoms (out_ptr all zeros, no row written). One launch, no
    atomics, no host synchronisation."""
    lig_pos = _c(lig_pos, _F32, _FP32_ONLY)
    n_slots, slot_cap = int(n_slots), int(slot_cap)
    if lig_pos.dim() != 2 or lig_pos.shape[1] != 3:
        raise ValueError('leave_out_parent_pack: lig_pos [L, 3]')
    if lig_ptr.dtype != torch.int32 or lig_ptr.dim() != 1 or lig_ptr.numel() < 1:
        raise ValueError('leave_out_parent_pack: an int32 lig_ptr [S + 1]')
    if copy_ptr.dtype != torch.int32 or copy_ptr.dim() != 1 or copy_ptr.numel() != lig_ptr.numel():
        raise ValueError('leave_out_parent_pack: an int32 copy_ptr [S + 1], as long as lig_ptr')
    if first_copy.dtype != torch.int32 or first_copy.numel() < 1:
        raise ValueError('leave_out_parent_pack: first_copy is one int32 on the device')
    if n_slots < 1 or slot_cap < 1:
        raise ValueError(f'leave_out_parent_pack: {n_slots} slots of up to {slot_cap} atoms')
    _lib.require_hip(lig_pos, lig_ptr, copy_ptr, first_copy)
    dev, rows = lig_pos.device, n_slots * slot_cap
    if out is None:
        out = (torch.empty((rows, 3), dtype=torch.float32, device=dev),
               torch.empty(n_slots + 1, dtype=torch.int32, device=dev), torch.empty(1, dtype=torch.int32, device=dev))
    out_pos, out_ptr, status = out
    _lib.require_hip(*out)
    if (out_pos.dtype != torch.float32 or out_pos.dim() != 2 or out_pos.shape[0] < rows or out_pos.shape[1] != 3
            or out_ptr.dtype != torch.int32 or out_ptr.numel() != n_slots + 1 or status.dtype != torch.int32
            or status.numel() < 1):
        raise ValueError(f'leave_out_parent_pack: out = (pos [>= {rows}, 3], int32 ptr [{n_slots + 1}], int32 status '
                         '[1])')
    _lib.check(_lib.lib().pvs_leave_out_parent_pack(
        _lib.ptr(lig_pos), _lib.ptr(lig_ptr.contiguous()), _lib.ptr(copy_ptr.contiguous()), lig_ptr.numel() - 1,
        lig_pos.shape[0], _lib.ptr(first_copy), n_slots, slot_cap, _lib.ptr(out_pos), _lib.ptr(out_ptr),
        _lib.ptr(status), _stream(dev)), 'pvs_leave_out_parent_pack')
    return out_pos, out_ptr, status


def crop_keep(lig_pos, lig_ptr, rec_pos, crop_radius, host_ptr=False):
    """Which receptor atoms the cropped complex of each packed hit keeps (pvs_crop_keep: the keep decision of the
    cropped pose-batch builders, by the same kernel, without building anything). lig_pos [L, 3] fp32, lig_ptr [S + 1]
    int32 (a hit has up to 1024 atoms), rec_pos [n_rec, 3] fp32, all on the device. Returns (keep [S, ceil(n_rec / 64)]
    int64: bit j % 64 of word j / 64 of row s is set when some atom of hit s is closer to receptor atom j than
    crop_radius; kept_ptr [S + 1] int32, the exclusive scan of the kept counts). kept_ptr[S] is read back once (the
    call's one wait for the device); ValueError when lig_ptr is no such table inside L. host_ptr: that one copy brings
    the whole kept_ptr, returned third (a host int32 tensor)."""
    lig_pos, rec_pos = _c(lig_pos, _F32, _FP32_ONLY), _c(rec_pos, _F32, _FP32_ONLY)
    if lig_pos.dim() != 2 or lig_pos.shape[1] != 3 or rec_pos.dim() != 2 or rec_pos.shape[1] != 3 or rec_pos.shape[0] < 1:
        raise ValueError('crop_keep: lig_pos [L, 3] and rec_pos [n_rec >= 1, 3]')
    if lig_ptr.dtype != torch.int32 or lig_ptr.dim() != 1 or lig_ptr.numel() < 1:
        raise ValueError('crop_keep: an int32 lig_ptr [S + 1]')
    if not float(crop_radius) > 0:
        raise ValueError(f'crop_keep: crop_radius must be positive (got {crop_radius})')
    _lib.require_hip(lig_pos, lig_ptr, rec_pos)
    dev, n_hits, n_rec = lig_pos.device, lig_ptr.numel() - 1, rec_pos.shape[0]
    keep = torch.empty((n_hits, (n_rec + 63) // 64), dtype=torch.int64, device=dev)
    kept_ptr = torch.empty(n_hits + 1, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().pvs_crop_keep(_lib.ptr(lig_pos), _lib.ptr(lig_ptr.contiguous()), n_hits, lig_pos.shape[0],
                                        _lib.ptr(rec_pos), n_rec, float(crop_radius), _lib.ptr(keep), _lib.ptr(kept_ptr),
                                        _stream(dev)), 'pvs_crop_keep')
    on_host = kept_ptr.cpu() if host_ptr else kept_ptr[n_hits:].cpu()
    if int(on_host[-1]) < 0:
        raise ValueError('crop_keep: lig_ptr is not an ascending table from 0 of hits of up to 1024 atoms inside lig_pos')
    return (keep, kept_ptr, on_host) if host_ptr else (keep, kept_ptr)


def kept_atoms(keep, n_rec):
    """The set bits of keep masks [S, ceil(n_rec / 64)] int64 as (hit [M] int64, receptor atom [M] int64), ascending by
    hit, then by atom, made on the device."""
    bits = torch.arange(64, device=keep.device, dtype=torch.int64)
    on = ((keep.unsqueeze(2) >> bits) & 1).reshape(keep.shape[0], -1)[:, :int(n_rec)].bool()
    hit, atom = on.nonzero(as_tuple=True)
    return hit, atom


def screen_copies_state_bytes(job):
    """The bytes of state that pvs_screen_copies_build needs for `job` (a _lib.PvsScreenCopiesJob; only its layout and
    counts are read); ValueError for counts or a layout that the build refuses."""
    if not isinstance(job, _lib.PvsScreenCopiesJob):
        raise ValueError('screen_copies_state_bytes: a _lib.PvsScreenCopiesJob')
    n = int(_lib.lib().pvs_screen_copies_state_bytes(C.byref(job)))
    if n == 0:
        raise ValueError('screen_copies_state_bytes: the job is not PVS_SLOTS_CROPPED, or its counts (n_slots, lig_cap, '
                         'n_rec, slot_cap, crop_cap) are ones that pvs_screen_copies_build refuses')
    return n


def screen_copies_build(job, state):
    """pvs_screen_copies_build of `job` (a _lib.PvsScreenCopiesJob of device addresses) with the scratch `state` (a
    uint8 tensor on the device, at least screen_copies_state_bytes(job)), on the current stream of the state's device.
    Everything the entry refuses it refuses by name before any launch (RuntimeError with its words)."""
    if not isinstance(job, _lib.PvsScreenCopiesJob):
        raise ValueError('screen_copies_build: a _lib.PvsScreenCopiesJob')
    if state.dtype != torch.uint8 or not state.is_contiguous():
        raise ValueError('screen_copies_build: state is a contiguous uint8 tensor')
    _lib.require_hip(state)
    _lib.check(_lib.lib().pvs_screen_copies_build(C.byref(job), _lib.ptr(state), state.numel(), _stream(state.device)),
               'pvs_screen_copies_build')


def new_contact_accumulators(n_rec, device):
    """Fresh accumulators of `contact_attention`: (rec_sum [n_rec] float64 zeros, rec_count [n_rec] int32 zeros,
    rec_max [n_rec] float32 NaN: none so far)."""
    return (torch.zeros(n_rec, dtype=torch.float64, device=device), torch.zeros(n_rec, dtype=torch.int32, device=device),
            torch.full((n_rec,), float('nan'), dtype=torch.float32, device=device))


def contact_attention(rowptr, etype, att, node_ptr, lig_ptr, n_rec, out=None):
    """Contact attention of a pose batch (pvs_contact_attention): rowptr [N + 1] int32 / etype [E] uint8 - either CSR
    of a compact pose batch (slot p: the rows node_ptr[p] .. node_ptr[p + 1], its lig_ptr[p + 1] - lig_ptr[p] ligand
    atoms, then the n_rec receptor atoms; node_ptr, lig_ptr [n_slots + 1] int32) - and att [>= E] fp32, one value per
    edge in that CSR's order, all on the device. Returns (lig_att [N - n_slots * n_rec], slot_rec_att [n_slots, n_rec],
    rec_sum [n_rec] float64, rec_count [n_rec] int32, rec_max [n_rec]): per packed ligand atom and per (slot, receptor
    atom) the largest att over the row's class-1 (ligand-receptor) edges, NaN without one (NaN values are skipped; the
    lig_att rows from lig_ptr[n_slots] on are not written); rec_sum / rec_count / rec_max are UPDATED with the slot
    values that are not NaN, in slot order (fresh ones: new_contact_accumulators). `out`: those five tensors to write
    into and accumulate on. Two launches, no atomics, no host synchronisation: the same bits every time."""
    att = _c(att, _F32, _FP32_ONLY)
    n_rec = int(n_rec)
    if (rowptr.dtype != torch.int32 or rowptr.dim() != 1 or rowptr.numel() < 1 or etype.dtype != torch.uint8
            or etype.dim() != 1 or att.dim() != 1 or att.numel() < etype.numel()):
        raise ValueError('contact_attention: an int32 rowptr [N + 1], a uint8 etype [E] and att [>= E]')
    if (node_ptr.dtype != torch.int32 or lig_ptr.dtype != torch.int32 or node_ptr.dim() != 1 or node_ptr.numel() < 1
            or lig_ptr.shape != node_ptr.shape):
        raise ValueError('contact_attention: int32 node_ptr and lig_ptr [n_slots + 1]')
    n_nodes, n_edges, n_slots = rowptr.numel() - 1, etype.numel(), node_ptr.numel() - 1
    if n_rec < 0 or n_slots * n_rec > n_nodes:
        raise ValueError(f'contact_attention: {n_nodes} rows cannot hold {n_slots} slots of {n_rec} receptor atoms')
    _lib.require_hip(rowptr, etype, att, node_ptr, lig_ptr)
    dev, n_lig = att.device, n_nodes - n_slots * n_rec
    if out is None:
        out = (torch.full((n_lig,), float('nan'), dtype=torch.float32, device=dev),
               torch.empty((n_slots, n_rec), dtype=torch.float32, device=dev)) + new_contact_accumulators(n_rec, dev)
    lig_att, slot_rec_att, rec_sum, rec_count, rec_max = out
    _lib.require_hip(*out)
    if (lig_att.dtype != torch.float32 or slot_rec_att.dtype != torch.float32 or rec_sum.dtype != torch.float64
            or rec_count.dtype != torch.int32 or rec_max.dtype != torch.float32 or lig_att.dim() != 1
            or lig_att.numel() < n_lig or slot_rec_att.shape != (n_slots, n_rec) or rec_sum.shape != (n_rec,)
            or rec_count.shape != (n_rec,) or rec_max.shape != (n_rec,)):
        raise ValueError(f'contact_attention: out = (lig_att [>= {n_lig}], slot_rec_att [{n_slots}, {n_rec}], float64 '
                         f'rec_sum [{n_rec}], int32 rec_count [{n_rec}], rec_max [{n_rec}])')
    _lib.check(_lib.lib().pvs_contact_attention(
        _lib.ptr(rowptr), _lib.ptr(etype), _lib.ptr(att), n_nodes, n_edges, _lib.ptr(node_ptr), _lib.ptr(lig_ptr),
        n_slots, n_rec, _lib.ptr(lig_att), _lib.ptr(slot_rec_att), _lib.ptr(rec_sum), _lib.ptr(rec_count),
        _lib.ptr(rec_max), _stream(dev)), 'pvs_contact_attention')
    return lig_att, slot_rec_att, rec_sum, rec_count, rec_max


def slot_node_values(y, node_ptr, lig_ptr, n_rec, column=0, n_mean=1, out=None):
    """`contact_attention`'s reduction over a value that every node has (pvs_slot_node_values): y [N, C] fp32 holds one
    row per node of a compact pose batch (slot p: the rows node_ptr[p] .. node_ptr[p + 1], its lig_ptr[p + 1] -
    lig_ptr[p] ligand atoms, then the n_rec receptor atoms; node_ptr, lig_ptr [n_slots + 1] int32), all on the device.
    A node's value is y[r, column] (n_mean 1) or ((y[r, column] + y[r, column + 1]) + y[r, column + 2]) / 3 (n_mean 3).
    Returns (lig_val [N - n_slots * n_rec], slot_rec_val [n_slots, n_rec], rec_sum [n_rec] float64, rec_count [n_rec]
    int32, rec_max [n_rec]): the value of every packed ligand atom (the rows from lig_ptr[n_slots] on are not
    written) and of every (slot, receptor atom) - a row of NaN for a slot without ligand atoms or with broken tables;
    rec_sum / rec_count / rec_max are UPDATED with the slot values that are not NaN, in slot order (fresh ones:
    new_contact_accumulators). `out`: those five tensors to write into and accumulate on. Two launches, no atomics, no
    host synchronisation: the same bits every time."""
    y = _c(y, _F32, _FP32_ONLY)
    n_rec, column, n_mean = int(n_rec), int(column), int(n_mean)
    if y.dim() != 2 or y.shape[1] < 1:
        raise ValueError('slot_node_values: y [N, C]')
    if n_mean not in (1, 3) or not 0 <= column <= y.shape[1] - n_mean:
        raise ValueError(f'slot_node_values: column {column}, n_mean {n_mean}: one column or the mean of three, inside '
                         f'the {y.shape[1]} of y')
    if (node_ptr.dtype != torch.int32 or lig_ptr.dtype != torch.int32 or node_ptr.dim() != 1 or node_ptr.numel() < 1
            or lig_ptr.shape != node_ptr.shape):
        raise ValueError('slot_node_values: int32 node_ptr and lig_ptr [n_slots + 1]')
    n_nodes, n_slots = y.shape[0], node_ptr.numel() - 1
    if n_rec < 0 or n_slots * n_rec > n_nodes:
        raise ValueError(f'slot_node_values: {n_nodes} rows cannot hold {n_slots} slots of {n_rec} receptor atoms')
    _lib.require_hip(y, node_ptr, lig_ptr)
    dev, n_lig = y.device, n_nodes - n_slots * n_rec
    if out is None:
        out = (torch.full((n_lig,), float('nan'), dtype=torch.float32, device=dev),
               torch.empty((n_slots, n_rec), dtype=torch.float32, device=dev)) + new_contact_accumulators(n_rec, dev)
    lig_val, slot_rec_val, rec_sum, rec_count, rec_max = out
    _lib.require_hip(*out)
    if (lig_val.dtype != torch.float32 or slot_rec_val.dtype != torch.float32 or rec_sum.dtype != torch.float64
            or rec_count.dtype != torch.int32 or rec_max.dtype != torch.float32 or lig_val.dim() != 1
            or lig_val.numel() < n_lig or slot_rec_val.shape != (n_slots, n_rec) or rec_sum.shape != (n_rec,)
            or rec_count.shape != (n_rec,) or rec_max.shape != (n_rec,)):
        raise ValueError(f'slot_node_values: out = (lig_val [>= {n_lig}], slot_rec_val [{n_slots}, {n_rec}], float64 '
                         f'rec_sum [{n_rec}], int32 rec_count [{n_rec}], rec_max [{n_rec}])')
    _lib.check(_lib.lib().pvs_slot_node_values(
        _lib.ptr(y), y.shape[1], column, n_mean, n_nodes, _lib.ptr(node_ptr.contiguous()), _lib.ptr(lig_ptr.contiguous()),
        n_slots, n_rec, _lib.ptr(lig_val), _lib.ptr(slot_rec_val), _lib.ptr(rec_sum), _lib.ptr(rec_count),
        _lib.ptr(rec_max), _stream(dev)), 'pvs_slot_node_values')
    return lig_val, slot_rec_val, rec_sum, rec_count, rec_max


def _cropped_tables(who, node_ptr, lig_ptr, keep, n_rec):
    """The slot tables of a cropped pose batch, checked: n_slots."""
    if (node_ptr.dtype != torch.int32 or lig_ptr.dtype != torch.int32 or node_ptr.dim() != 1 or node_ptr.numel() < 1
            or lig_ptr.shape != node_ptr.shape):
        raise ValueError(f'{who}: int32 node_ptr and lig_ptr [n_slots + 1]')
    n_slots = node_ptr.numel() - 1
    if n_rec < 0:
        raise ValueError(f'{who}: {n_rec} receptor atoms')
    if keep.dtype != torch.int64 or keep.shape != (n_slots, (n_rec + 63) // 64) or not keep.is_contiguous():
        raise ValueError(f'{who}: keep is a contiguous int64 tensor [{n_slots}, {(n_rec + 63) // 64}]: one mask of '
                         f'{n_rec} receptor atoms per slot, atom j bit j % 64 of word j / 64')
    return n_slots


def _cropped_out(who, out, lig_room, n_slots, n_rec, dev, names):
    """The five outputs of a cropped reduction: `out`, checked, or fresh ones with lig_room ligand rows of NaN."""
    if out is None:
        if lig_room is None:
            raise ValueError(f'{who}: the ligand rows of a cropped batch are known on the device only - give lig_room '
                             '(the ligand output then has that many rows, NaN-filled) or out')
        out = (torch.full((int(lig_room),), float('nan'), dtype=torch.float32, device=dev),
               torch.empty((n_slots, n_rec), dtype=torch.float32, device=dev)) + new_contact_accumulators(n_rec, dev)
    lig, slot_rec, rec_sum, rec_count, rec_max = out
    _lib.require_hip(*out)
    if (lig.dtype != torch.float32 or slot_rec.dtype != torch.float32 or rec_sum.dtype != torch.float64
            or rec_count.dtype != torch.int32 or rec_max.dtype != torch.float32 or lig.dim() != 1
            or (lig_room is not None and lig.numel() < int(lig_room)) or slot_rec.shape != (n_slots, n_rec)
            or rec_sum.shape != (n_rec,) or rec_count.shape != (n_rec,) or rec_max.shape != (n_rec,)
            or not all(t.is_contiguous() for t in out)):
        room = '>= lig_ptr[n_slots]' if lig_room is None else f'>= {int(lig_room)}'
        raise ValueError(f'{who}: out = ({names[0]} [{room}], {names[1]} [{n_slots}, {n_rec}], float64 rec_sum [{n_rec}], '
                         f'int32 rec_count [{n_rec}], rec_max [{n_rec}]), contiguous')
    return out


def contact_attention_cropped(rowptr, etype, att, node_ptr, lig_ptr, keep, n_rec, lig_room=None, out=None):
    """`contact_attention` over a CROPPED pose batch (pvs_contact_attention_cropped): slot p owns the rows node_ptr[p] ..
    node_ptr[p + 1], its lig_ptr[p + 1] - lig_ptr[p] ligand atoms, then the receptor atoms whose bit is set in keep[p]
    (keep [n_slots, ceil(n_rec / 64)] int64 on the device, atom j bit j % 64 of word j / 64: LibraryScreen.keep), in
    receptor order. Returns the five tensors of `contact_attention`; slot_rec_att[p, j] is NaN for an atom that slot p
    does not keep, so rec_count[j] grows by the slots that keep j and in which it has a contact. The host does not know
    how many ligand rows there are: without `out`, lig_att has `lig_room` rows (at least lig_ptr[n_slots]), NaN-filled;
    with `out`, its lig_att holds at least lig_ptr[n_slots] (and lig_room, if given). Two launches, no atomics, no host
    synchronisation: the same bits every time."""
    who = 'contact_attention_cropped'
    att = _c(att, _F32, _FP32_ONLY)
    n_rec = int(n_rec)
    if (rowptr.dtype != torch.int32 or rowptr.dim() != 1 or rowptr.numel() < 1 or etype.dtype != torch.uint8
            or etype.dim() != 1 or att.dim() != 1 or att.numel() < etype.numel()):
        raise ValueError(f'{who}: an int32 rowptr [N + 1], a uint8 etype [E] and att [>= E]')
    n_slots = _cropped_tables(who, node_ptr, lig_ptr, keep, n_rec)
    n_nodes, n_edges = rowptr.numel() - 1, etype.numel()
    _lib.require_hip(rowptr, etype, att, node_ptr, lig_ptr, keep)
    out = _cropped_out(who, out, lig_room, n_slots, n_rec, att.device, ('lig_att', 'slot_rec_att'))
    _lib.check(_lib.lib().pvs_contact_attention_cropped(
        _lib.ptr(rowptr), _lib.ptr(etype), _lib.ptr(att), n_nodes, n_edges, _lib.ptr(node_ptr), _lib.ptr(lig_ptr),
        _lib.ptr(keep), n_slots, n_rec, *(_lib.ptr(t) for t in out), _stream(att.device)),
        'pvs_contact_attention_cropped')
    return out


def slot_node_values_cropped(y, node_ptr, lig_ptr, keep, n_rec, column=0, n_mean=1, lig_room=None, out=None):
    """`slot_node_values` over a CROPPED pose batch (pvs_slot_node_values_cropped; the layout and `keep` as for
    `contact_attention_cropped`): slot_rec_val[p, j] is the node value of receptor atom j where slot p keeps it and has
    ligand atoms, NaN otherwise, so rec_count[j] grows by the slots that keep j. lig_room / out as there."""
    who = 'slot_node_values_cropped'
    y = _c(y, _F32, _FP32_ONLY)
    n_rec, column, n_mean = int(n_rec), int(column), int(n_mean)
    if y.dim() != 2 or y.shape[1] < 1:
        raise ValueError(f'{who}: y [N, C]')
    if n_mean not in (1, 3) or not 0 <= column <= y.shape[1] - n_mean:
        raise ValueError(f'{who}: column {column}, n_mean {n_mean}: one column or the mean of three, inside the '
                         f'{y.shape[1]} of y')
    n_slots = _cropped_tables(who, node_ptr, lig_ptr, keep, n_rec)
    _lib.require_hip(y, node_ptr, lig_ptr, keep)
    out = _cropped_out(who, out, lig_room, n_slots, n_rec, y.device, ('lig_val', 'slot_rec_val'))
    _lib.check(_lib.lib().pvs_slot_node_values_cropped(
        _lib.ptr(y), y.shape[1], column, n_mean, y.shape[0], _lib.ptr(node_ptr), _lib.ptr(lig_ptr), _lib.ptr(keep),
        n_slots, n_rec, *(_lib.ptr(t) for t in out), _stream(y.device)), 'pvs_slot_node_values_cropped')
    return out


HIT_RANK_TILE = 1024        # csrc/hit_ranks.h: kPvsRankTile, the candidates one workgroup stages in LDS at a time
HIT_RANK_MAX_LIGAND = 1024  # csrc/contact_attention.h: kPvsContactMaxLigand


def _checked_accumulators(who, acc, n_rec):
    """`acc`, a `new_contact_accumulators` triple over n_rec atoms on the device, checked."""
    if acc is None or len(acc) != 3:
        raise ValueError(f'{who}: acc = (float64 sum [{n_rec}], int32 count [{n_rec}], float32 max [{n_rec}]) - '
                         'new_contact_accumulators')
    rec_sum, rec_count, rec_max = acc
    _lib.require_hip(*acc)
    if (rec_sum.dtype != torch.float64 or rec_count.dtype != torch.int32 or rec_max.dtype != torch.float32
            or rec_sum.shape != (n_rec,) or rec_count.shape != (n_rec,) or rec_max.shape != (n_rec,)
            or not all(t.is_contiguous() for t in acc)):
        raise ValueError(f'{who}: acc = (float64 sum [{n_rec}], int32 count [{n_rec}], float32 max [{n_rec}]), '
                         'contiguous')
    return acc


def hit_rows_accumulate(rows, acc):
    """`contact_attention`'s accumulation by itself (pvs_hit_rows_accumulate): rows [n_hits, n_rec] fp32 on the device,
    NaN = no value; acc, a `new_contact_accumulators` triple, is UPDATED with every column's values that are not NaN,
    in hit order, and returned. One launch, no atomics: the same bits every time."""
    who = 'hit_rows_accumulate'
    rows = _c(rows, _F32, _FP32_ONLY)
    if rows.dim() != 2:
        raise ValueError(f'{who}: rows [n_hits, n_rec]')
    _lib.require_hip(rows)
    n_hits, n_rec = rows.shape
    acc = _checked_accumulators(who, acc, n_rec)
    _lib.check(_lib.lib().pvs_hit_rows_accumulate(_lib.ptr(rows), n_hits, n_rec, *(_lib.ptr(t) for t in acc),
                                                  _stream(rows.device)), 'pvs_hit_rows_accumulate')
    return acc


def hit_value_ranks(rows, lig_val=None, lig_ptr=None, out=None, acc=None):
    """Per-hit ranks (pvs_hit_value_ranks; the reference's hotspot.py with use_rank): rows [n_hits, n_rec] fp32 on the
    device holds every receptor atom's value in every hit, NaN = none. lig_val [>= lig_ptr[n_hits]] fp32 and lig_ptr
    [n_hits + 1] int32, both or neither: the packed ligand values of the hits, candidates too. The candidates of a hit
    are its ligand values, then its row values, NaN left out; u stands before v iff u > v, or u == v and u comes
    earlier (-0.0 == +0.0); a candidate's rank is the number of candidates of its hit that stand before it - the
    position in a descending stable sort, 0 = best. Returns (row_rank [n_hits, n_rec] - NaN where rows is -, lig_rank
    (parallel to lig_val, entries from lig_ptr[n_hits] on not written; None without lig_val), rank_sum, rank_count,
    rank_max): the last three are `acc` (fresh ones without: new_contact_accumulators), UPDATED with row_rank as
    `contact_attention` updates its own. A hit whose ligand range descends, is negative or has more than 1024 atoms
    gets a row of NaN, no ligand write and adds nothing. `out`: (row_rank, lig_rank) to write into. Two launches, no
    atomics, no workspace, no allocation with out and acc: the same bits every time."""
    who = 'hit_value_ranks'
    rows = _c(rows, _F32, _FP32_ONLY)
    if rows.dim() != 2:
        raise ValueError(f'{who}: rows [n_hits, n_rec]')
    n_hits, n_rec = rows.shape
    if n_rec + HIT_RANK_MAX_LIGAND >= 1 << 24:
        raise ValueError(f'{who}: {n_rec} receptor atoms: a rank is stored as a float and must be exact '
                         f'(n_rec + {HIT_RANK_MAX_LIGAND} < 2^24)')
    if (lig_val is None) != (lig_ptr is None):
        raise ValueError(f'{who}: lig_val and lig_ptr are given together or not at all')
    with_lig = lig_val is not None
    if with_lig:
        lig_val = _c(lig_val, _F32, _FP32_ONLY)
        if (lig_val.dim() != 1 or lig_ptr.dtype != torch.int32 or lig_ptr.shape != (n_hits + 1,)
                or not lig_ptr.is_contiguous()):
            raise ValueError(f'{who}: lig_val [>= lig_ptr[n_hits]] and a contiguous int32 lig_ptr [{n_hits + 1}]')
    _lib.require_hip(rows, lig_val, lig_ptr)
    dev = rows.device
    if out is None:
        # (the ligand ranks start as NaN: what a hit that is none leaves behind)
        out = (torch.empty_like(rows), torch.full_like(lig_val, float('nan')) if with_lig else None)
    if len(out) != 2:
        raise ValueError(f'{who}: out = (row_rank, lig_rank)')
    row_rank, lig_rank = out
    _lib.require_hip(row_rank, lig_rank)
    if (row_rank.dtype != torch.float32 or row_rank.shape != rows.shape or not row_rank.is_contiguous()
            or (lig_rank is None) == with_lig
            or (with_lig and (lig_rank.dtype != torch.float32 or lig_rank.shape != lig_val.shape
                              or not lig_rank.is_contiguous()))
            or row_rank.data_ptr() == rows.data_ptr() and rows.numel()
            or (with_lig and lig_rank.data_ptr() == lig_val.data_ptr() and lig_val.numel())):
        raise ValueError(f'{who}: out = (row_rank [{n_hits}, {n_rec}], lig_rank like lig_val - None without it), '
                         'contiguous fp32, not the inputs themselves')
    acc = _checked_accumulators(who, new_contact_accumulators(n_rec, dev) if acc is None else acc, n_rec)
    _lib.check(_lib.lib().pvs_hit_value_ranks(
        _lib.ptr(rows), n_hits, n_rec, _lib.ptr(lig_val), _lib.ptr(lig_ptr), _lib.ptr(row_rank), _lib.ptr(lig_rank),
        *(_lib.ptr(t) for t in acc), _stream(dev)), 'pvs_hit_value_ranks')
    return (row_rank, lig_rank) + tuple(acc)


class _BceLogitsMeanFn(torch.autograd.Function):
    """nn.BCEWithLogitsLoss() (mean) as one launch forward (loss + the gradient factor), one backward."""

    @staticmethod
    def forward(ctx, x, target):
        shape = x.shape
        x, target = _c(x, _F32, _FP32_ONLY).reshape(-1), _c(target, _F32, _FP32_ONLY).reshape(-1)
        _lib.require_hip(x, target)
        n = x.numel()
        loss = torch.empty((), dtype=torch.float32, device=x.device)
        grad = torch.empty_like(x)
        _lib.check(_lib.lib().pvs_bce_logits_fwd(_lib.ptr(x), _lib.ptr(target), n, _lib.ptr(loss), _lib.ptr(grad),
                                                 _stream(x.device)), 'pvs_bce_logits_fwd')
        ctx.save_for_backward(grad)
        ctx.shape = shape
        return loss

    @staticmethod
    def backward(ctx, g_loss):
        grad, = ctx.saved_tensors
        if g_loss.data_ptr() == _unit_gradient_ptr(g_loss.device):
            # `loss.backward(gradient=unit_gradient(device))` (the harness's backprop): the upstream gradient is the
            # constant 1, so the factor saved by the forward IS the gradient - no scaling launch (and autograd did not
            # have to fill a ones tensor either)
            return grad.reshape(ctx.shape), None
        g_loss = _c(g_loss, _F32, _FP32_ONLY)
        out = torch.empty_like(grad)
        _lib.check(_lib.lib().pvs_scale_by_device_scalar(_lib.ptr(grad), _lib.ptr(g_loss), grad.numel(), _lib.ptr(out),
                                                         _stream(grad.device)), 'pvs_scale_by_device_scalar')
        return out.reshape(ctx.shape), None


_UNIT_GRADIENTS = {}


def unit_gradient(device):
    """A scalar 1.0 on `device`, made once: `loss.backward(gradient=unit_gradient(loss.device))` is `loss.backward()`
    without the ones_like fill autograd launches for the root gradient, and lets the fused loss skip its own scaling
    launch (two launches of ~4 us per training step). Never written to."""
    device = torch.device(device)
    if device.type == 'cuda' and device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    unit = _UNIT_GRADIENTS.get(device)
    if unit is None:
        unit = _UNIT_GRADIENTS[device] = torch.ones((), dtype=torch.float32, device=device)
    return unit


def _unit_gradient_ptr(device):
    unit = _UNIT_GRADIENTS.get(device)
    return -1 if unit is None else unit.data_ptr()


def bce_with_logits_mean(y_pred, y_true):
    if y_pred.shape != y_true.shape:
        raise ValueError(f'Target size ({tuple(y_true.shape)}) must be the same as input size ({tuple(y_pred.shape)})')
    if y_pred.numel() == 0:
        raise ValueError('bce_with_logits_mean: empty input')
    return _BceLogitsMeanFn.apply(y_pred, y_true)


# The status words of pvs_segment_reduce_fwd, read WITHOUT blocking the stream (as graph.PreparedGraph.poll_status reads
# the graph preparation's): a call queues its word (nowait.LateQueue); every later segment_reduce call raises for
# whichever earlier words have landed, and the call's own backward waits for its own word (it has long landed by then).
# The reference's scatter_add_ raises at once (egnn_satorras.py:336); here the error surfaces one call late - or in the
# backward - but it does surface.
_SEGMENT_STATUS = LateQueue()


def _raise_for_segment_status(taken):
    """taken: what the queue handed out, (status word, tag) or None."""
    if taken is not None and taken[0] & 1:
        raise IndexError('unsorted_segment_sum / unsorted_segment_mean: segment_ids contains values outside '
                         '[0, num_segments)')


class _SegmentReduceFn(torch.autograd.Function):
    """unsorted_segment_sum / unsorted_segment_mean (egnn_satorras.py:332-347)."""

    @staticmethod
    def forward(ctx, data, segment_ids, num_segments, mean):
        kind = _kind_of('segment_reduce', data)
        data = data.contiguous()
        _lib.require_hip(data, segment_ids)
        ids = segment_ids.long().contiguous()
        e, c = data.shape
        dev = data.device
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            for taken in _SEGMENT_STATUS.landed():      # an earlier call's out-of-range ids raise here
                _raise_for_segment_status(taken)
        out = torch.empty((num_segments, c), dtype=kind.dtype, device=dev)
        ptr = torch.empty(num_segments + 1, dtype=torch.int32, device=dev)
        status = torch.empty(1, dtype=torch.int32, device=dev)
        ws_bytes = kind.segment_ws(e, num_segments)
        ws = _ws(ws_bytes, dev)
        kind.check(kind.segment_fwd(
            _lib.ptr(data), _lib.ptr(ids), e, c, num_segments, 1 if mean else 0, _lib.ptr(out),
            _lib.ptr(ptr), _lib.ptr(status), _lib.ptr(ws), ws_bytes, _stream(dev)), 'segment_fwd')
        ctx.status = None if capturing else _SEGMENT_STATUS.put(status)      # (no host-visible validation under capture)
        ctx.save_for_backward(ids, ptr)
        ctx.mean, ctx.shape, ctx.n_segments, ctx.kind = mean, (e, c), num_segments, kind
        return out

    @staticmethod
    def backward(ctx, g_out):
        ids, ptr = ctx.saved_tensors
        if ctx.status is not None and not torch.cuda.is_current_stream_capturing():
            _raise_for_segment_status(_SEGMENT_STATUS.take(ctx.status))
        e, c = ctx.shape
        kind = ctx.kind
        g_out = _c(g_out, kind.dtype)
        g_data = torch.empty((e, c), dtype=kind.dtype, device=g_out.device)
        kind.check(kind.segment_bwd(
            _lib.ptr(g_out), _lib.ptr(ids), _lib.ptr(ptr), e, c, ctx.n_segments, 1 if ctx.mean else 0,
            _lib.ptr(g_data), _stream(g_out.device)), 'segment_bwd')
        return g_data, None, None, None


def segment_reduce(data, segment_ids, num_segments, mean=False):
    return _SegmentReduceFn.apply(data, segment_ids, int(num_segments), bool(mean))


def segment_status_check():
    """Wait for every pending status word of segment_reduce and raise for the first bad one (call where a sync is fine)."""
    while len(_SEGMENT_STATUS):
        _raise_for_segment_status(_SEGMENT_STATUS.take())


def dropout_adj(edge_index, edge_attr=None, p=0.5, force_undirected=True, training=True, seed=0, step=0):
    """torch_geometric's dropout_adj as the reference calls it (egnn_satorras.py:320-323: force_undirected=True):
    of every pair only the row <= col copy is drawn, survivors first, their reverses behind, attributes
    repeated. Identity when not training or p == 0. The draw is the library's own counter-based stream
    (pvs_dropout_adj_mark: Philox keyed on (seed, step)), reproducible but not torch's. One host read (the
    number of survivors sizes the outputs), like every data-dependent filter."""
    if not training or not p:
        return edge_index, edge_attr
    if not force_undirected:
        raise NotImplementedError('the reference only calls dropout_adj with force_undirected=True')
    _lib.require_hip(edge_index, edge_attr)
    lib = _lib.lib()
    edge_index = edge_index.long().contiguous()
    n_edges = int(edge_index.shape[1])
    if n_edges == 0:          # nothing to draw from (an empty tensor has no device pointer to hand over)
        return edge_index, edge_attr
    dev = edge_index.device
    n_attr = 0
    if edge_attr is not None:
        edge_attr = edge_attr.long().contiguous()
        n_attr = int(edge_attr.shape[1])
    stream = _lib.stream(dev)
    pos = torch.empty(n_edges + 1, dtype=torch.int32, device=dev)
    ws_bytes = lib.pvs_dropout_adj_workspace_bytes(n_edges)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.pvs_dropout_adj_mark(_lib.ptr(edge_index), n_edges, float(p), int(seed) & (2 ** 64 - 1),
                                        int(step), _lib.ptr(pos), _lib.ptr(ws), ws_bytes, stream),
               'pvs_dropout_adj_mark')
    kept = int(pos[-1])
    out_index = torch.empty((2, 2 * kept), dtype=torch.int64, device=dev)
    out_attr = None if edge_attr is None else torch.empty((2 * kept, n_attr), dtype=torch.int64, device=dev)
    if kept == 0:             # nothing survived: the empty outputs have no device pointer, which the fill refuses
        return out_index, out_attr
    _lib.check(lib.pvs_dropout_adj_fill(_lib.ptr(edge_index), _lib.ptr(edge_attr), n_attr, n_edges, _lib.ptr(pos),
                                        kept, _lib.ptr(out_index), _lib.ptr(out_attr), stream),
               'pvs_dropout_adj_fill')
    return out_index, out_attr


def static_dropout_plan(n_nodes, n_half, p):
    """(cap, n_pad) of the fixed-shape dropped edge list of a batch with `n_nodes` nodes whose list has `n_half` edges
    with row <= col (the candidates of the draw; a self-loop survives twice, as in dropout_adj). Pure host arithmetic.
    cap = 2 * n_half holds every draw. n_pad = 2 * max(1, ceil(p * n_nodes / 2)) padding nodes: a draw leaves about
    p * cap slots empty, which are spread over n_pad rows, so a padding row then has about the batch's mean degree
    (cap / n_nodes) and balances like any other row - all dead slots on ONE pair of rows would serialise a launch on
    one wave."""
    n_nodes, n_half, p = int(n_nodes), int(n_half), float(p)
    if n_nodes < 0 or n_half < 0 or not 0.0 <= p < 1.0:
        raise ValueError(f'static_dropout_plan({n_nodes}, {n_half}, {p}): counts >= 0 and p in [0, 1)')
    return 2 * n_half, 2 * max(1, math.ceil(p * n_nodes / 2))


def dropout_key_table(device, seed=0, step=0):
    """Device table {seed, step} (two 64-bit words, held as int64 bits) that dropout_adj_padded draws from."""
    table = torch.zeros(2, dtype=torch.int64, device=device)
    write_dropout_key(table, seed, step)
    return table


def write_dropout_key(key_table, seed, step):
    """key_table <- (seed, step) on the current stream, by a launch with by-value arguments: NOT inside a capture (a
    replay would write the captured key back)."""
    _lib.require_hip(key_table)
    if key_table.dtype != torch.int64 or key_table.numel() != 2:
        raise ValueError('the dropout key table is an int64 tensor of two words')
    _lib.check(_lib.lib().pvs_dropout_key_write(_lib.ptr(key_table), int(seed) & (2 ** 64 - 1),
                                                int(step) & (2 ** 64 - 1), _lib.stream(key_table.device)),
               'pvs_dropout_key_write')


def dropout_adj_padded(edge_index, edge_attr, p, key_table, cap, n_nodes, n_pad, out=None):
    """dropout_adj(force_undirected=True, training=True) with a fixed output shape, for a captured training step: no
    host read, and the key (seed, step) comes from `key_table` (dropout_key_table / write_dropout_key) when the
    kernels RUN. Returns (out_index [2, cap], out_attr [cap, A] or None, n_kept: device int32 scalar K). The first 2K
    columns are dropout_adj's list for the table's key; every slot behind them is an edge between two of the `n_pad`
    padding nodes n_nodes .. n_nodes + n_pad - 1, both directions in turn, attribute row one-hot class 0
    (pvs_dropout_adj_fill_padded). cap: even, at least twice the number of row <= col edges (static_dropout_plan; 2 E
    always suffices) - a smaller one leaves the outputs unwritten, and n_kept tells. out = (out_index, out_attr):
    buffers of those shapes to write into."""
    _lib.require_hip(edge_index, edge_attr, key_table)
    if not 0.0 <= float(p) < 1.0:
        raise ValueError(f'dropout probability {p} not in [0, 1)')
    cap, n_nodes, n_pad = int(cap), int(n_nodes), int(n_pad)
    if cap < 0 or cap % 2 or n_pad < 2 or n_pad % 2:
        raise ValueError(f'cap={cap} must be even and >= 0, n_pad={n_pad} even and >= 2')
    if key_table.dtype != torch.int64 or key_table.numel() != 2:
        raise ValueError('the dropout key table is an int64 tensor of two words')
    lib = _lib.lib()
    edge_index = edge_index.long().contiguous()
    n_edges = int(edge_index.shape[1])
    dev = edge_index.device
    n_attr = 0
    if edge_attr is not None:
        edge_attr = edge_attr.long().contiguous()
        n_attr = int(edge_attr.shape[1])
    if out is None:
        out_index = torch.empty((2, cap), dtype=torch.int64, device=dev)
        out_attr = None if edge_attr is None else torch.empty((cap, n_attr), dtype=torch.int64, device=dev)
    else:
        out_index, out_attr = out
        if (out_index.dtype != torch.int64 or tuple(out_index.shape) != (2, cap) or (out_attr is None) != (edge_attr is None)
                or (out_attr is not None and (out_attr.dtype != torch.int64 or tuple(out_attr.shape) != (cap, n_attr)))):
            raise ValueError(f'out must be int64 buffers of shape (2, {cap}) and ({cap}, {n_attr})')
        _lib.require_hip(out_index, out_attr)
    stream = _lib.stream(dev)
    pos = torch.empty(n_edges + 1, dtype=torch.int32, device=dev)
    ws_bytes = lib.pvs_dropout_adj_workspace_bytes(n_edges)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.pvs_dropout_adj_mark_dev(_lib.ptr(edge_index) if n_edges else None, n_edges, float(p),
                                            _lib.ptr(key_table), _lib.ptr(pos), _lib.ptr(ws), ws_bytes, stream),
               'pvs_dropout_adj_mark_dev')
    _lib.check(lib.pvs_dropout_adj_fill_padded(
        _lib.ptr(edge_index) if n_edges else None, _lib.ptr(edge_attr) if n_edges else None, n_attr, n_edges,
        _lib.ptr(pos), cap, n_nodes, n_pad, _lib.ptr(out_index) if cap else None,
        _lib.ptr(out_attr) if cap and out_attr is not None else None, stream), 'pvs_dropout_adj_fill_padded')
    return out_index, out_attr, pos[n_edges]
