"""Virtual-screening forward (BASELINE config 5): many rigid poses of one
ligand against one receptor. Reference loop: `val` / inference.py
(/root/reference/point_vs/models/point_neural_network_base.py:208-360, point_vs/inference.py:35-146).

What is reused across poses: the receptor-receptor messages of the FIRST EGNN layer depend only on
receptor features and coordinates, so their per-node sums are computed once
(`pvs_egnn_layer_edge_sums` on the receptor-only graph); per batch the first layer only runs over
the edges that touch a ligand atom (`pvs_egnn_layer_fwd_partial`), the other layers over the full
graph. Graphs are built on the GPU from the coordinates (radius_graph.py). Scores equal the plain
`model(batch)` forward up to fp32 summation order. A first layer with edge attention under softmax_attention has no
sums that add; with `softmax_reuse=True` its receptor side is kept as softmax statistics instead, which merge exactly
(`pvs_egnn_layer_edge_stats_softmax`, `pvs_egnn_layer_fwd_partial_softmax`).
"""
import contextlib
import ctypes as C
from collections import namedtuple

import torch
from torch import nn

from . import _lib
from . import functional as PF
from .library_steps import (STEPS, _PlainStep, _csr_buffers, _graph_pair, _ligand_csr, library_route,       # noqa: F401
                            model_route)
from .nowait import LateQueue, StagingRing, capture_fixed_step, pinned
from .radius_graph import PoseBatcher, radius_graph


# The most ligand atoms a pose-batch slot holds (the builders keep a ligand atom's ligand-ligand contacts in
# ceil(n / 64) mask words); the same number as parquet_data.MAX_LIGAND_ATOMS, the data-root path's limit.
MAX_SCREEN_LIGAND_ATOMS = 1024


def _stream(dev):
    return _lib.stream(dev)


# The first-layer reuse of one kind of layer: the entry that makes a receptor's base, the entry that runs the layer on top
# of it (the one that takes att_out, or NULL), the mode of pvs_egnn_layer_workspace_bytes and what a base row holds
# behind its H channels. Sums that add (sigmoid attention or none; _att with NULL is pvs_egnn_layer_fwd_partial bit for
# bit) | softmax statistics
_ReuseKind = namedtuple('_ReuseKind', 'base_entry partial_entry ws_mode row_extra')
_SUMS = _ReuseKind('pvs_egnn_layer_edge_sums', 'pvs_egnn_layer_fwd_partial_att', 2, 0)
_SOFTMAX = _ReuseKind('pvs_egnn_layer_edge_stats_softmax', 'pvs_egnn_layer_fwd_partial_softmax', 3, 4)


TASKS = ('pose', 'affinity', 'both')


def _resolve_tasks(model, tasks):
    """Which heads a screen of `model` evaluates. A model with one head (`feats_linear_layers`) takes only None and
    gives None: the screen's single-head path. A two-headed model (`feats_linear_layers_pose` / `_affinity`) gives
    'pose', 'affinity' or 'both' (pose first): `tasks` itself, or for None the head its current task selects
    ('classification' in model_task: pose, as its forward decides). Pure host logic; ValueError for anything else."""
    two_headed = hasattr(model, 'feats_linear_layers_pose') and hasattr(model, 'feats_linear_layers_affinity')
    if not two_headed:
        if tasks is not None:
            raise ValueError(f'tasks={tasks!r}: {type(model).__name__} has one head; tasks selects the heads of a '
                             'two-headed model (leave it None)')
        return None
    if tasks is None:
        return 'pose' if 'classification' in model.model_task else 'affinity'
    if tasks not in TASKS:
        raise ValueError(f"tasks={tasks!r}: one of 'pose', 'affinity', 'both' or None")
    return tasks


def resolve_attention_layer(model, layer):
    """The index into model.layers (>= 1: layer 0 is the embedding) that `layer` names, the reference's attribution
    `--layer` (negative: from the end); None stays None. ValueError, listing the layers that qualify, for an index
    outside the model or a layer without edge attention. Pure host logic."""
    if layer is None:
        return None
    layers = list(model.layers)
    have = [k for k, l in enumerate(layers) if getattr(l, 'edge_attention', False)]
    at = int(layer) + len(layers) if int(layer) < 0 else int(layer)
    if at not in have:
        raise ValueError(f'contact attention of layer {layer}: model.layers[{layer}] has no edge attention (the layers '
                         f'that have it: {have}, of {len(layers)})')
    return at


def resolve_cam(model, heads, tasks, cam):
    """What `cam=` of a LibraryScreen selects: None for None, else (the head modules evaluated per node, their output
    widths, first column, columns averaged). The heads are the ones the screen evaluates (`heads` of a two-headed
    model, else model.feats_linear_layers). True follows the reference's rule (attribution_fns.cam): one output column
    is the value, three are averaged, anything else - the two heads of tasks='both' included - is a ValueError that
    asks for a column; an int selects that column of the raw outputs."""
    if cam is None:
        return None
    heads = list(heads) if heads is not None else [model.feats_linear_layers]
    if any(head is None for head in heads):
        raise ValueError('cam: the model has no head (feats_linear_layers is None): there is nothing to apply per node')
    widths = []
    for head in heads:
        linears = [m for m in head if isinstance(m, nn.Linear)]
        if not linears:
            raise ValueError('cam: a head without a Linear has no known output width')
        widths.append(int(linears[-1].out_features))
    total = sum(widths)
    if cam is True:
        if tasks == 'both' or total not in (1, 3):
            raise ValueError(f"cam=True: the reference's rule covers one output column (itself) or three (their mean); "
                             f"the heads evaluated here (tasks={tasks!r}) give {total} - name a column: cam=<int> / "
                             'column=<int>')
        return heads, widths, 0, total
    if isinstance(cam, bool) or not isinstance(cam, int):
        raise ValueError(f'cam={cam!r}: None, True or a column of the raw outputs')
    if not 0 <= cam < total:
        raise ValueError(f'cam: column {cam} of {total} outputs')
    return heads, widths, int(cam), 1


class _ReceptorSideScreen:
    """What ReceptorScreen and LibraryScreen do alike, once: the receptor-receptor sums of the first layer and their
    weights fingerprint, the ligand-touching first layer, the layers after it, the deferred status word and the
    capture / replay scaffolding. A subclass provides `_cache_receptor_sums()` (where the sums are kept),
    `_raise_for(code)` (its status bits), `_head(h)` (pooling + head of a single-head model), `_pool_ptr()` (the
    batch's node offsets, for the heads of a two-headed model) and, once its builder has run, `_fast` (the live buffer
    dict with `status`)."""

    def __init__(self, model, edge_radius, intra_radius, tasks=None, softmax_reuse=False):
        if any(p.dtype == torch.float64 for p in model.parameters()):
            raise NotImplementedError(f'{type(self).__name__} and its pose-batch builder are fp32 only (no fp64 '
                                      'screening kernels): score fp64 models through the model forward')
        layers = list(model.layers)
        self.model, self.embed, self.egnn = model, layers[0], layers[1:]
        self.r_inter = edge_radius
        self.r_intra = edge_radius if intra_radius is None else intra_radius
        # opt-in: a first layer with edge attention under softmax_attention takes the first-layer reuse as well, its
        # receptor side kept as softmax statistics (base rows of H + 4 floats) instead of sums
        self.softmax_reuse = bool(softmax_reuse)
        first = self.egnn[0] if self.egnn else None
        self._soft = bool(self.softmax_reuse and first is not None and first.softmax_attention and first.edge_attention)
        self._kind = _SOFTMAX if self._soft else _SUMS      # decided here, read by the base and the partial first layer
        # None: a single-head model, the path below as it always was; else the heads of a two-headed model, resolved
        # here (a captured step has them baked in) and never by changing model.model_task
        self.tasks = _resolve_tasks(model, tasks)
        self.heads = None if self.tasks is None else model.task_heads(self.tasks)
        self._graph, self._captured, self._l1_ws, self._fast = None, False, None, None
        self._fingerprint = None            # of the weights behind what is cached of the receptor; None: nothing is
        self._late = LateQueue(ring=1)      # the one status word in flight: checked before the next builder launch
        self.cam, self._h_final = None, None      # (LibraryScreen(cam=...): per-node heads of the final embedding)

    def _first_layer_reusable(self):
        """The first layer's part in `reuse`: hidden size 32 or 64, and no softmax attention - unless the screen was
        built with softmax_reuse and the layer has edge attention (a softmax flag without edge attention stays out)."""
        first = self.egnn[0] if self.egnn else None
        return (first is not None and first.hidden_nf in (32, 64)
                and (not first.softmax_attention or self._soft))

    def _weights_fingerprint(self):
        """Version counters of everything the cached receptor-receptor sums were computed from (the
        embedding and the first layer): an optimiser step or load_weights() bumps them."""
        mods = [self.embed.m, self.egnn[0]]
        return tuple((p.data_ptr(), p._version) for m in mods for p in m.parameters())

    def stale(self):
        """True when the weights the cached receptor-receptor sums came from have changed since
        (load_weights(), an optimiser step): a captured step has those sums baked in."""
        return self._fingerprint is not None and self._fingerprint != self._weights_fingerprint()

    def _weights_changed(self):
        return RuntimeError(f'{type(self).__name__}: the model\'s weights changed after capture(); build a new screen')

    def _refresh_if_stale(self):
        """The weights changed under the screen (load_weights(), a training step): the cached sums are recomputed
        once - never inside a captured graph, which bakes them in."""
        if self._fingerprint != self._weights_fingerprint():
            if torch.cuda.is_current_stream_capturing() or self._graph is not None:
                raise self._weights_changed()
            self._cache_receptor_sums()

    def _first_layer_args(self):
        first = self.egnn[0]
        desc = _lib.PvsLayerDesc(*first._desc())
        params = [None if p is None else p.detach().float().contiguous() for p in first._params()]
        return desc, params, _lib.PvsLayerParams(*[_lib.ptr(p) for p in params])

    def _receptor_sums(self, rec_feats, rec_pos):
        """Per-node sums of the first layer's receptor-receptor messages (pose and ligand independent):
        (magg [n_rec,H], xsum [n_rec,3], deg [n_rec]); under softmax_reuse magg is the layer's base rows [n_rec,H+4]
        (weighted mean | maximum logit | denominator | 0 | 0: pvs_egnn_layer_edge_stats_softmax). Keeps the
        receptor-receptor template CSR (`_rr`: rowptr /
        col, receptor-local ids) and the fingerprint of the weights used."""
        lib = _lib.lib()
        dev, n_rec = rec_pos.device, rec_pos.shape[0]
        self._fingerprint = self._weights_fingerprint()
        with torch.no_grad():
            h_rec = self.embed.embed(rec_feats, rec_pos)
            pg = radius_graph(rec_pos, torch.ones(n_rec, dtype=torch.uint8, device=dev), None,
                              self.r_inter, self.r_intra, need_backward=False)
            desc, params, pstruct = self._first_layer_args()
            name = self._kind.base_entry
            magg = torch.empty((n_rec, self.egnn[0].hidden_nf + self._kind.row_extra), dtype=torch.float32, device=dev)
            xsum = torch.empty((n_rec, 3), dtype=torch.float32, device=dev)
            ws_bytes = lib.pvs_egnn_layer_workspace_bytes(C.byref(desc), n_rec, pg.n_edges, self._kind.ws_mode)
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            _lib.check(getattr(lib, name)(
                C.byref(desc), C.byref(pg.c), C.byref(pstruct), _lib.ptr(h_rec.contiguous()),
                _lib.ptr(rec_pos.contiguous()), _lib.ptr(magg), _lib.ptr(xsum), _lib.ptr(ws), ws_bytes,
                _stream(dev)), name)
            deg = (pg.t['rowptr'][1:] - pg.t['rowptr'][:-1]).float()
            self._rr = pg
            torch.cuda.current_stream(dev).synchronize()    # ws / params go out of scope
        return magg, xsum, deg

    def _partial_first_layer(self, g, h, x, base_magg, base_xsum, base_deg, ws_nodes, ws_edges, att_out=None):
        """First layer over the ligand-touching edges `g` on top of the receptor-receptor sums `base_*` (one row
        per node). ws_nodes / ws_edges size the saved / workspace pair, allocated at the first call. att_out
        [>= g's edge room]: receives the layer's edge attention in g's edge order; None: the entry gets NULL and keeps it
        in its workspace (pvs_egnn_layer_fwd_partial_att, then pvs_egnn_layer_fwd_partial bit for bit).
        Under softmax_reuse base_magg holds base rows and the entry is pvs_egnn_layer_fwd_partial_softmax, whose
        attention is normalised over all edges of a row."""
        lib = _lib.lib()
        dev = h.device
        desc, params, pstruct = self._first_layer_args()
        if getattr(self, '_gn_slots', False) and self.egnn[0].graphnorm:
            desc.flags |= _lib.GRAPHNORM_SEGMENTS      # (g carries the slots' node_ptr: library_steps._ReuseStep._graphs)
        h_out, x_out = torch.empty_like(h), torch.empty_like(x)
        natt = torch.empty(h.shape[0], dtype=torch.float32, device=dev) if self.egnn[0].node_attention else None
        if self._l1_ws is None:
            self._l1_ws = (
                torch.empty(lib.pvs_egnn_layer_saved_floats(C.byref(desc), ws_nodes, ws_edges), dtype=torch.float32,
                            device=dev),
                torch.empty(lib.pvs_egnn_layer_workspace_bytes(C.byref(desc), ws_nodes, ws_edges, self._kind.ws_mode),
                            dtype=torch.uint8, device=dev))
        saved, ws = self._l1_ws
        name = self._kind.partial_entry
        _lib.check(getattr(lib, name)(
            C.byref(desc), C.byref(g), C.byref(pstruct), _lib.ptr(h), _lib.ptr(x), _lib.ptr(base_magg),
            _lib.ptr(base_xsum), _lib.ptr(base_deg), _lib.ptr(h_out), _lib.ptr(x_out), _lib.ptr(natt), _lib.ptr(att_out),
            _lib.ptr(saved), _lib.ptr(ws), ws.numel(), _stream(dev)), name)
        return h_out, x_out

    def _receptor_template(self, rec_pos):
        """The receptor-receptor template CSR alone (`_rr`), for a step that keeps no first-layer sums (a cropped
        LibraryScreen); the weights fingerprint is taken as `_receptor_sums` takes it, so stale() and a captured step's
        refusal after a weight change work alike."""
        self._fingerprint = self._weights_fingerprint()
        dev, n_rec = rec_pos.device, rec_pos.shape[0]
        with torch.no_grad():
            self._rr = radius_graph(rec_pos, torch.ones(n_rec, dtype=torch.uint8, device=dev), None, self.r_inter,
                                    self.r_intra, need_backward=False)

    def _tail(self, pg_full, h, x, layers=None):
        """The layers after the first (or `layers`) over the full graph, then the head."""
        m_sorted = None
        for layer in self.egnn[1:] if layers is None else layers:
            h, x, m_sorted = layer.forward_prepared(pg_full, h, x, m_sorted, need_m=layer.edge_residual,
                                                    need_coords=layer is not self.egnn[-1])
        if self.cam is not None:
            self._h_final = h
        if self.tasks is not None:
            return self._heads_out(h, self._pool_ptr())
        return h if self.model.feats_linear_layers is None else self._head(h)

    def _heads_out(self, feats, graph_ptr):
        """[batch_size, sum of the heads' outputs] of a two-headed model: one pooling, every selected head
        (PF.pool_heads: one launch)."""
        return self.model._pool_and_heads(self.heads, feats, graph_ptr, self.b)

    def _plain(self, batch):
        """The model's plain forward on `batch`, for the routes the first-layer reuse does not cover: the model's own
        forward (single head), or its trunk and then the same head code as the reuse route. With `cam` the trunk's
        final embedding and the batch's node offsets are kept (`_h_final`, `_plain_ptr`)."""
        if self.tasks is None and self.cam is None:
            return self.model(batch)
        feats, _, graph_ptr, n_graphs = self.model._embed_graph(batch)
        if self.cam is not None:
            self._h_final, self._plain_ptr = feats, graph_ptr
        if self.tasks is None:      # (the model's own forward, said out)
            head = self.model.feats_linear_layers
            return feats if head is None else self.model._pool_and_head(head, feats, graph_ptr, n_graphs)
        return self._heads_out(feats, graph_ptr)

    def _queue_status(self, status):
        """Queues the copy of a builder's status word into the screen's pinned word; check() reads it later."""
        self._late.put(status)

    def check(self):
        """Raises if the edge buffers of an earlier batch were too small (checked one batch late so that the loop
        never waits for the device; call once more after the last batch)."""
        taken = self._late.take()
        if taken is not None:
            self._raise_for(taken[0])

    def _capture(self, step, dev):
        """Captures step() (builder + layer stack + head) in a hipGraph on `dev` after two eager warm-up calls (probe,
        buffers, lazy allocations)."""
        self._graph, self._static_out = capture_fixed_step(step, dev, self.check)
        self._captured = True
        return self

    def _replay(self, load):
        if self.stale():           # host-only comparison of version counters
            raise self._weights_changed()
        self.check()
        load()
        self._graph.replay()
        self._queue_status(self._fast['status'])
        return self._static_out


class ReceptorScreen(_ReceptorSideScreen):
    """scores = ReceptorScreen(model, rec_pos, feats, n_lig, batch_size, edge_radius)(lig_poses)

    feats [n_lig + n_rec, F]: ligand rows first, last column = bp (preprocessing.make_bit_vector);
    lig_poses [batch_size, n_lig, 3] on the device. Returns the model's raw outputs [batch_size, ...].
    tasks (two-headed models, `_resolve_tasks`): 'pose', 'affinity' or 'both' - [batch_size, 1 + A], pose logit first,
    from one trunk pass.
    softmax_reuse (opt-in, default False): a first layer with edge attention under softmax_attention takes the first-layer
    reuse too (its receptor side as softmax statistics, merged per row with the ligand-touching edges'); without it such a
    model runs the plain forward. The keyword changes nothing for any other model."""

    def __init__(self, model, rec_pos, feats, n_lig, batch_size, edge_radius, intra_radius=None, tasks=None,
                 softmax_reuse=False):
        super().__init__(model, edge_radius, intra_radius, tasks, softmax_reuse)
        self.reuse = self._first_layer_reusable() and not self.egnn[0].edge_residual
        dev = rec_pos.device
        self.batcher = PoseBatcher(rec_pos, feats, n_lig, batch_size, edge_radius, intra_radius)
        self.n_lig, self.b = n_lig, batch_size
        self._lig_buf = None
        self._graph_ptr = self.batcher.batch.ptr.to(device=dev, dtype=torch.int32)
        # the specialised pose-batch builder (pvs_screen_graph_build) leaves the edge counts on the
        # device; layers that return edge messages (edge_residual) need them on the host
        self.fast_graph = (self.reuse and n_lig <= MAX_SCREEN_LIGAND_ATOMS
                           and not any(l.edge_residual for l in self.egnn))
        self._rec_pos, self._feats = rec_pos, feats
        if self.reuse:
            self._cache_receptor_sums()

    def _cache_receptor_sums(self):
        """The receptor sums tiled into the batch layout: [ligand rows (no base) | receptor rows] per pose."""
        dev, n_lig = self._rec_pos.device, self.n_lig
        magg, xsum, deg = self._receptor_sums(self._feats[n_lig:].to(dev).float(), self._rec_pos)
        n = n_lig + self._rec_pos.shape[0]
        self.base_magg = torch.zeros((self.b, n, magg.shape[1]), dtype=torch.float32, device=dev)
        self.base_xsum = torch.zeros((self.b, n, 3), dtype=torch.float32, device=dev)
        self.base_deg = torch.zeros((self.b, n), dtype=torch.float32, device=dev)
        self.base_magg[:, n_lig:] = magg
        self.base_xsum[:, n_lig:] = xsum
        self.base_deg[:, n_lig:] = deg
        # the tiling copies are done before magg / xsum / deg are released and before a capture opens its side
        # stream; without this wait a sweep over 57 size buckets read corrupted status words
        # (profiles/screening_refactor.txt, 7)
        torch.cuda.current_stream(dev).synchronize()

    def _probe_cap_l(self, batch):
        """One synchronous probe of the loaded batch sizes the ligand-edge buffers; later batches are checked
        asynchronously."""
        probe = radius_graph(batch.pos, batch.x[:, -1], batch.ptr, self.r_inter, self.r_intra,
                             max_graph_nodes=self.batcher.n, need_backward=False, ligand_pairs_only=True)
        return min(4 * self.n_lig * self.batcher.n * self.b, 2 * probe.n_edges + 4096)

    def _ligand_graph(self, batch):
        """CSR of the full graph's ligand-touching edges, filtered on the device (no host round trip);
        the edge count stays on the device (PvsGraph.n_edges_dev)."""
        lib = _lib.lib()
        full = batch.prepared
        dev = batch.pos.device
        n = full.n_nodes
        if self._lig_buf is None:
            b = _csr_buffers(dev, n, self._probe_cap_l(batch))
            b['ws'] = torch.empty(lib.pvs_graph_filter_workspace_bytes(n), dtype=torch.uint8, device=dev)
            b['bp'] = batch.x[:, -1].to(torch.uint8).contiguous()
            b['gl'] = _ligand_csr(b, n, n)
            self._lig_buf = b
        b = self._lig_buf
        self.check()      # the previous batch's overflow flag has landed by now
        _lib.check(lib.pvs_graph_filter_ligand_edges(
            C.byref(full.c), _lib.ptr(b['bp']), b['cap_l'], _lib.ptr(b['rowptr_l']), _lib.ptr(b['row_l']),
            _lib.ptr(b['col_l']), _lib.ptr(b['etype_l']), _lib.ptr(b['status']), _lib.ptr(b['ws']), b['ws'].numel(),
            _stream(dev)), 'pvs_graph_filter_ligand_edges')
        self._queue_status(b['status'])
        return b['gl']

    def _raise_for(self, code):
        if code & 4:
            raise RuntimeError('ReceptorScreen: ligand-edge buffer overflow (more ligand contacts than '
                               'twice the first batch); rebuild the screen with a larger probe')

    def _build_fast(self, lig_poses):
        """Full graph + ligand-touching subgraph of the pose batch from the receptor template
        (pvs_screen_graph_build): no receptor-receptor distance tests, no host round trip."""
        lib = _lib.lib()
        dev = lig_poses.device
        n, b_, n_rec = self.batcher.n, self.b, self.batcher.n - self.n_lig
        if self._fast is None:
            cap_l = self._probe_cap_l(self.batcher.load(lig_poses))
            f = _csr_buffers(dev, n * b_, cap_l, b_ * self._rr.n_edges + cap_l,
                             state=torch.empty(lib.pvs_screen_graph_state_bytes(b_, self.n_lig, n_rec),
                                               dtype=torch.uint8, device=dev))
            f['pg'], f['gl'] = _graph_pair(f, n * b_, n * b_)
            self._fast = f
        f = self._fast
        capturing = torch.cuda.is_current_stream_capturing()
        if not capturing:
            self.check()
        self.batcher._pos[:, :self.n_lig] = lig_poses
        _lib.check(lib.pvs_screen_graph_build(
            _lib.ptr(lig_poses.contiguous()), _lib.ptr(self.batcher._pos[0, self.n_lig:].contiguous()),
            _lib.ptr(self._rr.t['rowptr']), _lib.ptr(self._rr.t['col']), b_, self.n_lig, n_rec,
            float(self.r_inter), float(self.r_intra), f['cap'], f['cap_l'],
            _lib.ptr(f['rowptr']), _lib.ptr(f['row']), _lib.ptr(f['col']), _lib.ptr(f['etype']),
            _lib.ptr(f['inv_deg']), _lib.ptr(f['rowptr_l']), _lib.ptr(f['row_l']), _lib.ptr(f['col_l']),
            _lib.ptr(f['etype_l']), _lib.ptr(f['status']), _lib.ptr(f['state']), f['state'].numel(),
            _stream(dev)), 'pvs_screen_graph_build')
        if not capturing:
            self._queue_status(f['status'])
        return f['pg'], f['gl']

    def capture(self, example_poses):
        """Captures one whole screening step (graph build + layer stack + head) in a hipGraph; after
        this, `replay(lig_poses)` copies the poses into the captured input buffer and launches the
        graph (BASELINE config 5: "hipGraph-captured layer stack"). Needs the device-side edge counts
        (self.fast_graph)."""
        if not self.fast_graph:
            raise RuntimeError(f'capture needs the pose-batch builder (<= {MAX_SCREEN_LIGAND_ATOMS} ligand atoms, '
                               'no edge_residual)')
        self._static_in = example_poses.clone()
        return self._capture(lambda: self(self._static_in), example_poses.device)

    def replay(self, lig_poses):
        return self._replay(lambda: self._static_in.copy_(lig_poses))

    def _head(self, h):
        return self.model._pool_and_head(self.model.feats_linear_layers, h, self._graph_ptr, self.b)

    def _pool_ptr(self):
        return self._graph_ptr

    @torch.no_grad()
    def __call__(self, lig_poses):
        if not self.reuse:
            return self._plain(self.batcher.load(lig_poses))
        self._refresh_if_stale()
        if self.fast_graph:
            pg_full, g_lig = self._build_fast(lig_poses)
            batch = self.batcher.batch
        else:
            batch = self.batcher.load(lig_poses)
            pg_full, g_lig = batch.prepared, None
        h = self.embed.embed(batch.x.float(), batch.pos).contiguous()
        x = batch.pos.contiguous()
        if g_lig is None:
            g_lig = self._ligand_graph(batch)
        h, x = self._partial_first_layer(g_lig, h, x, self.base_magg, self.base_xsum, self.base_deg,
                                         h.shape[0], g_lig.n_edges)
        return self._tail(pg_full, h, x)


def plan_library(pose_counts, lig_sizes, batch_size, max_lig_atoms=64):
    """Batches of a library sweep: a list of batches, each a list of up to `batch_size` pairs (ligand index, pose
    index), in library order then pose order, slots filled densely (only the last batch may have empty slots).
    Pure host logic. Raises ValueError for a ligand that has poses and no atoms or more than `max_lig_atoms`."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f'batch_size must be positive (got {batch_size})')
    if len(pose_counts) != len(lig_sizes):
        raise ValueError('pose_counts and lig_sizes differ in length')
    batches, cur = [], []
    for lig, (count, size) in enumerate(zip(pose_counts, lig_sizes)):
        if int(count) > 0 and not 1 <= int(size) <= max_lig_atoms:
            raise ValueError(f'ligand {lig} has {int(size)} atoms: a library batch slot holds 1..{max_lig_atoms}')
        for pose in range(int(count)):
            cur.append((lig, pose))
            if len(cur) == batch_size:
                batches.append(cur)
                cur = []
    if cur:
        batches.append(cur)
    return batches


def leave_out_plan(sizes, batch_size):
    """Slot sizes of the batches that hold every leave-one-atom-out copy of ligands of `sizes` atoms: ligand s owns
    sizes[s] + 1 consecutive copies (the whole ligand: sizes[s] atoms; then one copy per atom left out: sizes[s] - 1),
    sum(sizes) + len(sizes) copies in all, `batch_size` per batch in that order. A list of batches, each a list of
    `batch_size` atom counts; the slots after the last copy are empty (0). What pvs_leave_out_ligand_pack lays out on
    the device, as pure host arithmetic."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f'batch_size must be positive (got {batch_size})')
    sizes = [int(n) for n in sizes]
    if any(n < 0 for n in sizes):
        raise ValueError(f'ligand sizes must not be negative (got {sizes})')
    copies = [m for n in sizes for m in [n] + [n - 1] * n]
    copies += [0] * ((-len(copies)) % batch_size)
    return [copies[k:k + batch_size] for k in range(0, len(copies), batch_size)]


def leave_out_pair_plan(pair_counts, sizes, batch_size, ligand_atom=True, receptor_atom=True):
    """The batches that hold every copy of hits of `sizes` atoms that leaves out one row of the hit's pair table
    (`pair_counts[s]` rows): hit s owns pair_counts[s] + 1 consecutive copies (the whole ligand: sizes[s] atoms, the
    whole receptor; then one copy per row: sizes[s] - 1 atoms when the rows name a ligand atom, `ligand_atom`, and a
    receptor without one atom when they name a receptor atom, `receptor_atom`), sum(pair_counts) + len(sizes) copies in
    all, `batch_size` per batch in that order. A list of batches, each (a list of `batch_size` atom counts, the number
    of its slots that lack a receptor atom); the slots after the last copy are empty (0). What
    pvs_leave_out_pair_pack lays out on the device, as pure host arithmetic."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError(f'batch_size must be positive (got {batch_size})')
    sizes, pair_counts = [int(n) for n in sizes], [int(k) for k in pair_counts]
    if len(sizes) != len(pair_counts):
        raise ValueError('pair_counts and sizes differ in length')
    if any(n < 0 for n in sizes) or any(k < 0 for k in pair_counts):
        raise ValueError(f'sizes and pair counts must not be negative (got {sizes}, {pair_counts})')
    if ligand_atom and any(k > 0 and n == 0 for k, n in zip(pair_counts, sizes)):
        raise ValueError('a hit without atoms has no ligand atom to leave out')
    less = 1 if ligand_atom else 0
    copies = [c for n, k in zip(sizes, pair_counts) for c in [(n, 0)] + [(n - less, 1 if receptor_atom else 0)] * k]
    copies += [(0, 0)] * ((-len(copies)) % batch_size)
    return [([n for n, _ in copies[k:k + batch_size]], sum(d for _, d in copies[k:k + batch_size]))
            for k in range(0, len(copies), batch_size)]


def slot_offsets(batch_sizes, batch_size):
    """The slot offsets of batches of a LibraryScreen: batch_sizes, a list of per-batch lists of up to `batch_size`
    atom counts, as an int32 table [len(batch_sizes), batch_size + 1] on the host - row b: the exclusive prefix sums
    of batch b's sizes, the slots after its last one empty (they repeat the last offset). What load_packed takes as
    lig_ptr, one row per batch. Pure host arithmetic."""
    ptrs = torch.zeros((len(batch_sizes), int(batch_size) + 1), dtype=torch.int32)
    for b, sizes in enumerate(batch_sizes):
        ptrs[b, 1:len(sizes) + 1] = torch.tensor(sizes, dtype=torch.int32)
    return ptrs.cumsum(1, dtype=torch.int32)


class LibraryScreen(_ReceptorSideScreen):
    """Library screening: every one of the `batch_size` slots of a batch holds one pose of ANY ligand of up to
    `max_lig_atoms` (<= MAX_SCREEN_LIGAND_ATOMS = 1024) atoms against the one receptor, or nothing (the last batch of
    a library).

        screen = LibraryScreen(model, rec_pos, rec_feats, batch_size, max_lig_atoms, edge_radius)
        scores = screen([(lig_feats [n,F], pose [n,3]), ...])        # [batch_size, ...] raw outputs

    A screen runs ONE of three steps, chosen once at construction (`library_steps.library_route`, kept in `self.route`;
    each step's docstring in library_steps.py says what it builds and launches): `reuse`, the first-layer reuse, for
    hidden size 32 / 64 without edge_residual and without softmax attention; `plain`, the model's own forward on the
    same mixed batch, for every other model; `cropped` under crop_radius. The two builder steps run at the padded shape
    N_cap = batch_size * (max_lig_atoms + n_rec) (padding nodes have no edges and belong to no graph), and no host
    argument of theirs depends on the batch's composition, so ONE captured step (`capture`) serves every batch;
    `self.reuse` says whether the screen has such a step. fp32 only. tasks: as for ReceptorScreen (every route).

    padded_graphnorm (opt-in, default False; modifies reuse, required by cropped): GraphNorm normalises over the batch's
    nodes, so such a model runs the reuse step eager at the exact node count; with the keyword it runs at N_cap like
    every other model, eager and captured, with the statistics over the node_ptr[batch_size] real rows in front of the
    padding, a count the layers read on the device (PvsGraph.n_norm_rows_dev). The copies of one batch still normalise
    each other, as in every batched route, unless `slot_graphnorm=True`. Changes nothing for a model without graphnorm,
    nor for the plain route.

    slot_graphnorm (opt-in, default False; implies padded_graphnorm, giving both is fine): every slot of a GraphNorm
    model's batch is normalised by its own rows - the reference's semantics for one complex per forward - so a pose's
    score no longer depends on what shares its batch and equals the batch_size=1 score, at the padded shape in the one
    captured step: both graphs of the reuse step and the cropped step's graph carry the slots' node_ptr as a segment
    table (PreparedGraph.set_norm_segments, `_lib.GRAPHNORM_SEGMENTS`) instead of the real-row count. An empty slot is
    a segment of length 0, a struck or cropped slot a shorter one. Covers what padded_graphnorm covers. A GraphNorm
    model on the plain route raises NotImplementedError (fp64 models are refused as always); on a cropped screen it
    stands in for padded_graphnorm=True. Changes nothing for a model without graphnorm: same launches, same bits.

    softmax_reuse (opt-in, default False; selects reuse): as for ReceptorScreen - a first layer with edge attention
    under softmax_attention takes the reuse, and with it capture(), struck slots and contact_attention.

    cam (every route): None, True or a column (`resolve_cam`): the class-activation map of every step - the heads the
    screen evaluates, applied to every node's final embedding (PF.node_heads) and gathered per slot
    (PF.slot_node_values), inside the captured step - in the static buffers `screen.cam`: node_y [N_cap, C] (the heads'
    raw outputs per node), lig_val [batch_size * max_lig_atoms] (packed atom order of the loaded batch) and slot_rec_val
    [batch_size, n_rec] (NaN for an empty slot) of the LAST step, and rec_sum / rec_count / rec_max [n_rec], accumulated
    over every step since reset_cam(). Needs no attention layer; the plain route runs it eagerly.

    contact_attention (modifies reuse; cropped under cropped_maps; NotImplementedError on plain): None, or a layer index
    into model.layers as the reference's attribution `--layer` (1: the first EGNN layer; negative: from the end) whose
    edge attention every step reduces on the device (PF.contact_attention, inside the captured step) into the static
    buffers `screen.contact`: lig_att [batch_size * max_lig_atoms] (packed atom order of the loaded batch) and
    slot_rec_att [batch_size, n_rec] - the largest attention over each atom's ligand-receptor edges, NaN without one -
    of the LAST step, and rec_sum / rec_count / rec_max [n_rec], accumulated since reset_contact_attention().

    struck (modifies reuse; ValueError on plain and cropped): None, or True for a screen whose slots may lack one
    receptor atom each (receptor-atom and contact masking: the reference's atom_masking / bond_masking remove atoms
    together with their edges). The screen then owns a static `rec_drop [batch_size]` int32 (-1: the whole receptor; r:
    the slot's receptor is without atom r, so the slot has n_rec - 1 receptor rows), which `load(slots, rec_drop=[...])`
    and `load_leave_out_pairs` fill. Goes with neither `cam` nor `contact_attention` (their reductions assume n_rec
    receptor rows per slot). A screen without it launches exactly what it always launched.

    crop_radius (selects cropped): None, or the radius of the training loader's crop (the reference's make_box(...,
    relative_to_ligand=True), the data-root path's `radius`; CLI default 10): every slot keeps only the receptor atoms
    closer than it to one of the slot's ligand atoms, so a pose scores what `val()` gives the same pose, and the layers
    run over the rows the model was trained on. capture() / replay() and `tasks` work as above; `screen.keep` holds the
    last step's masks, `screen._fast['node_ptr']` its offsets. Models as captured_scoring.model_refusal accepts them
    (fp32, no edge_residual, 17..128 channels: NotImplementedError otherwise); GraphNorm models need
    padded_graphnorm=True (the row count is only known on the device); struck, cam and contact_attention do not go with
    it (their reductions assume n_rec rows per slot): ValueError - cam and contact_attention unless `cropped_maps` is on.
    None: the screen launches exactly what it launches without the keyword.

    cropped_maps (opt-in, default False; modifies cropped, ValueError without crop_radius): `cam` and
    `contact_attention` on a cropped screen - the maps of the complexes the scores are of, into the same static buffers,
    inside the captured step. contact_attention takes any layer that has edge attention, 1 included. The models are
    those of a cropped screen, not those of the first-layer reuse. struck stays refused. False, or True without a map:
    the screen launches exactly what it launches without the keyword.

    crop_parents (opt-in, default False; modifies cropped, ValueError without crop_radius): the slots may be leave-out
    COPIES of hits on the hits' cropped complexes - the reference's atom_masking / bond_masking get the loader's
    complex, cropped around the WHOLE ligand, and strike atoms out of that one, so a copy must not be cropped again
    around what is left of it. The screen then owns three more static tables - `crop_pos [batch_size * max_lig_atoms,
    3]` / `crop_ptr [batch_size + 1]`: the atoms every slot is cropped AROUND, and `rec_drop [batch_size]`: -1 or the
    receptor atom the slot lacks whatever the crop says. A plain load (`screen(slots)`, `load_packed`) crops every slot
    around its own atoms - the ligand table is copied into the crop table on the device, rec_drop is -1 - and gives the
    bits of a screen without the keyword. `load_leave_out` and `load_leave_out_pairs` work on such a screen: the
    existing packer launch plus one PF.leave_out_parent_pack launch that lays the copies' parents into the crop table,
    both outside the captured step; the pair packer writes this screen's rec_drop. False: the screen launches exactly
    what it launches without the keyword."""

    def __init__(self, model, rec_pos, rec_feats, batch_size, max_lig_atoms, edge_radius, intra_radius=None,
                 tasks=None, contact_attention=None, cam=None, struck=None, padded_graphnorm=False,
                 softmax_reuse=False, crop_radius=None, crop_parents=False, cropped_maps=False, slot_graphnorm=False):
        super().__init__(model, edge_radius, intra_radius, tasks, softmax_reuse)
        self.slot_graphnorm = bool(slot_graphnorm)
        self.struck = bool(struck)
        self.crop_parents = bool(crop_parents)
        self.cropped_maps = bool(cropped_maps)
        if self.cropped_maps and crop_radius is None:
            raise ValueError('LibraryScreen(cropped_maps=True) needs crop_radius: without it cam and contact_attention '
                             'reduce the whole receptor as they are')
        if self.crop_parents and crop_radius is None:
            raise ValueError('LibraryScreen(crop_parents=True) needs crop_radius: the parents\' atoms are what a cropped '
                             'slot is cropped around')
        self.padded_graphnorm = bool(padded_graphnorm)
        self.crop_radius = None if crop_radius is None else float(crop_radius)
        if self.crop_radius is not None:
            self._check_crop(model, contact_attention, cam)
        if self.struck and (cam is not None or contact_attention is not None):
            which = 'cam' if cam is not None else 'contact_attention'
            raise ValueError(f'LibraryScreen(struck=True, {which}=...): the {which} reduction assumes n_rec receptor '
                             'rows in every slot, and a struck slot has one less; use two screens')
        self.cam_request = cam
        self._cam_plan = resolve_cam(model, self.heads, self.tasks, cam)
        if not 1 <= int(max_lig_atoms) <= MAX_SCREEN_LIGAND_ATOMS:
            raise ValueError(f'max_lig_atoms must be 1..{MAX_SCREEN_LIGAND_ATOMS} (got {max_lig_atoms})')
        _lib.require_hip(rec_pos)
        self.graphnorm = any(getattr(l, 'graphnorm', False) for l in self.egnn)
        if self.crop_radius is not None and self.graphnorm and not (self.padded_graphnorm or self.slot_graphnorm):
            raise ValueError('LibraryScreen(crop_radius=...): a GraphNorm model needs padded_graphnorm=True - the row '
                             'count of a cropped batch is only known on the device, where the layers then read it - or '
                             'slot_graphnorm=True')
        dev = rec_pos.device
        self.b, self.max_lig_atoms = int(batch_size), int(max_lig_atoms)
        self.slot_cap = max(self.max_lig_atoms, 64)      # what the builder validates lig_ptr against
        self.n_rec = int(rec_pos.shape[0])
        self._contact_request = contact_attention
        self.contact_attention = resolve_attention_layer(model, contact_attention)       # (index into model.layers)
        # the route is chosen here, once; its step says what it refuses (plain: struck slots, contact_attention)
        self.route = model_route(model, self.softmax_reuse, self.crop_radius)
        self._step = STEPS[self.route](self)
        self.reuse = self._step.has_builder         # the screen runs its own fixed-shape step, not the plain forward
        # a graphnorm model at the padded shape: the statistics over the node_ptr[batch_size] real rows, read on the device
        self._gn_padded = (self.padded_graphnorm or self.slot_graphnorm) and self.graphnorm and self._step.has_builder
        # ... and every slot by its own rows: the slots' node_ptr as the layers' segment table
        self._gn_slots = self.slot_graphnorm and self.graphnorm
        if self._gn_slots and not self._step.has_builder:
            raise NotImplementedError(
                'LibraryScreen(slot_graphnorm=True): per-slot GraphNorm runs in the fixed-shape steps (the first-layer '
                'reuse or a cropped screen), which this model does not have - ' + self._step.capture_refusal() +
                '; score it at batch_size=1, or mask it one complex at a time with pointvs_amd.attribution')
        self.l_cap = self.b * self.max_lig_atoms
        self.n_cap = self.l_cap + self.b * self.n_rec
        self._rec_pos = rec_pos.float().contiguous()
        self._rec_feats = rec_feats.to(dev).float().contiguous()
        n_feats = int(self._rec_feats.shape[1])
        self.lig_pos = torch.zeros((self.l_cap, 3), dtype=torch.float32, device=dev)
        self.lig_feats = torch.zeros((self.l_cap, n_feats), dtype=torch.float32, device=dev)
        self.lig_ptr = torch.zeros(self.b + 1, dtype=torch.int32, device=dev)
        self.n_atoms = 0             # host copies of what load() was given
        self._sizes = [0] * self.b
        # two pinned staging sets for load() - the previous batch's copies may still be in flight - pinned at its first
        # call: a sweep that only calls load_packed needs none
        self._stage = StagingRing(2, lambda: dict(
            pos=pinned((self.l_cap, 3), torch.float32), feats=pinned((self.l_cap, n_feats), torch.float32),
            ptr=pinned(self.b + 1, torch.int32)))
        self._pack_status = None     # load_leave_out's status word
        self.rec_drop = (torch.full((self.b,), -1, dtype=torch.int32, device=dev)
                         if self.struck or self.crop_parents else None)
        if self.crop_parents:        # what every slot is cropped around (a plain load: its own atoms)
            self.crop_pos = torch.zeros((self.l_cap, 3), dtype=torch.float32, device=dev)
            self.crop_ptr = torch.zeros(self.b + 1, dtype=torch.int32, device=dev)
        self._n_struck = 0           # host copy: how many slots of the loaded batch lack a receptor atom
        self.contact = None
        if self.contact_attention is not None:
            self.contact = self._value_buffers('lig_att', 'slot_rec_att')
        if self._cam_plan is not None:
            self.cam = self._value_buffers('lig_val', 'slot_rec_val', node_width=sum(self._cam_plan[1]))
        self._cache_receptor_sums()

    def _check_crop(self, model, contact_attention, cam):
        """What a cropped screen refuses, before anything is allocated."""
        from .captured_scoring import model_refusal
        if not self.crop_radius > 0:
            raise ValueError(f'crop_radius must be positive (got {self.crop_radius})')
        for which, given in (('struck', self.struck), ('cam', cam is not None),
                             ('contact_attention', contact_attention is not None)):
            if given and not (self.cropped_maps and which != 'struck'):      # (cropped_maps: the masked reductions)
                raise ValueError(f'LibraryScreen(crop_radius=..., {which}=...): the {which} path assumes n_rec receptor '
                                 'rows in every slot, and a cropped slot has those inside the radius; use two screens')
        why = model_refusal(model)
        if why is not None:
            raise NotImplementedError(f'LibraryScreen(crop_radius=...): {why}')

    @property
    def keep(self):
        """The keep masks of the last step of a cropped screen, [batch_size, ceil(n_rec / 64)] int64 on the device."""
        return self._step.keep()

    def _value_buffers(self, lig_key, slot_key, node_width=None):
        """The static buffers of `contact` / `cam`: the three accumulators, with node_width node_y [N_cap, node_width],
        and the last step's values per packed ligand atom (`lig_key`) and per slot and receptor atom (`slot_key`)."""
        f32 = dict(dtype=torch.float32, device=self.lig_pos.device)
        rec_sum, rec_count, rec_max = PF.new_contact_accumulators(self.n_rec, f32['device'])
        values = {} if node_width is None else dict(node_y=torch.zeros((self.n_cap, node_width), **f32))
        values.update({lig_key: torch.full((self.l_cap,), float('nan'), **f32),
                       slot_key: torch.full((self.b, self.n_rec), float('nan'), **f32)},
                      rec_sum=rec_sum, rec_count=rec_count, rec_max=rec_max)
        return values

    def _reset_values(self, values, who, feature):
        if values is None:
            raise RuntimeError(f'{who}: the screen was built without {feature}')
        values['rec_sum'].zero_()
        values['rec_count'].zero_()
        values['rec_max'].fill_(float('nan'))

    def reset_cam(self):
        """The accumulators of `cam` as before the first step: sums and counts zero, maxima NaN (none so far)."""
        self._reset_values(self.cam, 'reset_cam', 'cam')

    def reset_contact_attention(self):
        """The accumulators of `contact` as before the first step: sums and counts zero, maxima NaN (none so far)."""
        self._reset_values(self.contact, 'reset_contact_attention', 'contact_attention')

    def _cache_receptor_sums(self):
        """What the step keeps of the receptor, once: the first-layer sums and the template (reuse), the template alone
        (cropped), nothing (plain)."""
        self._step.cache_receptor()

    # ---- inputs ----
    def _checked_sizes(self, sizes):
        """The slots' atom counts as a list of ints, or a ValueError for more slots or atoms than the screen holds."""
        sizes = [int(n) for n in sizes]
        if len(sizes) > self.b or any(not 0 <= n <= self.max_lig_atoms for n in sizes):
            raise ValueError(f'a batch holds up to {self.b} slots of 0..{self.max_lig_atoms} atoms (got {sizes})')
        return sizes

    def _loaded(self, sizes, n_struck):
        """The host's copies of what was loaded: the slots' atom counts, their sum, the slots that lack a receptor
        atom."""
        self._sizes = sizes + [0] * (self.b - len(sizes))
        self.n_atoms = sum(sizes)
        self._n_struck = int(n_struck)

    def _packer_status(self):
        """The status word of the leave-out packers, allocated at the first leave-out batch."""
        if self._pack_status is None:      # (crop_parents: a second word, the parent packer's)
            self._pack_status = torch.zeros(2 if self.crop_parents else 1, dtype=torch.int32,
                                            device=self.lig_pos.device)
        return self._pack_status

    def _crop_around_own_atoms(self):
        """crop_parents, a plain load: the crop table <- the ligand table, on the device."""
        if self.crop_parents:
            self.crop_pos.copy_(self.lig_pos)
            self.crop_ptr.copy_(self.lig_ptr)

    def _pack_parents(self, lig_pos, lig_ptr, copy_ptr, first_copy):
        """crop_parents, a leave-out load: the crop table <- the whole hits behind the batch's copies
        (PF.leave_out_parent_pack, one launch)."""
        if self.crop_parents:
            PF.leave_out_parent_pack(lig_pos, lig_ptr, copy_ptr, first_copy, self.b, self.max_lig_atoms,
                                     out=(self.crop_pos, self.crop_ptr, self._packer_status()[1:]))

    def _load_rec_drop(self, rec_drop, n_slots):
        """The static rec_drop of a struck screen <- a host list (None: every slot has the whole receptor). Returns
        how many slots lack a receptor atom."""
        if rec_drop is None:
            if self.rec_drop is not None:
                self.rec_drop.fill_(-1)
            return 0
        if self.rec_drop is None:
            raise ValueError('rec_drop: the screen was built without struck=True')
        drops = [int(r) for r in rec_drop]
        if len(drops) > self.b or len(drops) != n_slots or any(not -1 <= r < self.n_rec for r in drops):
            raise ValueError(f'rec_drop: one entry of -1..{self.n_rec - 1} per slot ({n_slots}; got {drops})')
        drops += [-1] * (self.b - len(drops))
        self.rec_drop.copy_(torch.tensor(drops, dtype=torch.int32))
        return sum(r >= 0 for r in drops)

    def load_packed(self, lig_pos, lig_feats, lig_ptr, sizes, rec_drop=None):
        """One batch from packed device (or pinned host) tensors: lig_pos [L,3], lig_feats [L,F] (L = sum of
        sizes), lig_ptr [batch_size+1] int32; `sizes`: the host's copy of the slots' atom counts. Three
        asynchronous copies into the step's static inputs. rec_drop (a struck screen): a host list, one entry per
        slot of `sizes`."""
        sizes = self._checked_sizes(sizes)
        n_struck = self._load_rec_drop(rec_drop, len(sizes))
        total = sum(sizes)
        if lig_pos.shape[0] != total or lig_feats.shape[0] != total or lig_ptr.numel() != self.b + 1:
            raise ValueError('packed ligand tensors do not match the slot sizes')
        self.lig_pos[:total].copy_(lig_pos, non_blocking=True)
        self.lig_feats[:total].copy_(lig_feats, non_blocking=True)
        self.lig_ptr.copy_(lig_ptr, non_blocking=True)
        self._crop_around_own_atoms()
        self._loaded(sizes, n_struck)
        return self

    def load(self, slots, rec_drop=None):
        """slots: up to batch_size pairs (lig_feats [n,F], pose [n,3]), n = 0..max_lig_atoms (host or device
        tensors); the slots after them are empty. Host tensors are packed into pinned staging. rec_drop (a struck
        screen, hand-built batches): a host list with one entry per slot, -1 or the receptor atom the slot lacks."""
        slots = list(slots)
        sizes = self._checked_sizes(pose.shape[0] for _, pose in slots)
        total = sum(sizes)
        st = self._stage.acquire()
        at = 0
        for k in range(self.b):
            st['ptr'][k] = at
            if k < len(slots) and sizes[k]:
                feats, pose = slots[k]
                st['pos'][at:at + sizes[k]].copy_(pose)
                st['feats'][at:at + sizes[k]].copy_(feats)
                at += sizes[k]
        st['ptr'][self.b] = at
        self.load_packed(st['pos'][:total], st['feats'][:total], st['ptr'], sizes, rec_drop)
        self._stage.release(self.lig_pos.device)
        return self

    def load_leave_out(self, lig_pos, lig_feats, lig_ptr, sizes, first_copy):
        """One batch of leave-one-atom-out copies (PF.leave_out_ligand_pack: slot k holds copy first_copy + k of the
        ligands lig_pos [L,3] / lig_feats [L,F] / lig_ptr [S+1] int32, all on the device; first_copy: one int32 on the
        device), packed by one launch straight into the step's static inputs. `sizes`: the host's copy of the slots'
        atom counts (a batch of `leave_out_plan`); nothing is copied back. `check_leave_out()` reads the packer's
        verdict on lig_ptr."""
        sizes = self._checked_sizes(sizes)
        PF.leave_out_ligand_pack(lig_pos, lig_feats, lig_ptr, first_copy, self.b, self.max_lig_atoms,
                                 out=(self.lig_pos, self.lig_feats, self.lig_ptr, self._packer_status()[:1]))
        self._pack_parents(lig_pos, lig_ptr, lig_ptr, first_copy)
        self._loaded(sizes, self._load_rec_drop(None, len(sizes)))
        return self

    def load_leave_out_pairs(self, lig_pos, lig_feats, lig_ptr, pairs, pair_ptr, sizes, n_struck, first_copy):
        """One batch of copies that leave out one ligand-receptor pair each (PF.leave_out_pair_pack: slot k holds copy
        first_copy + k of the hits lig_pos [L,3] / lig_feats [L,F] / lig_ptr [S+1] with the pair table pairs [K,2] /
        pair_ptr [S+1], all on the device), packed by one launch straight into the step's static inputs, rec_drop
        among them. `sizes`, `n_struck`: the host's copy of the slots' atom counts and of how many of them lack a
        receptor atom (a batch of `leave_out_pair_plan`); nothing is copied back. `check_leave_out()` reads the
        packer's verdict on the tables."""
        if not self.struck and not self.crop_parents:
            raise ValueError('load_leave_out_pairs: the screen was built without struck=True (or, cropped, without '
                             'crop_parents=True): it has no rec_drop table')
        sizes = self._checked_sizes(sizes)
        if not 0 <= int(n_struck) <= len(sizes):
            raise ValueError(f'n_struck: 0..{len(sizes)} of the batch\'s slots (got {n_struck})')
        PF.leave_out_pair_pack(lig_pos, lig_feats, lig_ptr, pairs, pair_ptr, self.n_rec, first_copy, self.b,
                               self.max_lig_atoms,
                               out=(self.lig_pos, self.lig_feats, self.lig_ptr, self.rec_drop,
                                    self._packer_status()[:1]))
        self._pack_parents(lig_pos, lig_ptr, pair_ptr, first_copy)
        self._loaded(sizes, n_struck)
        return self

    def check_leave_out(self):
        """Raises if the last load_leave_out() was given a lig_ptr that is no table of 0..max_lig_atoms-atom ligands
        (its batch was empty then). Waits for the device."""
        # (crop_parents: the parent packer's word beside the packer's, one copy back for both)
        if self._pack_status is not None and any(int(code) & 8 for code in self._pack_status.tolist()):
            raise ValueError(f'LibraryScreen.load_leave_out: lig_ptr is not a table of 0..{self.max_lig_atoms}-atom '
                             'ligands inside lig_pos'
                             + (', or the pair table is not one of pairs inside them'
                                if self.struck or self.crop_parents else ''))

    # ---- the graph and the node tables ----
    def _job(self, f, probe=False):
        """The step's PvsScreenSlotsJob of the loaded batch into f (probe: into its probe's buffers, no room for edges)."""
        return self._step.job(f, probe)

    def _launch_builder(self, f, probe=False):
        """The step's builder of the loaded batch into f."""
        self._step.launch(f, probe)

    def _probe_capacities(self):
        """One synchronous probe: the builder with no room for edges leaves both exact edge counts in its row
        pointers. Room for the ligand-touching edges: twice the loaded batch's contacts per ligand atom at a full
        batch of L_cap atoms, at most what L_cap atoms can have (per atom: inter and intra contacts with the receptor,
        both directions, and the slot's other ligand atoms). A struck screen adds the whole rows of the receptor rows
        that the struck atom can touch (`_struck_room`) for every slot. The step says which buffers its probe needs."""
        probe = self._step.probe_buffers()
        self._launch_builder(probe, probe=True)
        n_lig_edges = int(probe['rowptr_l'][self.n_cap].item())
        per_atom = -(-n_lig_edges // max(self.n_atoms, 1))
        cap_l = min(self.l_cap * (4 * self.n_rec + self.slot_cap), 2 * per_atom * self.l_cap + 4096)
        cap = self.b * self._rr.n_edges + cap_l
        if self.struck:
            cap_l += self.b * self._struck_room()
        if cap >= 2 ** 31:
            raise ValueError(f'a batch of {self.b} slots can have {cap} edges (>= 2^31): use a smaller batch_size')
        return cap, cap_l

    def _struck_room(self):
        """The most receptor-receptor entries that one struck atom moves into a slot's ligand-touching CSR: max over r
        of the sum over r's template neighbours j of deg_rr(j) - 1. From the template on the device, one number back
        (at construction of the buffers)."""
        n_edges = int(self._rr.n_edges)
        if n_edges == 0:
            return 0
        rowptr, col = self._rr.t['rowptr'].long(), self._rr.t['col'][:n_edges].long()
        deg = rowptr[1:] - rowptr[:-1]
        rows = torch.repeat_interleave(torch.arange(self.n_rec, device=deg.device), deg)
        moved = torch.zeros(self.n_rec, dtype=torch.int64, device=deg.device).index_add_(0, rows, deg[col] - 1)
        return int(moved.max().item())

    def _build(self, capacities=None):
        """The loaded batch's graph and node tables, into the step's buffers by the step's builder. capacities: (full,
        ligand-touching) edge room instead of the probe's."""
        capturing = torch.cuda.is_current_stream_capturing()
        if self._fast is None:
            cap, cap_l = capacities or self._probe_capacities()
            self._fast = self._step.buffers(cap, cap_l)
        f = self._fast
        if not capturing:
            self.check()
        self._launch_builder(f)
        if not capturing:
            self._queue_status(f['status'])
        return f

    def _raise_for(self, code):
        if code & 8:
            raise ValueError(f'LibraryScreen: lig_ptr is not a table of 0..{self.slot_cap}-atom slots'
                             + (f', or rec_drop has an entry outside -1..{self.n_rec - 1}'
                                if self.struck or self.crop_parents else '')
                             + (', or crop_ptr is no table of crop sets of up to 1024 atoms' if self.crop_parents else ''))
        if code & 4:
            raise RuntimeError('LibraryScreen: edge buffer overflow (more ligand contacts per atom than twice '
                               'the first batch); rebuild the screen with a denser first batch')

    # ---- the step ----
    def _plain_forward(self):
        """The plain route's step on the loaded batch (it needs no buffers, so a screen of any route can run it)."""
        return _PlainStep.run(self._step)

    def _head(self, h):
        return self.model._pool_and_head_padded(self.model.feats_linear_layers, h, self._fast['node_ptr'], self.b)

    def _pool_ptr(self):
        return self._fast['node_ptr']

    @torch.no_grad()
    def __call__(self, slots=None):
        if slots is not None:
            self.load(slots)
        return self._step.run()

    def needs_sizing_batch(self):
        """True while the step's edge buffers are still to be sized, from the first batch the screen is shown (the plain
        route has none)."""
        return self._step.has_builder and self._fast is None

    def capture_refusal(self):
        """Why capture() would refuse (the step's reason), or None."""
        return self._step.capture_refusal()

    def capture(self, example_slots=None):
        """Captures one whole step (builder + layer stack + head) in a hipGraph; `replay(slots)` then serves every
        batch of a library, whatever its composition."""
        why = self.capture_refusal()
        if why is not None:
            raise RuntimeError(why)
        if example_slots is not None:
            self.load(example_slots)
        return self._capture(lambda: self(), self.lig_pos.device)

    def replay(self, slots=None):
        return self._replay(lambda: None if slots is None else self.load(slots))


class _SweepSink:
    """What a sweep does with a batch's raw outputs: the sigmoid (every column of a single-head classification model,
    as `val` does; the pose column alone of a two-headed one), the predictions file(s) - one PredictionsWriter each,
    so the loop never waits for the host - and, for a hits file, the raw rows per ligand."""

    def __init__(self, sweep, predictions_file, sigmoid, keep_raw):
        from .predictions import PredictionsWriter, task_files
        tasks, model = sweep.tasks, sweep.model
        if tasks is None:
            if sigmoid is None:
                sigmoid = getattr(model, 'model_task', 'classification') == 'classification'
            self.sig_cols = None if sigmoid else 0          # (None: all of them)
        else:
            has_pose = tasks != 'affinity'
            self.sig_cols = 1 if has_pose and (sigmoid is None or sigmoid) else 0
        self.sweep, self.receptor = sweep, sweep.receptor_name
        self.raw = {} if keep_raw else None
        self.writers = []          # (writer, first column, columns)
        if predictions_file:
            at = 0
            for task, path in task_files(predictions_file, tasks).items():
                width = model.task_heads('affinity')[0][0].out_features if task == 'affinity' else 1
                if width not in (1, 3):      # (the reference has line formats for one affinity and for three)
                    raise ValueError(f'predictions_file: no line format for an affinity head of {width} outputs '
                                     '(1 or 3); the returned scores hold them all')
                # three affinity columns: format_lines' unlabelled multi_regression form
                form = 'multi_regression' if width == 3 else 'regression'
                self.writers.append((PredictionsWriter(path, form, flush_every=10), at, width))
                at += width

    def scored(self, y):
        """y [n, C] raw -> what the sweep returns and writes."""
        if self.sig_cols == 0:
            return y
        if self.sig_cols is None or y.shape[1] == 1:
            return torch.sigmoid(y)
        return torch.cat([torch.sigmoid(y[:, :1]), y[:, 1:]], 1)

    def write(self, y, ligands):
        for writer, at, cols in self.writers:
            writer.submit(y[:, at] if cols == 1 else y[:, at:at + cols], None, [self.receptor] * len(ligands), ligands)

    def keep_raw(self, name, raw):
        if self.raw is not None:
            self.raw.setdefault(name, []).append(raw)

    def take(self, raw, name, first_pose, keep):
        """One batch of a ligand's poses, done: raw [batch_size, C], of which the first `keep` slots hold the poses
        first_pose .. of ligand `name`. Scores them, keeps their raw rows, writes their predictions lines, counts the
        batch; returns the kept slots' scores."""
        y = self.scored(raw)[:keep]
        self.keep_raw(name, raw[:keep])
        if self.writers:
            self.write(y, [f'{name}_pose{first_pose + i}' for i in range(keep)])
        self.sweep.batches_run += 1
        return y

    def close(self):
        error = None
        for writer, _, _ in self.writers:
            try:
                writer.close()
            except Exception as exc:     # (the other file is still closed)
                error = error or exc
        if error is not None:
            raise error


class ScreeningSweep:
    """Virtual-screening sweep (BASELINE config 5; the reference's `val` / inference.py loop,
    point_neural_network_base.py:208-360, inference.py:77-146): many ligands, each with many rigid
    poses, against ONE receptor, forward only.

    Poses are streamed in fixed-size batches through a `ReceptorScreen` per SIZE BUCKET (= number of
    ligand atoms: a captured hipGraph has fixed shapes, so every distinct ligand size gets its own
    captured step, built on first use and replayed for every later batch of that size; the ligand's
    features are written into the bucket's static input buffers). The last batch of a ligand is
    padded with copies of its last pose; the padding's scores are dropped. Scores leave the device
    through `PredictionsWriter` (pinned buffers + a writer thread, reference line format
    `'{score:.3f} | {receptor} {pose name}'`, :318-325), so the loop never waits for the host.

        sweep = ScreeningSweep(model, rec_pos, rec_feats, edge_radius=10.0, batch_size=32)
        scores = sweep.run([(name, lig_feats [n_lig,F], poses [P,n_lig,3]), ...], 'predictions.txt')

    A two-headed model (MultitaskSatorrasEGNN) is screened on the heads `tasks` names: None (the head its current
    task selects), 'pose', 'affinity', or 'both' - pose logit in column 0, the affinity head's outputs behind it, from
    ONE trunk pass and one pooling (PF.pool_heads); model.model_task is never changed. With 'both' the predictions go
    to `pose_<name>` and `affinity_<name>` beside the path given (`val`'s naming), same line order. `hits_file` (any
    model): after the sweep the best pose of every ligand is picked on the device (PF.segment_argmax on the raw
    column 0: larger wins, ties to the lower pose, NaN never wins) and written one line per ligand; `sweep.hits`
    keeps {name: (best pose or -1, its row)}. `ligand_atom_masking(best_poses(ligands))` then says which ligand atoms
    carry each hit's score: every leave-one-atom-out copy of every hit as a LibraryScreen slot;
    `receptor_hotspots(best_poses(ligands))` says which receptor atoms the hits bind to: one layer's edge attention
    reduced per atom inside the screening step and averaged over the hits on the device - or, with attribution='cam',
    the class-activation map (the heads applied to every atom's final embedding), which needs no attention layer.
    softmax_reuse (opt-in, default False): handed to every screen the sweep creates (LibraryScreen's docstring): models
    with edge attention under softmax_attention then take the captured routes and the attribution methods above.
    crop_radius (opt-in, default None): every pose is scored on the complex cropped around it, as training and `val()`
    see it (LibraryScreen's docstring). `run` and `run_library` then go through cropped LibraryScreens - `run` is
    `run_library`, a ligand above max_lig_atoms gets a cropped screen of its own size (`self.crop_buckets`) - with
    predictions, hits files, tasks and best_poses unchanged in form. The four attribution methods raise
    NotImplementedError on such a sweep unless one of the two keywords below opts them in: the reference masks after
    cropping around the WHOLE ligand, so a copy must not crop again around what is left of it.
    cropped_attribution (opt-in, default False; needs crop_radius >= edge_radius, ValueError otherwise: below the edge
    radius a listed contact's receptor atom may not be kept, at or above it every contact atom is): `ligand_atom_masking`,
    `contact_masking` and `receptor_atom_masking` then work on the cropped sweep as the reference's masking does on the
    loader's complex - every copy of a hit is cropped around the WHOLE hit and lacks what the copy leaves out - through
    ONE LibraryScreen(crop_radius=..., crop_parents=True), `self.cropped_copies`; arguments, return values, `*_raw`,
    score files, `column` and `sigmoid` as on an uncropped sweep. A receptor atom that a hit's crop does not keep is not
    an atom of that hit's complex: atoms='all' means the kept atoms of each hit (PF.crop_keep), and an index tensor is
    intersected with them per hit. Under GraphNorm the copies of one batch normalise each other, as in every batched
    route, unless `slot_graphnorm=True`. `receptor_hotspots` stays refused under this keyword; it runs under `cropped_hotspots` - but for its
    attribution='atom_masking', which IS these masking methods and is opted in here.
    cropped_hotspots (opt-in, default False; needs crop_radius, ValueError otherwise; any crop radius - below the edge
    radius a ligand atom's edges simply reach kept atoms only): `receptor_hotspots` then maps every hit on the complex
    cropped around it, the one its score is of - the hits stream whole through LibraryScreen(crop_radius=...,
    cropped_maps=True, contact_attention=gnn_layer | cam=...), still `self.hotspot` / `self.cam_screen`, in
    ceil(hits / batch_size) steps; arguments, keys and score files as on an uncropped sweep. A receptor atom that a
    hit's crop does not keep is no atom of that hit's complex: NaN in its per_hit row, nothing added to count - under
    'cam' count[j] is the number of hits that keep j. A hit whose crop keeps nothing still has ligand values under
    'cam'; under 'edge_attention' they are NaN.
    """

    def __init__(self, model, rec_pos, rec_feats, edge_radius, batch_size=32, intra_radius=None, capture=True,
                 receptor_name='receptor', tasks=None, padded_graphnorm=False, softmax_reuse=False, crop_radius=None,
                 cropped_attribution=False, cropped_hotspots=False, slot_graphnorm=False):
        self.model, self.rec_pos, self.rec_feats = model, rec_pos, rec_feats
        self.crop_radius = None if crop_radius is None else float(crop_radius)
        self.cropped_attribution = bool(cropped_attribution)
        self.cropped_hotspots = bool(cropped_hotspots)
        if self.cropped_hotspots and self.crop_radius is None:
            raise ValueError('ScreeningSweep(cropped_hotspots=True) needs crop_radius: without it receptor_hotspots maps '
                             'the whole receptor as it is')
        if self.cropped_attribution and self.crop_radius is None:
            raise ValueError('ScreeningSweep(cropped_attribution=True) needs crop_radius: without it the masking methods '
                             'work on the whole receptor as they are')
        if self.cropped_attribution and self.crop_radius < float(edge_radius):
            raise ValueError(f'ScreeningSweep(cropped_attribution=True): crop_radius {self.crop_radius:g} is below the '
                             f'edge radius {float(edge_radius):g} - a contact\'s receptor atom may then not be kept by '
                             'the crop; mask at crop_radius >= edge_radius (training crops at 10 with edge radii of 4 to '
                             '10)')
        self.cropped_copies = None     # the LibraryScreen(crop_parents=True) of the masking methods of a cropped sweep
        self.crop_buckets = {}     # n_lig -> the cropped LibraryScreen of the ligands above run_library's max_lig_atoms
        self.padded_graphnorm = bool(padded_graphnorm)      # handed to every LibraryScreen of the sweep
        self.slot_graphnorm = bool(slot_graphnorm)          # likewise
        # (what the per-ligand ReceptorScreen route cannot give: its batches normalise over all poses)
        self._gn_slots = self.slot_graphnorm and any(getattr(l, 'graphnorm', False) for l in list(model.layers)[1:])
        self.softmax_reuse = bool(softmax_reuse)            # handed to every screen of the sweep
        self.tasks = _resolve_tasks(model, tasks)
        self.hits = {}
        self.atom_masking_raw = {}     # ligand_atom_masking: {name: raw rows [n + 1, C], whole ligand first}
        self.edge_radius, self.intra_radius, self.b = edge_radius, intra_radius, int(batch_size)
        self.capture, self.receptor_name = capture, receptor_name
        self.buckets = {}          # n_lig -> ReceptorScreen (captured when possible)
        self.library = None        # the LibraryScreen of run_library
        self.masking = None        # the LibraryScreen of ligand_atom_masking (its edge room is sized for whole ligands)
        self.hotspot = None        # the LibraryScreen of receptor_hotspots (it reduces one layer's edge attention)
        self.cam_screen = None     # the LibraryScreen of receptor_hotspots(attribution='cam') (per-node heads)
        self.struck = None         # the LibraryScreen(struck=True) of contact_masking and receptor_atom_masking
        self.contact_masking_raw = {}          # contact_masking: {name: raw rows [K + 1, C], whole complex first}
        self.receptor_atom_masking_raw = {}    # receptor_atom_masking: {name: raw rows [M + 1, C]}
        self.batches_run = 0

    def _bucket(self, n_lig, lig_feats, example_poses):
        screen = self.buckets.get(n_lig)
        if screen is not None and screen.stale():
            # the model was trained on or reloaded since this bucket was captured: its cached receptor
            # sums (baked into the captured step) are out of date - build and capture it again
            screen = None
        if screen is None:
            feats = torch.cat([lig_feats.to(self.rec_feats.device), self.rec_feats], 0)
            screen = ReceptorScreen(self.model, self.rec_pos, feats, n_lig, self.b, self.edge_radius, self.intra_radius,
                                    tasks=self.tasks, softmax_reuse=self.softmax_reuse)
            if self.capture and screen.fast_graph:
                screen.capture(example_poses)
            self.buckets[n_lig] = screen
        return screen

    @staticmethod
    def _set_ligand_feats(screen, lig_feats):
        """The bucket's static node-feature buffer: ligand rows of every pose slot <- this ligand."""
        x = screen.batcher.batch.x
        x.view(screen.b, screen.batcher.n, -1)[:, :screen.n_lig] = lig_feats.to(x.device, x.dtype)

    def _run_ligand_cropped(self, name, lig_feats, poses, sink):
        """`_run_ligand` on a cropped sweep: the ligand's poses through a cropped LibraryScreen of its own size, up to
        batch_size slots per step (the last step's other slots are empty); no padding poses."""
        n_poses, n_lig = int(poses.shape[0]), int(poses.shape[1])
        dev = self.rec_pos.device
        screen = self.crop_buckets.get(n_lig)
        if screen is None or screen.stale():
            screen = LibraryScreen(self.model, self.rec_pos, self.rec_feats, self.b, n_lig, self.edge_radius,
                                   self.intra_radius, tasks=self.tasks, padded_graphnorm=self.padded_graphnorm,
                                   softmax_reuse=self.softmax_reuse, crop_radius=self.crop_radius,
                                   slot_graphnorm=self.slot_graphnorm)
            self.crop_buckets[n_lig] = screen
        feats = lig_feats.to(dev).float()
        scores = []
        for k in range(0, n_poses, self.b):
            keep = min(self.b, n_poses - k)
            ptr = slot_offsets([[n_lig] * keep], self.b)[0]
            screen.load_packed(poses[k:k + keep].to(dev).float().reshape(-1, 3), feats.repeat(keep, 1), ptr.to(dev),
                               [n_lig] * keep)
            scores.append(sink.take(self._library_step(screen), name, k, keep))
        screen.check()
        return torch.cat(scores, 0)

    def _run_ligand(self, name, lig_feats, poses, sink):
        """All poses of one ligand through its size bucket; returns its scores [P, ...]."""
        if self.crop_radius is not None:
            return self._run_ligand_cropped(name, lig_feats, poses, sink)
        n_poses, n_lig = int(poses.shape[0]), int(poses.shape[1])
        if self._gn_slots:
            raise ValueError(f'ScreeningSweep(slot_graphnorm=True): ligand {name!r} ({n_lig} atoms) would go through the '
                             'per-ligand ReceptorScreen route, whose poses normalise each other; use run_library with '
                             'max_lig_atoms at least the largest ligand')
        pad = (-n_poses) % self.b
        if pad:
            poses = torch.cat([poses, poses[-1:].expand(pad, -1, -1)], 0)
        screen = self._bucket(n_lig, lig_feats, poses[:self.b].contiguous())
        self._set_ligand_feats(screen, lig_feats)
        scores = []
        for k in range(0, poses.shape[0], self.b):
            chunk = poses[k:k + self.b]
            y = screen.replay(chunk).clone() if screen._captured else screen(chunk.contiguous())
            scores.append(sink.take(y.reshape(self.b, -1), name, k, min(self.b, n_poses - k)))
        screen.check()
        return torch.cat(scores, 0)

    @contextlib.contextmanager
    def _sweeping(self, predictions_file, sigmoid, hits_file):
        """What a sweep runs inside: yields its _SweepSink - sigmoid defaults to what `val` does for the model's task
        (two-headed: on whenever there is a pose column), the predictions writers are closed at the end - with the
        long-lived heap frozen (no full-heap collection pause inside the sweep: see its docstring)."""
        from .point_neural_network_base import long_lived_heap_frozen
        sink = _SweepSink(self, predictions_file, sigmoid, hits_file is not None)
        try:
            with long_lived_heap_frozen():
                yield sink
        finally:
            sink.close()

    def _pick_hits(self, names, sink, hits_file):
        """The best pose of every ligand of `names` (library order; a ligand without poses is an empty segment): one
        PF.segment_argmax over the raw scores on column 0 - before the sigmoid, which saturates into ties - one
        device-to-host copy, `self.hits` and the hits file (predictions.format_hit_lines)."""
        if hits_file is None:
            return
        from pathlib import Path
        from .predictions import format_hit_lines
        raw = {name: torch.cat(parts, 0) for name, parts in sink.raw.items()}
        lines, self.hits = [], {name: (-1, None) for name in names}
        if raw:
            counts = [int(raw[name].shape[0]) if name in raw else 0 for name in names]
            scores = torch.cat([raw[name] for name in names if name in raw], 0)
            seg_ptr = torch.tensor([0] + counts).cumsum(0).to(device=scores.device, dtype=torch.int32)
            best, rows = PF.segment_argmax(scores, seg_ptr, 0)
            # (best beside its row: ONE copy to the host; a pose index is exact in fp32 below 2^24)
            packed = torch.cat([best.to(rows.dtype).unsqueeze(1), sink.scored(rows)], 1).cpu()
            best, rows = packed[:, 0].long().tolist(), packed[:, 1:]
            self.hits = {name: (best[i], rows[i]) for i, name in enumerate(names)}
            lines = format_hit_lines(best, rows.numpy(), self.receptor_name, names)
        path = Path(hits_file).expanduser()
        path.parent.mkdir(parents=True, exist_ok=True)
        path.write_text(''.join(line + '\n' for line in lines))

    @torch.no_grad()
    def run(self, ligands, predictions_file=None, sigmoid=None, hits_file=None):
        """ligands: iterable of (name, lig_feats [n_lig,F], poses [P,n_lig,3] on the device).
        Returns {name: scores [P, C] on the device} (raw model outputs; sigmoid-ed like `val` does for
        classification models when sigmoid is None/True - the pose column alone of a two-headed model).
        predictions_file, hits_file: optional paths (class docstring)."""
        if self.crop_radius is not None:      # (cropped slots are library slots: one path for both)
            return self.run_library(ligands, predictions_file, sigmoid, hits_file=hits_file)
        if self._gn_slots:
            raise ValueError('ScreeningSweep(slot_graphnorm=True).run: the per-ligand ReceptorScreen route normalises a '
                             'GraphNorm model over all poses of a batch; use run_library (LibraryScreen slots are '
                             'normalised one by one)')
        out, names = {}, []
        with self._sweeping(predictions_file, sigmoid, hits_file) as sink:
            for name, lig_feats, poses in ligands:
                names.append(name)
                if int(poses.shape[0]) == 0:
                    continue
                out[name] = self._run_ligand(name, lig_feats, poses, sink)
            self._pick_hits(names, sink, hits_file)
        return out

    def _library_screen(self, max_atoms, which='library', contact_attention=None, cam=None, struck=None,
                        crop_parents=False):
        """The sweep's LibraryScreen `which`, built anew when there is none, when the weights changed under it, when it
        is too narrow for `max_atoms`, when it reduces another layer's attention than `contact_attention` or maps
        another value than `cam`."""
        screen = getattr(self, which)
        layer = resolve_attention_layer(self.model, contact_attention)
        if (screen is None or screen.stale() or screen.max_lig_atoms < max_atoms
                or screen.contact_attention != layer
                or (type(screen.cam_request), screen.cam_request) != (type(cam), cam)):      # (True is not column 1)
            screen = LibraryScreen(self.model, self.rec_pos, self.rec_feats, self.b, max_atoms, self.edge_radius,
                                   self.intra_radius, tasks=self.tasks, contact_attention=layer, cam=cam, struck=struck,
                                   padded_graphnorm=self.padded_graphnorm, softmax_reuse=self.softmax_reuse,
                                   slot_graphnorm=self.slot_graphnorm,
                                   crop_radius=self.crop_radius, crop_parents=crop_parents,
                                   cropped_maps=self.cropped_hotspots and (layer is not None or cam is not None))
            setattr(self, which, screen)
        return screen

    def _capture_if_wanted(self, screen):
        """Captures the step of `screen` on the batch loaded into it, where a captured step can be had."""
        if self.capture and not screen._captured and screen.capture_refusal() is None:
            screen.capture()

    def _library_step(self, screen):
        """The raw outputs [batch_size, C] of the batch loaded into `screen`: the captured step where one can be had
        (captured at the first batch), the eager one otherwise."""
        self._capture_if_wanted(screen)
        return (screen.replay().clone() if screen._captured else screen()).reshape(self.b, -1)

    @torch.no_grad()
    def run_library(self, ligands, predictions_file=None, sigmoid=None, max_lig_atoms=64, hits_file=None):
        """`run` for a docking library (many ligands of different sizes with a few poses each): the poses of all
        ligands of up to `max_lig_atoms` (1..MAX_SCREEN_LIGAND_ATOMS) atoms are streamed through ONE LibraryScreen in dense mixed batches (`plan_library`:
        library order, then pose order; ceil(total poses / batch_size) batches, one captured step for all of them),
        larger ligands through their size bucket as in `run`. Same arguments, return value and predictions lines
        as `run`; the lines are in library order, then pose order."""
        max_lig_atoms = int(max_lig_atoms)
        if not 1 <= max_lig_atoms <= MAX_SCREEN_LIGAND_ATOMS:
            raise ValueError(f'max_lig_atoms must be 1..{MAX_SCREEN_LIGAND_ATOMS} (got {max_lig_atoms})')
        ligands = list(ligands)
        names = [item[0] for item in ligands]
        ligands = [item for item in ligands if int(item[2].shape[0]) > 0]
        dev = self.rec_pos.device
        small = [k for k, (_, _, poses) in enumerate(ligands) if int(poses.shape[1]) <= max_lig_atoms]
        large = [k for k in range(len(ligands)) if int(ligands[k][2].shape[1]) > max_lig_atoms]
        sizes = [int(ligands[k][2].shape[1]) for k in small]
        counts = [int(ligands[k][2].shape[0]) for k in small]
        plan = plan_library(counts, sizes, self.b, max_lig_atoms)
        out, kept, kept_raw = {}, [], []
        with self._sweeping(predictions_file, sigmoid, hits_file) as sink:
            if plan:
                # the whole library packed once, in plan order: a batch is a contiguous range of it
                all_pos = torch.cat([ligands[k][2].to(dev).float().reshape(-1, 3) for k in small], 0)
                all_feats = torch.cat([ligands[k][1].to(dev).float().repeat(c, 1) for k, c in zip(small, counts)], 0)
                ptrs = slot_offsets([[sizes[lig] for lig, _ in batch] for batch in plan], self.b)
                ptrs_dev = ptrs.to(dev)
                screen = self._library_screen(max(sizes))
            next_large, at = 0, 0

            def run_large_before(k):       # the larger ligands whose place in the library is before ligand k
                nonlocal next_large
                while next_large < len(large) and large[next_large] < k:
                    name, lig_feats, poses = ligands[large[next_large]]
                    out[name] = self._run_ligand(name, lig_feats, poses, sink)
                    next_large += 1

            for b, batch in enumerate(plan):
                batch_sizes = [sizes[lig] for lig, _ in batch]
                total = int(ptrs[b, -1])
                screen.load_packed(all_pos[at:at + total], all_feats[at:at + total], ptrs_dev[b], batch_sizes)
                at += total
                raw = self._library_step(screen)
                y = sink.scored(raw)
                kept.append(y[:len(batch)])
                if sink.raw is not None:
                    kept_raw.append(raw[:len(batch)])
                self.batches_run += 1
                if sink.writers:
                    lo = 0
                    while lo < len(batch):      # one submit per run of slots that no larger ligand interrupts
                        run_large_before(small[batch[lo][0]])
                        hi = lo + 1
                        stop = large[next_large] if next_large < len(large) else len(ligands)
                        while hi < len(batch) and small[batch[hi][0]] < stop:
                            hi += 1
                        sink.write(y[lo:hi], [f'{ligands[small[lig]][0]}_pose{pose}' for lig, pose in batch[lo:hi]])
                        lo = hi
            run_large_before(len(ligands))
            if plan:
                screen.check()
                scores, at = torch.cat(kept, 0), 0
                raw_scores = torch.cat(kept_raw, 0) if kept_raw else None
                for k, c in zip(small, counts):
                    out[ligands[k][0]] = scores[at:at + c]
                    if raw_scores is not None:
                        sink.keep_raw(ligands[k][0], raw_scores[at:at + c])
                    at += c
            self._pick_hits(names, sink, hits_file)
        return {name: out[name] for name, _, _ in ligands}

    def best_poses(self, ligands):
        """(name, lig_feats, poses[best]) of every ligand of `ligands` - what `run` / `run_library(hits_file=...)` was
        given - that has a best pose in `self.hits`; a ligand without one (no poses, NaN scores only) is skipped. What
        `ligand_atom_masking` takes."""
        for name, lig_feats, poses in ligands:
            best = self.hits.get(name, (-1, None))[0]
            if best >= 0:
                yield name, lig_feats, poses[best]

    # ---- attribution of hits: the bodies are in hit_attribution.py ----
    def _no_attribution_when_cropped(self, method):
        if self.cropped_attribution and method != 'receptor_hotspots':      # (the three masking methods: opted in)
            return
        if self.cropped_hotspots and method == 'receptor_hotspots':         # (the maps: opted in on their own)
            return
        if self.crop_radius is not None:
            raise NotImplementedError(
                f'ScreeningSweep(crop_radius=...).{method}: the reference masks after cropping around the WHOLE '
                'ligand, so a copy must not be cropped again around what is left of it - and the attention and CAM '
                'reductions assume n_rec receptor rows per slot. Not built yet: use a sweep without crop_radius')

    def ligand_atom_masking(self, items, scores_file=None, sigmoid=None, column=0):
        """Atom masking (the reference's attribution_fns.atom_masking, :365-431) of the LIGAND atoms of many complexes
        with this receptor: items = iterable of (name, lig_feats [n,F], pose [n,3]), n <= MAX_SCREEN_LIGAND_ATOMS,
        unique names. A complex without ligand atom a is a pose of an (n - 1)-atom ligand, and its radius graph is what
        the reference's masking leaves (the atom goes together with its edges): every item's n + 1 copies - the whole
        ligand, then one per atom left out - stream through ONE LibraryScreen in dense batches, laid out on the device
        (LibraryScreen.load_leave_out: one packer launch per batch, then the one captured step), ceil((sum n +
        len(items)) / batch_size) steps in all (and, for a new screen, one batch of the batch_size largest whole ligands
        before them, from which the screen sizes its edge buffers).
        Returns {name: scores [n] on the device}, scores[a] = s(y_whole[column]) - s(y_without_a[column]), s = the
        sigmoid where a sweep applies it to that column (`sigmoid` as in `run`; False: raw differences);
        `self.atom_masking_raw[name]` keeps the raw rows [n + 1, C], whole ligand first. scores_file: one line per
        ligand atom, item order then atom order, '{score:.6f} | {receptor} {name}_atom{a}'."""
        self._no_attribution_when_cropped('ligand_atom_masking')
        from . import hit_attribution
        return hit_attribution.ligand_atom_masking(self, items, scores_file, sigmoid, column)

    def contact_masking(self, items, scores_file=None, sigmoid=None, column=None):
        """Bond masking (the reference's attribution_fns.bond_masking, its default way to rank interactions) of the
        ligand-receptor contacts of many complexes with this receptor: items as for `ligand_atom_masking`. A contact is
        a pair (ligand atom a, receptor atom r) with a class-1 edge at the sweep's edge radius (PF.contact_pairs, on the
        device); the complex without both atoms is a struck pose-batch slot - the (n - 1)-atom ligand against the
        receptor without r - whose graph is what the reference's masking leaves. Every item's K + 1 copies (the whole
        complex, then one per contact, by a then r) stream through ONE LibraryScreen(struck=True), `self.struck`, in
        dense batches: ceil((sum K + len(items)) / batch_size) steps (and the sizing batch of a new screen).
        Returns {name: (pairs [K,2] int32, scores [K])} on the device, scores[k] = s(y_whole[column]) -
        s(y_without_pair_k[column]); column None: the reference's rule, column 1 of more than one output, else column 0
        (tasks='both': name it). One value per unordered pair (the reference lists a contact once per direction, with
        equal scores). `self.contact_masking_raw[name]`: the raw rows [K + 1, C]. scores_file: one line per contact,
        item order then pair order, '{score:.6f} | {receptor} {name}_atom{a} atom{r}'."""
        self._no_attribution_when_cropped('contact_masking')
        from . import hit_attribution
        return hit_attribution.contact_masking(self, items, scores_file, sigmoid, column)

    def receptor_atom_masking(self, items, atoms='contacts', scores_file=None, sigmoid=None, column=0):
        """Atom masking (the reference's attribution_fns.atom_masking) of RECEPTOR atoms of many complexes with this
        receptor, through the same struck screen as `contact_masking`: a copy keeps the whole ligand and lacks one
        receptor atom. atoms: 'contacts' (per hit, the receptor atoms in at least one of its contacts, ascending),
        'all' (every receptor atom) or a 1-D index tensor that applies to every hit. Returns {name: (atoms [M] int32,
        scores [M])} on the device, scores[m] = s(y_whole[column]) - s(y_without_atom_m[column]);
        `self.receptor_atom_masking_raw[name]`: the raw rows [M + 1, C]. scores_file: one line per atom, item order
        then atom order, '{score:.6f} | {receptor} {name} atom{r}'."""
        self._no_attribution_when_cropped('receptor_atom_masking')
        from . import hit_attribution
        return hit_attribution.receptor_atom_masking(self, items, atoms, scores_file, sigmoid, column)

    def receptor_hotspots(self, items, gnn_layer=1, scores_file=None, per_hit=False, attribution='edge_attention',
                          column=None, ligand_scores_file=None, atoms='contacts', sigmoid=None, use_rank=False, top=None):
        """Which receptor atoms the hits of a sweep bind to (the reference's attribution/hotspot.py with its default
        attribution, edge_attention): items as for `ligand_atom_masking` - (name, lig_feats [n,F], pose [n,3]), unique
        names, e.g. `best_poses(ligands)` - are the binding events; per event every atom gets the largest attention
        value of layer `gnn_layer` (an index into model.layers as the reference's `--layer`: 1 = the first EGNN layer,
        negative from the end) over its ligand-receptor edges, and a receptor atom's score is the mean of these over
        the events in which it has such an edge. The whole ligands stream through ONE LibraryScreen (`self.hotspot`,
        built with contact_attention=gnn_layer) in ceil(len(items) / batch_size) steps - and, for a new screen, one
        batch of the batch_size largest ligands before them, from which it sizes its edge buffers; that batch and the
        warm-up steps of the capture are not part of the result. The reduction runs inside the step on the device
        (PF.contact_attention); nothing is copied to the host per hit.
        Returns a dict of device tensors: mean [n_rec] float64 (NaN for an atom without a contact), count [n_rec]
        int32 (the events in which the atom has a contact), max [n_rec] (its largest value over them, NaN without),
        ligand {name: [n]} (the same per ligand atom of each hit, NaN without a contact) and, with per_hit, per_hit
        [len(items), n_rec] (every event's values, item order). scores_file: one line per receptor atom that has a
        contact, atom order, '{mean:.6f} {count} | {receptor} atom{j}'.
        attribution='cam' (the reference's `--scoring_method cam`): the value of an atom is the class-activation map
        instead - the heads the sweep evaluates, applied to the atom's final embedding; `column`: None for the
        reference's rule (one output: itself, three: their mean), else a column of the raw outputs (required with
        tasks='both'). Every atom has a value, so count is the number of hits that have atoms, for every receptor
        atom, and scores_file gets a line for each; `gnn_layer` is ignored. The hits stream through `self.cam_screen`
        (LibraryScreen(cam=...)), which needs neither an attention layer nor the first-layer reuse. Same keys.
        ligand_scores_file: one line per ligand atom of every hit, item order then atom order, '{value:.6f} |
        {receptor} {name}_atom{a}'.
        attribution='atom_masking' (the reference's `--scoring_method atom_masking`): the value of an atom in a hit is
        its masking score - this sweep's own `receptor_atom_masking(items, atoms=atoms, sigmoid=sigmoid, column=column
        or 0)` and `ligand_atom_masking(items, sigmoid=sigmoid, column=column or 0)`, whose `*_raw` attributes stay
        filled as those calls leave them - laid out as NaN-filled rows [hits, n_rec] and reduced over the hits on the
        device (PF.hit_rows_accumulate). Same keys: count[j] is the number of hits that list atom j. atoms: 'contacts'
        (default: per hit the receptor atoms in a contact), 'all' - on an uncropped sweep n_rec copies of every hit
        through the struck screen, n_rec * len(items) / batch_size steps; on a cropped sweep every hit's kept atoms,
        the reference's complex exactly - or a 1-D index tensor without repeats (ValueError otherwise). `atoms` and
        `sigmoid` with another attribution: ValueError; `gnn_layer` is ignored. On a sweep with crop_radius this
        attribution is opted in by cropped_attribution=True, the masking keyword, not by cropped_hotspots.
        use_rank=True (the reference's `--use_rank`): beside the values, every hit's values are replaced by their
        ranks within the hit - the position in a descending stable sort, 0 = best, ties to the earlier atom, the
        ligand atoms before the receptor's (PF.hit_value_ranks, once per batch behind the step, outside its capture);
        'edge_attention' ranks the receptor atoms among themselves, 'cam' and 'atom_masking' all atoms of the complex.
        Added keys: rank_mean [n_rec] float64 (the mean rank over the hits in which the atom has a value, NaN without
        one), ligand_rank {name: [n]} ('cam' and 'atom_masking'), per_hit_rank [len(items), n_rec] with per_hit;
        scores_file then carries rank_mean in place of mean. The value keys are what they are without use_rank.
        With use_rank or top: order, the receptor atoms with count > 0, best first - by mean descending, under
        use_rank by rank_mean ascending (the reference's final sort), ties to the lower atom - cut to the first `top`
        (the reference's `--cutoff`; top < 0: ValueError)."""
        if attribution == 'atom_masking':       # (gated as the masking methods it calls: cropped_attribution)
            self._no_attribution_when_cropped('receptor_atom_masking')
        else:
            self._no_attribution_when_cropped('receptor_hotspots')
        from . import hit_attribution
        return hit_attribution.receptor_hotspots(self, items, gnn_layer, scores_file, per_hit, attribution, column,
                                                 ligand_scores_file, atoms, sigmoid, use_rank, top)
