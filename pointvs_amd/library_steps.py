"""The three steps of a LibraryScreen (screening.py), one class per route, and the one rule that picks the route.

    plain     the model's own forward on a batch from the general radius-graph builder
    reuse     the first-layer reuse: the receptor-receptor side of the first layer kept once, both CSRs from the slot builder
    cropped   every slot cropped around its ligand: the full CSR alone, every layer through forward_prepared

`library_route` decides from the model's facts and the keywords, once, at the screen's construction; the screen then calls
its step (`screen._step`) and asks it - never its own keywords or the keys of a buffer dict - what the route does: which
buffers the step and its capacity probe need, how the builder job is filled and launched, the forward from the built
buffers to the outputs, the map reductions, and why the step cannot be captured. The value buffers, the inputs and every
`load*`, the status word and capture / replay stay with the screen. Also here, because both screens and the steps use them:
the buffers of a device-built pose-batch graph and the graph structs over them."""
import ctypes as C

import torch

from . import _lib
from . import functional as PF

PLAIN, REUSE, CROPPED = 'plain', 'reuse', 'cropped'


def library_route(hidden, edge_residual, softmax_attention, edge_attention, softmax_reuse=False, crop_radius=None):
    """The route of a LibraryScreen. Pure host logic: no device, no allocation.
    hidden, softmax_attention, edge_attention: the first EGNN layer's (hidden None: a model without one);
    edge_residual: whether any EGNN layer has it; softmax_reuse, crop_radius: the screen's keywords.
    crop_radius selects CROPPED for every model the screen lets through (captured_scoring.model_refusal is the
    constructor's business, before this). Else REUSE needs a hidden size of 32 or 64, no edge_residual, and no softmax
    attention - unless softmax_reuse is on and the first layer has edge attention, whose softmax statistics merge (a
    softmax flag without edge attention stays out). Everything else is PLAIN."""
    if crop_radius is not None:
        return CROPPED
    sums_merge = not softmax_attention or bool(softmax_reuse and edge_attention)
    return REUSE if hidden in (32, 64) and sums_merge and not edge_residual else PLAIN


def model_route(model, softmax_reuse=False, crop_radius=None):
    """`library_route` of a model: reads the facts off model.layers (layer 0 is the embedding)."""
    egnn = list(model.layers)[1:]
    first = egnn[0] if egnn else None
    return library_route(None if first is None else first.hidden_nf, any(l.edge_residual for l in egnn),
                         bool(first is not None and first.softmax_attention),
                         bool(first is not None and first.edge_attention), softmax_reuse, crop_radius)


def _csr_buffers(dev, n_nodes, cap_l, cap=None, **extra):
    """Buffers of a device-built pose-batch graph over n_nodes nodes: the ligand-touching CSR (`*_l`, room for cap_l
    edges; None: without it) and, with `cap`, the full CSR and its inv_deg; the builder's status word; `ones` (the
    ligand-touching graph's inv_deg). The builders read f['cap'] / f['cap_l'] at every launch."""
    i32 = dict(dtype=torch.int32, device=dev)
    f = dict(cap=cap, cap_l=cap_l, status=torch.zeros(1, **i32), **extra)
    for tag, c in (('', cap), ('_l', cap_l)):
        if c is not None:
            f['rowptr' + tag] = torch.empty(n_nodes + 1, **i32)
            f['row' + tag] = torch.empty(c, **i32)
            f['col' + tag] = torch.empty(c, **i32)
            f['etype' + tag] = torch.empty(c, dtype=torch.uint8, device=dev)
    if cap is not None:
        f['inv_deg'] = torch.empty(n_nodes, dtype=torch.float32, device=dev)
    f['ones'] = torch.ones(n_nodes, dtype=torch.float32, device=dev)
    return f


def _ligand_csr(f, n_nodes, n_end):
    """PvsGraph of f's ligand-touching CSR over the first n_nodes nodes; its edge count stays on the device, in
    rowptr_l[n_end] (the rows from n_nodes to n_end are padding, without edges)."""
    gl = _lib.PvsGraph()
    gl.n_nodes, gl.n_edges = n_nodes, f['cap_l']
    gl.rowptr, gl.row, gl.col, gl.etype = (_lib.ptr(f[k + '_l']) for k in ('rowptr', 'row', 'col', 'etype'))
    gl.inv_deg = _lib.ptr(f['ones'])
    gl.n_edges_dev = f['rowptr_l'][n_end:].data_ptr()
    return gl


def _full_graph(f, n_nodes, n_end):
    """PreparedGraph of f's full CSR over the first n_nodes nodes, its edge count on the device (rowptr[n_end])."""
    from .graph import PreparedGraph
    csr = {k: f[k] for k in ('rowptr', 'row', 'col', 'etype', 'inv_deg', 'status')}
    return PreparedGraph.over_buffers(n_nodes, f['cap'], csr, f['rowptr'][n_end:])


def _graph_pair(f, n_nodes, n_end):
    """(`_full_graph`, `_ligand_csr`) of f over the first n_nodes nodes."""
    return _full_graph(f, n_nodes, n_end), _ligand_csr(f, n_nodes, n_end)


class _Step:
    """What the steps share. `s` is the screen: its inputs, its keywords and its value buffers are read there by name at
    every use, so that whatever a refresh replaces (the template, the receptor sums) is simply read again.
    The two builder steps (`has_builder`: the screen's own fixed-shape step at N_cap nodes, what `screen.reuse` reports)
    share the slot builder's own buffers, the job fields of every layout and the launch; all three share the per-node
    heads of `cam`."""
    has_builder = True

    def __init__(self, screen):
        self.s = screen

    def capture_refusal(self):
        """Why the step cannot be captured: a string, or None."""
        return None

    def keep(self):
        raise RuntimeError('keep: the masks of a cropped screen (crop_radius=...) after its first step')

    def run(self):
        """One step on the loaded batch: the cached receptor side refreshed where the weights changed, the builder, then
        the route's forward."""
        self.s._refresh_if_stale()
        return self.forward(self.s._build())

    # ---- the slot builder ----
    def _builder_buffers(self, layout, feats=True):
        """What pvs_screen_slots_build of `layout` writes beside the CSRs, over N_cap nodes: its state, node_ptr,
        node_graph, pos and (feats) the feature rows x."""
        s = self.s
        dev, n_cap = s.lig_pos.device, s.n_cap
        i32 = dict(dtype=torch.int32, device=dev)
        f32 = dict(dtype=torch.float32, device=dev)
        counts = _lib.PvsScreenSlotsJob(layout=layout, n_slots=s.b, lig_cap=s.l_cap, n_rec=s.n_rec, slot_cap=s.slot_cap)
        own = dict(
            state=torch.empty(_lib.lib().pvs_screen_slots_state_bytes(C.byref(counts)), dtype=torch.uint8, device=dev),
            node_ptr=torch.zeros(s.b + 1, **i32), node_graph=torch.empty(n_cap, **i32),
            pos=torch.empty((n_cap, 3), **f32))
        if feats:
            own['x'] = torch.empty((n_cap, s.lig_feats.shape[1]), **f32)
        return own

    def _slots_job(self, f, layout, probe, lig_csr, feats=True):
        """The PvsScreenSlotsJob of the loaded batch into f as far as every layout has it, filled at every launch from
        the screen's attributes and f by name: nothing keeps a device address across steps. probe: no room for edges.
        lig_csr: f has the ligand-touching CSR; feats: f has feature rows."""
        p, s = _lib.ptr, self.s
        job = _lib.PvsScreenSlotsJob(
            layout=layout, lig_pos=p(s.lig_pos), lig_ptr=p(s.lig_ptr), rec_drop=p(s.rec_drop) if s.struck else None,
            rec_pos=p(s._rec_pos), rr_rowptr=p(s._rr.t['rowptr']), rr_col=p(s._rr.t['col']), n_slots=s.b,
            lig_cap=s.l_cap, n_rec=s.n_rec, slot_cap=s.slot_cap, inter_radius=float(s.r_inter),
            intra_radius=float(s.r_intra), inv_deg=p(f['inv_deg']), node_ptr=p(f['node_ptr']),
            node_graph=p(f['node_graph']), pos=p(f['pos']), status=p(f['status']))
        full = job.full
        full.rowptr, full.row, full.col, full.etype = p(f['rowptr']), p(f['row']), p(f['col']), p(f['etype'])
        full.capacity = 0 if probe else f['cap']
        if lig_csr:
            lig = job.lig
            lig.rowptr, lig.row, lig.col, lig.etype = p(f['rowptr_l']), p(f['row_l']), p(f['col_l']), p(f['etype_l'])
            lig.capacity = 0 if probe else f['cap_l']
        if feats:
            t = job.tables
            t.n_feats, t.feats = f['x'].shape[1], p(f['x'])
            t.lig_feats, t.rec_feats = p(s.lig_feats), p(s._rec_feats)
        return job

    def launch(self, f, probe=False):
        """pvs_screen_slots_build of the loaded batch into f."""
        job = self.job(f, probe)
        _lib.check(_lib.lib().pvs_screen_slots_build(C.byref(job), _lib.ptr(f['state']), f['state'].numel(),
                                                     _lib.stream(self.s.lig_pos.device)), 'pvs_screen_slots_build')

    # ---- cam ----
    def _node_heads(self, h):
        """The heads on every row of the final embedding h [n, H] into cam['node_y'][:n] - one launch (PF.node_heads)
        when every head is one that PF.pool_heads takes, else each head per node on the linear op. Returns node_y[:n],
        the column and the number of columns averaged, and the output buffers of the slots' values."""
        s = self.s
        heads, widths, column, n_mean = s._cam_plan
        c, n = s.cam, h.shape[0]
        node_y = c['node_y'][:n]
        fused = [s.model._fused_head(head) for head in heads]
        if all(f is not None for f in fused) and len(fused) <= PF.MAX_POOL_HEADS and h.shape[1] <= PF.POOL_HEAD_MAX_WIDTH:
            PF.node_heads(h, fused, out=node_y)
        else:
            at = 0
            for head, width in zip(heads, widths):
                node_y[:, at:at + width].copy_(s.model._run_head(head, h).reshape(n, width))
                at += width
        return node_y, column, n_mean, (c['lig_val'], c['slot_rec_val'], c['rec_sum'], c['rec_count'], c['rec_max'])

    def _reduce_cam(self, h, node_ptr, lig_ptr):
        """`cam` of a step whose slots hold the whole receptor: the heads per node, then the slots' values and the
        accumulators (PF.slot_node_values)."""
        node_y, column, n_mean, out = self._node_heads(h)
        PF.slot_node_values(node_y, node_ptr, lig_ptr, self.s.n_rec, column, n_mean, out=out)


class _PlainStep(_Step):
    """The models the first-layer reuse does not cover (edge_residual, softmax attention without softmax_reuse, a hidden
    size other than 32 / 64), uncropped: the same mixed batch, its graph from the general radius-graph builder
    (radius_graph.attach_radius_graph) at the exact node count, then the model's own forward - or, for `tasks` / `cam`,
    its trunk and the same head code as the other routes. No builder, no buffers (`_fast` stays None), nothing to
    capture; `cam` runs eagerly behind it, struck slots and contact_attention are refused."""
    has_builder = False

    def __init__(self, screen):
        super().__init__(screen)
        if screen.struck:
            raise ValueError(
                'LibraryScreen(struck=True): struck slots are built for the step of the first-layer reuse, which this '
                'model does not have (softmax attention without softmax_reuse=True, edge_residual or a hidden size other '
                'than 32 / 64); mask it '
                'one complex at a time with pointvs_amd.attribution.bond_masking / atom_masking')
        if screen.contact_attention is not None:
            raise NotImplementedError(
                f'LibraryScreen(contact_attention={screen._contact_request}): the contact-attention reduction '
                'runs in the step of the first-layer reuse, which this model does not have (softmax attention without '
                'softmax_reuse=True, edge_residual or a hidden size other than 32 / 64 take the plain forward)')

    def capture_refusal(self):
        return ('capture needs the first-layer reuse (no edge_residual, no softmax attention - or '
                'softmax_reuse=True -, hidden size 32 or 64)')

    def cache_receptor(self):
        """(nothing of the receptor is kept)"""

    def run(self):
        from .graph import Batch
        from .radius_graph import attach_radius_graph
        s = self.s
        dev = s.lig_pos.device
        pos, x, counts, at = [], [], [], 0
        for n in s._sizes:
            pos += [s.lig_pos[at:at + n], s._rec_pos]
            x += [s.lig_feats[at:at + n], s._rec_feats]
            counts.append(n + s.n_rec)
            at += n
        ptr = torch.tensor([0] + counts, dtype=torch.int64).cumsum(0)
        batch = Batch(x=torch.cat(x, 0), pos=torch.cat(pos, 0), edge_index=None, edge_attr=None,
                      batch=torch.arange(s.b, device=dev).repeat_interleave(torch.tensor(counts, device=dev)),
                      ptr=ptr, y=torch.zeros(s.b, device=dev), lig_fname=['pose'] * s.b,
                      rec_fname=['receptor'] * s.b, num_graphs=s.b, graph_node_counts=counts)
        y = s._plain(attach_radius_graph(batch, s.r_inter, s.r_intra))
        if s.cam is not None:      # (eager: the offsets come from the host-known sizes)
            lig_ptr = torch.tensor([0] + list(s._sizes), dtype=torch.int64).cumsum(0).to(device=dev, dtype=torch.int32)
            self._reduce_cam(s._h_final.contiguous(), s._plain_ptr, lig_ptr)
        return y


class _ReuseStep(_Step):
    """The first-layer reuse. What ReceptorScreen reuses across the poses of one ligand is reused across ligands: the
    receptor-receptor template CSR and the first layer's receptor-receptor sums (kept once, `screen.rec_magg` /
    `rec_xsum` / `rec_deg` [n_rec, .]), the ligand-touching first layer, device-side edge counts. The mixed batch's graph
    and node tables come from pvs_screen_slots_build (PVS_SLOTS_RAGGED; slot cap max(max_lig_atoms, 64): ceil(cap / 64)
    ligand-ligand words per atom) in a compact layout (slot p: its ligand atoms, then the receptor): both CSRs, the feature
    rows x and the base rows base_magg / base_xsum / base_deg, which the builder expands from the receptor's. The step:
    the embedding, the partial first layer over the ligand-touching CSR on top of the base rows, the other layers over the
    full CSR, pooling and heads by node_ptr. It runs at the padded shape N_cap - a GraphNorm model at the exact node
    count instead, eager only, unless padded_graphnorm is on (`_graphs`, by node count); under slot_graphnorm every slot
    is normalised by its own rows (the slots' node_ptr as the layers' segment table).
    Variants: softmax_reuse - the base rows are H + 4 floats (PvsRaggedNodeTables.hidden is a free row width) and the
    attention is normalised over ALL edges of a row; struck - PVS_SLOTS_STRUCK slots read `screen.rec_drop`: the rows that
    had the struck atom r as a receptor-receptor neighbour take their whole first-layer row through the ligand-touching
    CSR with a zero base, every other row and every kernel is as without it; contact_attention - the layer's edge attention
    reduced per atom (PF.contact_attention) over the ligand-touching CSR (layer 1, from `att_l`) or the full one."""

    def __init__(self, screen):
        super().__init__(screen)
        self.layout = _lib.SLOTS_STRUCK if screen.struck else _lib.SLOTS_RAGGED

    def capture_refusal(self):
        if self.s.graphnorm and not self.s._gn_padded:
            return ('a graphnorm model normalises over the batch\'s nodes and runs at the exact node '
                    'count: it cannot be captured at the padded shape; call the screen eagerly')
        return None

    def cache_receptor(self):
        """The receptor sums kept once, [n_rec, .]; every builder launch reads them (and the template) anew (`job`)."""
        s = self.s
        s.rec_magg, s.rec_xsum, s.rec_deg = s._receptor_sums(s._rec_feats, s._rec_pos)

    def buffers(self, cap, cap_l):
        """Both CSRs (room for cap / cap_l edges), the builder's own buffers with the feature rows, the first-layer base
        rows (a row's width: the hidden size + the reuse kind's row_extra), for contact_attention=1 the first EGNN
        layer's attention in the ligand-touching CSR's order, and `pgs`: the graph pairs of `_graphs`, by node count."""
        s = self.s
        f32 = dict(dtype=torch.float32, device=s.lig_pos.device)
        own = self._builder_buffers(self.layout)
        own.update(base_magg=torch.empty((s.n_cap, s.rec_magg.shape[1]), **f32),
                   base_xsum=torch.empty((s.n_cap, 3), **f32), base_deg=torch.empty(s.n_cap, **f32))
        f = _csr_buffers(f32['device'], s.n_cap, cap_l, cap, **own)
        if s.contact_attention == 1:
            f['att_l'] = torch.empty(max(cap_l, 1), **f32)
        f['pgs'] = {}
        return f

    def probe_buffers(self):
        """(a set like the step's, so that the step's buffers are then allocated as they always were)"""
        return self.buffers(1, 1)

    def job(self, f, probe=False):
        p, s = _lib.ptr, self.s
        job = self._slots_job(f, self.layout, probe, lig_csr=True)
        t = job.tables
        t.hidden, t.rec_magg, t.rec_xsum, t.rec_deg = f['base_magg'].shape[1], p(s.rec_magg), p(s.rec_xsum), p(s.rec_deg)
        t.base_magg, t.base_xsum, t.base_deg = p(f['base_magg']), p(f['base_xsum']), p(f['base_deg'])
        return job

    def _graphs(self, n):
        """(PreparedGraph of the full CSR, PvsGraph of the ligand-touching CSR) over the first n nodes (the nodes
        after n are padding, without edges: rowptr[n] == rowptr[N_cap] == the edge count)."""
        s = self.s
        pgs = s._fast['pgs']
        if n not in pgs:
            pgs[n] = _graph_pair(s._fast, n, s.n_cap)
            if s._gn_slots:       # slot_graphnorm: every slot by its own rows, the slots' node_ptr as the segment table
                node_ptr = s._fast['node_ptr']
                pgs[n][0].set_norm_segments(node_ptr)
                pgs[n][1].n_norm_rows_dev, pgs[n][1].n_graphs = node_ptr.data_ptr(), s.b
            elif s._gn_padded:    # both graphs: the partial first layer's and the full one of the layers behind it
                real_nodes = s._fast['node_ptr'][s.b:]
                pgs[n][0].set_norm_rows(real_nodes)
                pgs[n][1].n_norm_rows_dev = real_nodes.data_ptr()
        return pgs[n]

    def forward(self, f):
        s = self.s
        # graphnorm's statistics run over the batch's nodes: no padding rows there (the host knows the count) - or, with
        # padded_graphnorm, the padded shape and the count where the builder left it (PvsGraph.n_norm_rows_dev)
        exact = s.graphnorm and not s._gn_padded
        n = s.n_atoms + s.b * s.n_rec - s._n_struck if exact else s.n_cap
        pg_full, g_lig = self._graphs(n)
        x = f['pos'][:n]
        h = s.embed.embed(f['x'][:n], x).contiguous()
        h, x = s._partial_first_layer(g_lig, h, x, f['base_magg'], f['base_xsum'], f['base_deg'],
                                      s.n_cap, f['cap_l'], f.get('att_l'))
        y = s._tail(pg_full, h, x)
        if s.contact_attention == 1:
            self._reduce_contacts(f, '_l', f['att_l'])
        elif s.contact_attention is not None:      # (a later layer: what its forward_prepared left, full CSR order)
            self._reduce_contacts(f, '', s.model.layers[s.contact_attention]._att_sorted)
        if s.cam is not None:
            self._reduce_cam(s._h_final, f['node_ptr'], s.lig_ptr)
        return y

    def _reduce_contacts(self, f, tag, att):
        """PF.contact_attention over f's CSR `tag` ('_l': ligand-touching, '': full) with `att` in its edge order."""
        s, c = self.s, self.s.contact
        PF.contact_attention(f['rowptr' + tag], f['etype' + tag], att, f['node_ptr'], s.lig_ptr, s.n_rec,
                             out=(c['lig_att'], c['slot_rec_att'], c['rec_sum'], c['rec_count'], c['rec_max']))


class _CroppedStep(_Step):
    """crop_radius: every slot keeps only the receptor atoms closer than it to one of the slot's ligand atoms (fp64
    decision on the fp32 coordinates, strict, a coincident atom is kept; an empty slot keeps nothing), in receptor order
    behind the ligand atoms, and the slot's graph is generate_edges on that cropped complex. The builder is
    pvs_screen_slots_build (PVS_SLOTS_CROPPED): the full CSR alone, the feature rows and the keep masks `keep`
    [batch_size, ceil(n_rec / 64)] int64 (bit j % 64 of word j / 64), `node_ptr` the slots' offsets; then the embedding
    and EVERY EGNN layer through forward_prepared on the ONE PreparedGraph `pg` over N_cap nodes (edge count on the
    device), pooling and heads by node_ptr. Of the receptor only the template CSR is kept: the first-layer sums are not
    used (a row at the rim of the crop has lost template neighbours). The capacity probe is the uncropped builder's
    (PVS_SLOTS_RAGGED into row pointers, node_ptr and pos alone): an uncropped batch bounds its cropped one.
    Variants: crop_parents - the slots may be leave-out copies, cropped around `screen.crop_pos` / `crop_ptr` (their
    parents' atoms) and without the receptor atom `screen.rec_drop` names: the builder is pvs_screen_copies_build on the
    same job, everything behind it is the same step; cropped_maps - behind the tail, `contact_attention` (any layer with
    edge attention: every layer runs on the full CSR, so the values are the layer's own) and `cam` through
    PF.contact_attention_cropped / PF.slot_node_values_cropped, which find a receptor atom's row through the slot's keep
    mask; an atom that a slot does not keep has NaN in slot_rec_att / slot_rec_val and adds nothing to rec_count."""

    def cache_receptor(self):
        """(a cropped step keeps the template and no sums)"""
        self.s._receptor_template(self.s._rec_pos)

    def keep(self):
        return super().keep() if self.s._fast is None else self.s._fast['keep']

    def buffers(self, cap, cap_l=None):
        """The full CSR (room for cap edges), the builder's own buffers with the feature rows, the keep masks and the
        PreparedGraph of the full CSR over N_cap nodes."""
        s = self.s
        dev = s.lig_pos.device
        own = self._builder_buffers(_lib.SLOTS_CROPPED)
        own['keep'] = torch.zeros((s.b, (s.n_rec + 63) // 64), dtype=torch.int64, device=dev)
        f = _csr_buffers(dev, s.n_cap, None, cap, **own)
        f['pg'] = _full_graph(f, s.n_cap, s.n_cap)
        if s._gn_slots:
            f['pg'].set_norm_segments(f['node_ptr'])
        elif s.graphnorm:
            f['pg'].set_norm_rows(f['node_ptr'][s.b:])
        return f

    def probe_buffers(self):
        return _csr_buffers(self.s.lig_pos.device, self.s.n_cap, 1, 1, **self._builder_buffers(_lib.SLOTS_RAGGED, False))

    def job(self, f, probe=False):
        if probe:
            return self._slots_job(f, _lib.SLOTS_RAGGED, True, lig_csr=True, feats=False)
        job = self._slots_job(f, _lib.SLOTS_CROPPED, False, lig_csr=False)
        job.crop_radius, job.keep = self.s.crop_radius, _lib.ptr(f['keep'])
        return job

    def launch(self, f, probe=False):
        """As every step's; the step proper of a crop_parents screen through pvs_screen_copies_build."""
        if probe or not self.s.crop_parents:
            return super().launch(f, probe)
        p, s = _lib.ptr, self.s
        PF.screen_copies_build(_lib.PvsScreenCopiesJob(slots=self.job(f), crop_pos=p(s.crop_pos), crop_ptr=p(s.crop_ptr),
                                                       rec_drop=p(s.rec_drop), crop_cap=s.l_cap), f['state'])

    def forward(self, f):
        s = self.s
        x = f['pos']
        y = s._tail(f['pg'], s.embed.embed(f['x'], x).contiguous(), x, layers=s.egnn)
        if s.contact is not None:      # (the attention that the layer's forward_prepared left in the full CSR's order)
            c = s.contact
            PF.contact_attention_cropped(
                f['rowptr'], f['etype'], s.model.layers[s.contact_attention]._att_sorted, f['node_ptr'], s.lig_ptr,
                f['keep'], s.n_rec, out=(c['lig_att'], c['slot_rec_att'], c['rec_sum'], c['rec_count'], c['rec_max']))
        if s.cam is not None:
            node_y, column, n_mean, out = self._node_heads(s._h_final)
            PF.slot_node_values_cropped(node_y, f['node_ptr'], s.lig_ptr, f['keep'], s.n_rec, column, n_mean, out=out)
        return y


STEPS = {PLAIN: _PlainStep, REUSE: _ReuseStep, CROPPED: _CroppedStep}
