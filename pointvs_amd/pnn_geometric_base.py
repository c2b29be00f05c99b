"""Graph unpacking, input embedding wrapper, pooling + head.

Mirrors /root/reference/point_vs/models/geometric/pnn_geometric_base.py:
  PNNGeometricBase.forward                   :24-41
  PNNGeometricBase.unpack_input_data_and_predict :43-53
  PNNGeometricBase.unpack_graph              :55-58
  PygLinearPass                              :61-94
"""
import os
from abc import abstractmethod

import torch
from torch import nn

from . import functional as PF
from .global_objects import DEVICE
from .graph import prepare_graph, prepared_for, runs_layout
from .point_neural_network_base import PointNeuralNetworkBase


def batch_tables(graph, batch):
    """(num_graphs, ptr: int64 node offsets) of a batch object: its own where it carries them, else derived from the
    batch vector with data-dependent ops (a maximum read on the host - the reference syncs there too, torch.max(batch),
    :27 - and a bincount). Whoever captures steps on the batch leaves them on it beforehand (StepReplayer)."""
    n_graphs = getattr(graph, 'num_graphs', None)
    if n_graphs is None:
        n_graphs = int(batch.max()) + 1
    ptr = getattr(graph, 'ptr', None)
    if ptr is None:
        counts = torch.bincount(batch, minlength=n_graphs)
        ptr = torch.cat([counts.new_zeros(1), counts.cumsum(0)])
    return n_graphs, ptr


class PNNGeometricBase(PointNeuralNetworkBase):
    """Base class of the geometric point networks."""

    @abstractmethod
    def get_embeddings(self, feats, edges, coords, edge_attributes, batch):
        """Input features -> final node embeddings."""

    def unpack_graph(self, graph):
        edges = getattr(graph, 'edge_index', None)      # None when the graph was built on the GPU
        attrs = getattr(graph, 'edge_attr', None)
        if self._model_dtype() == torch.float64:      # --double: features and coordinates in the model's dtype
            return (graph.x.to(DEVICE, torch.float64), None if edges is None else edges.to(DEVICE),
                    graph.pos.to(DEVICE, torch.float64), None if attrs is None else attrs.to(DEVICE),
                    graph.batch.to(DEVICE))
        return (graph.x.float().to(DEVICE), None if edges is None else edges.to(DEVICE),
                graph.pos.float().to(DEVICE), None if attrs is None else attrs.to(DEVICE),
                graph.batch.to(DEVICE))

    def _model_dtype(self):
        """float64 for a model built or moved to fp64 (the embedding's weight decides), else float32."""
        embed = self.layers[0] if getattr(self, 'layers', None) is not None and len(self.layers) else None
        w = getattr(getattr(embed, 'm', None), 'weight', None)
        return torch.float32 if w is None else w.dtype

    def _graph_inputs(self, graph):
        """The batch as the layer stack takes it: (feats, edges, coords, edge_attributes, n_graphs, graph_ptr: device
        int32 node offsets, layout, pg: the PreparedGraph of a graph built on the GPU or None)."""
        feats, edges, coords, edge_attributes, batch = self.unpack_graph(graph)
        n_graphs, ptr = batch_tables(graph, batch)
        # (the node offsets as device int32: from the batch's cached layout tables where it has them, else converted
        # ONCE per batch object - two conversions and a gather per step were three launches of ~4 us each)
        layout = None if edges is None else runs_layout(graph, feats.device)
        if layout is not None:
            graph_ptr = layout[0]
        else:
            cached = graph.__dict__.get('_pvs_ptr32') if hasattr(graph, '__dict__') else None
            if cached is not None and cached[0] is ptr and cached[1] == ptr._version and cached[2].device == feats.device:
                graph_ptr = cached[2]
            else:
                graph_ptr = ptr.to(device=feats.device, dtype=torch.int32).contiguous()
                if hasattr(graph, '__dict__'):
                    graph.__dict__['_pvs_ptr32'] = (ptr, ptr._version, graph_ptr)
        pg = getattr(graph, 'prepared', None)     # built on the GPU (radius_graph.attach_radius_graph)
        return feats, edges, coords, edge_attributes, n_graphs, graph_ptr, layout, pg

    @staticmethod
    def _coo_of(pg):
        """A graph built on the GPU: its sorted list back as the COO (edges, one-hot attributes) the dropout draws from."""
        e = pg.n_edges
        return (torch.stack([pg.t['row'][:e].long(), pg.t['col'][:e].long()]),
                None if pg.n_edge_attr == 0 else torch.nn.functional.one_hot(pg.t['etype'][:e].long(), pg.n_edge_attr))

    def _embed_graph(self, graph):
        feats, edges, coords, edge_attributes, n_graphs, graph_ptr, layout, pg = self._graph_inputs(graph)
        n_nodes = feats.size(0)
        dropping = self.training and float(getattr(self, 'dropout_p', 0.0) or 0.0) > 0.0
        if (dropping and getattr(self, 'static_dropout', None)
                and (pg.n_edges if pg is not None else int(edges.shape[1])) > 0):
            return self._embed_graph_static_dropout(graph, feats, edges, coords, edge_attributes, pg, graph_ptr, n_graphs)
        if dropping:      # edge dropout ahead of the layer stack (egnn_satorras.py:320-323): a new edge list
            if pg is not None:
                edges, edge_attributes = self._coo_of(pg)
            edges, edge_attributes = self.edge_dropout(edges, edge_attributes)
            pg = prepared_for(edges, edge_attributes, n_nodes)
        elif pg is None:
            pg = prepared_for(edges, edge_attributes, n_nodes, layout=layout)     # (sets graph_eptr itself from a layout)
        pg.poll_status()
        pg.set_graph_ptr(graph_ptr)
        feats, _, _ = self.embed_prepared(pg, feats, coords, need_coords=False)
        return feats, pg, graph_ptr, n_graphs

    # ---- edge dropout with a fixed-shape edge list (model.static_dropout; captured training turns it on) ----
    # None / False: the draw sizes its output by its result (one host read per step), today's path bit for bit.
    # True, while training with dropout > 0: the dropped list always has cap = 2 * #{row <= col} columns; the slots a
    # draw leaves empty hold edges between n_pad padding nodes appended behind the batch's own (features zero, the two
    # nodes of a pair 1 A apart), which pooling and heads never see: feats[:N] goes on, autograd's slice hands the
    # padding rows a zero gradient, so every padding edge contributes exact zeros to the weight gradients. Not for
    # GraphNorm models (the statistics run over all rows of the batch, padding included): the step raises.
    static_dropout = None

    def plan_static_dropout(self, graph):
        """static_dropout_state of a batch, ahead of the step that needs it (the replayer: _make_capturable). A batch
        without edges has no plan (its step takes the eager path, which then draws nothing)."""
        feats, edges, _, edge_attributes, n_graphs, graph_ptr, _, pg = self._graph_inputs(graph)
        if (pg.n_edges if pg is not None else int(edges.shape[1])) == 0:
            return None
        return self.static_dropout_state(graph, feats, edges, edge_attributes, pg, graph_ptr, n_graphs)

    def static_dropout_state(self, graph, feats, edges, edge_attributes, pg, graph_ptr, n_graphs):
        """What the static-shape draw needs of one batch object, computed ONCE, outside any capture, and left on the
        batch: the COO list the draw numbers (a graph built on the GPU: its sorted list), n_half = #{row <= col} (the
        one host read), (cap, n_pad) = PF.static_dropout_plan, the static output buffers, the padding rows and the node
        offsets extended by the padding block [..., N, N + n_pad] - a graph of its own for PvsGraph.graph_eptr, so
        tiles of the fp16-split backward end before it - and, for a batch of one graph, the offsets [0, N] the pooling
        shortcut reads (_whole_ptr). Whoever captures a step on these tensors keeps the state (the replayer does)."""
        n_nodes, p = int(feats.size(0)), float(self.dropout_p)
        source = pg if pg is not None else edges
        key = (None if pg is not None else (edges.data_ptr(), edges._version, tuple(edges.shape)),
               None if pg is not None or edge_attributes is None else (edge_attributes.data_ptr(), edge_attributes._version),
               n_nodes, p, feats.dtype, feats.device, int(feats.size(1)), n_graphs)
        holder = getattr(graph, '__dict__', None)
        state = None if holder is None else holder.get('_pvs_static_dropout')
        if state is not None and state['source'] is source and state['key'] == key:
            return state
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError('static edge dropout: the batch has no plan yet and counting its row <= col edges is a host '
                               'read, which a capture cannot hold (visit the batch once outside the capture)')
        if pg is not None:
            edges, edge_attributes = self._coo_of(pg)
        edges = edges.long().contiguous()
        if edge_attributes is not None:
            edge_attributes = edge_attributes.long().contiguous()
        n_half = int((edges[0] <= edges[1]).sum())
        cap, n_pad = PF.static_dropout_plan(n_nodes, n_half, p)
        dev = feats.device
        pad_coords = torch.zeros((n_pad, 3), dtype=feats.dtype, device=dev)     # (unpack_graph: one dtype)
        pad_coords[1::2, 0] = 1.0
        node_ptr = torch.cat([graph_ptr.to(device=dev, dtype=torch.long),
                              torch.tensor([n_nodes + n_pad], dtype=torch.long, device=dev)])
        node_ptr._pvs_as_long = node_ptr
        whole = None
        if n_graphs == 1:
            whole = torch.tensor([0, n_nodes], dtype=torch.int32, device=dev)
            whole._pvs_whole = n_nodes
        state = dict(
            source=source, key=key, edges=edges, attrs=edge_attributes, n_half=n_half, cap=cap, n_pad=n_pad,
            out_index=torch.empty((2, cap), dtype=torch.int64, device=dev),
            out_attr=(None if edge_attributes is None else
                      torch.empty((cap, int(edge_attributes.shape[1])), dtype=torch.int64, device=dev)),
            pad_feats=torch.zeros((n_pad, int(feats.size(1))), dtype=feats.dtype, device=dev), pad_coords=pad_coords,
            node_ptr=node_ptr, whole=whole)
        if holder is not None:
            holder['_pvs_static_dropout'] = state
        return state

    def _embed_graph_static_dropout(self, graph, feats, edges, coords, edge_attributes, pg, graph_ptr, n_graphs):
        if any(getattr(layer, 'graphnorm', False) for layer in self.layers):
            raise NotImplementedError('static_dropout does not cover a model with GraphNorm: the norm runs over every row '
                                      'of the batch, so the padding rows of the fixed-shape edge dropout would enter its '
                                      'statistics (leave static_dropout off: the eager draw has no padding)')
        n_nodes = int(feats.size(0))
        st = self.static_dropout_state(graph, feats, edges, edge_attributes, pg, graph_ptr, n_graphs)
        (seed, step), key_table = self.dropout_keys.take(self, feats.device)
        out_index, out_attr, n_kept = PF.dropout_adj_padded(
            st['edges'], st['attrs'], float(self.dropout_p), key_table, st['cap'], n_nodes, st['n_pad'],
            out=(st['out_index'], st['out_attr']))
        # prepare_graph, never prepared_for's cache: the static buffers are written through raw pointers, their tensor
        # _version never moves, and the cache would hand back the graph of an earlier draw
        dropped = prepare_graph(out_index, out_attr, n_nodes + st['n_pad'])
        dropped.poll_status()
        dropped.set_graph_ptr(st['node_ptr'])
        h, _, _ = self.embed_prepared(dropped, torch.cat([feats, st['pad_feats']]),
                                      torch.cat([coords, st['pad_coords']]), need_coords=False)
        self.last_dropout = dict(seed=seed, step=step, cap=st['cap'], n_pad=st['n_pad'], n_kept=n_kept,
                                 out_index=out_index, out_attr=out_attr)
        return h[:n_nodes], dropped, graph_ptr if st['whole'] is None else st['whole'], n_graphs

    @staticmethod
    def _whole_ptr(feats, graph_ptr):
        """[0, N] as device int32: the node offsets of a batch of one graph. The static-dropout path hands over the
        tensor it keeps with the batch's plan (tagged with its N: static_dropout_state), so that a captured step reads
        offsets that live as long as the batch does; every other caller gets a fresh tensor per call."""
        if getattr(graph_ptr, '_pvs_whole', None) == feats.size(0) and graph_ptr.device == feats.device:
            return graph_ptr
        return torch.tensor([0, feats.size(0)], dtype=torch.int32, device=feats.device)

    @classmethod
    def _pool(cls, feats, graph_ptr, n_graphs):
        """global_mean_pool, or plain mean over nodes for a single graph (:29-33)."""
        if n_graphs == 1:
            whole = cls._whole_ptr(feats, graph_ptr)
            return PF.mean_pool(feats, whole).reshape(-1)
        return PF.mean_pool(feats, graph_ptr)

    @staticmethod
    def _run_head(head, pooled):
        out = pooled
        for mod in head:
            out = PF.linear(out, mod.weight, mod.bias) if isinstance(mod, nn.Linear) else mod(out)
        return out

    @classmethod
    def _pool_and_head(cls, head, feats, graph_ptr, n_graphs):
        """head(pool(feats)) (:29-36). A head that starts with a Linear takes the pooling and that Linear as one
        op (PF.pool_head: one launch forward, one backward)."""
        mods = list(head)
        if (not mods or not isinstance(mods[0], nn.Linear) or feats.size(1) > PF.POOL_HEAD_MAX_WIDTH
                or feats.dtype != torch.float32                    # (fp64: mean_pool + linear)
                or os.environ.get('PVS_FUSED_HEAD') == '0'):       # (=0: the two ops apart, for A/B)
            return cls._run_head(head, cls._pool(feats, graph_ptr, n_graphs))
        if n_graphs == 1:
            whole = cls._whole_ptr(feats, graph_ptr)
            out = PF.pool_head(feats, whole, mods[0].weight, mods[0].bias).reshape(-1)
        else:
            out = PF.pool_head(feats, graph_ptr, mods[0].weight, mods[0].bias)
        return cls._run_head(mods[1:], out)

    @classmethod
    def _pool_and_head_padded(cls, head, feats, graph_ptr, n_graphs):
        """_pool_and_head for the fixed-shape steps, whose feats end in padding rows: with one graph the pooling still
        ends at graph_ptr[1] (a device word), not at feats' last row as _pool's plain mean would."""
        if n_graphs == 1:
            return cls._run_head(head, PF.mean_pool(feats, graph_ptr))
        return cls._pool_and_head(head, feats, graph_ptr, n_graphs)

    @staticmethod
    def _fused_head(head):
        """(weight, bias, act) when `head` is a Linear followed by nothing, ReLU or a default Softplus - what
        PF.pool_heads evaluates - else None."""
        mods = list(head)
        if not mods or len(mods) > 2 or not isinstance(mods[0], nn.Linear):
            return None
        act = None
        if len(mods) == 2:
            if isinstance(mods[1], nn.ReLU):
                act = 'relu'
            elif isinstance(mods[1], nn.Softplus) and mods[1].beta == 1 and mods[1].threshold == 20:
                act = 'softplus'
            else:
                return None
        return mods[0].weight, mods[0].bias, act

    @classmethod
    def _pool_and_heads(cls, heads, feats, graph_ptr, n_graphs):
        """Several heads on the same pooled embedding, forward only (the screens): [n_graphs, sum of the heads'
        outputs], the heads' columns side by side. One launch (PF.pool_heads) when every head is a Linear followed by
        nothing, ReLU or a default Softplus and the features are fp32 and at most POOL_HEAD_MAX_WIDTH wide; else (and
        with PVS_FUSED_HEAD=0, the A/B switch of _pool_and_head) one pooling, then each head."""
        fused = [cls._fused_head(head) for head in heads]
        if (heads and all(f is not None for f in fused) and len(fused) <= PF.MAX_POOL_HEADS
                and feats.dtype == torch.float32 and feats.size(1) <= PF.POOL_HEAD_MAX_WIDTH
                and os.environ.get('PVS_FUSED_HEAD') != '0'):
            return PF.pool_heads(feats, graph_ptr, fused)
        pooled = PF.mean_pool(feats, graph_ptr)
        return torch.cat([cls._run_head(head, pooled).reshape(n_graphs, -1) for head in heads], 1)

    def forward(self, x):
        feats, _, graph_ptr, n_graphs = self._embed_graph(x)
        if self.feats_linear_layers is not None:
            feats = self._pool_and_head(self.feats_linear_layers, feats, graph_ptr, n_graphs)
        return feats

    def unpack_input_data_and_predict(self, input_data):
        y_true = input_data.y
        try:
            y_true = y_true.float()
        except (AttributeError, TypeError):
            pass
        y_pred = self(input_data).reshape(-1, )
        return y_pred, y_true, input_data.lig_fname, input_data.rec_fname


class PygLinearPass(nn.Module):
    """Linear input embedding with the layer-like call signature (:61-94)."""

    def __init__(self, module, feats_appended_to_coords=False, return_coords_and_edges=False):
        super().__init__()
        if feats_appended_to_coords:
            raise NotImplementedError('feats_appended_to_coords is only used by the lucid EGNN')
        self.m = module
        self.feats_appended_to_coords = feats_appended_to_coords
        self.return_coords_and_edges = return_coords_and_edges
        self._coords_src = None

    @property
    def intermediate_coords(self):
        return None if self._coords_src is None else self._coords_src().detach().cpu().numpy()

    @intermediate_coords.setter
    def intermediate_coords(self, value):
        self._coords_src = None if value is None else (lambda: torch.as_tensor(value))

    def embed(self, h, coord=None):
        if coord is not None:
            self._coords_src = lambda: coord
        return PF.linear(h, self.m.weight, self.m.bias)

    def forward(self, h, **kwargs):
        res = self.embed(h, kwargs.get('coord'))
        if self.return_coords_and_edges:
            return res, kwargs['coord'], kwargs['edge_attr'], kwargs.get('edge_messages', None)
        return res
