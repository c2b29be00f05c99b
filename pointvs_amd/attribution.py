"""Attribution: which atoms (or ligand-receptor contacts) drive a score.

Mirrors /root/reference/point_vs/attribution/attribution_fns.py for the geometric models:
  bond_masking    :39-115      atom_masking :356-456
  cam             :298-353     node_attention :238-275     edge_attention :278-295

The reference scores one masked graph per forward and rebuilds each masked edge list on the host (a device sync per
atom). Here the complex is prepared once; per chunk of `bs` masks the leave-out batch is made on the GPU
(`pvs_mask_graph_build`: the disjoint union of `bs` copies of the complex, each without its masked atoms, filtered from
the parent's CSR without a sort), features and coordinates are gathered with one `index_select` each, and the model's
ordinary batched forward scores all copies. Nothing is copied to the host per atom: the scores of all chunks and the
builders' status words leave the device once, at the end.

PDB parsing, PLIP, PyMOL and `attribute()` itself are not part of this package.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .global_objects import DEVICE
from .graph import Data, PreparedGraph, prepare_graph
from .pnn_geometric_base import PNNGeometricBase

SIGMOID = False

# Edges of one leave-out batch: the largest batch the layer kernels are tested at (BASELINE config 2, 32 graphs of
# 2,000 atoms at 10 A: ~10.2 M edges), far inside int32. `bs` is lowered silently for graphs that would exceed it.
MAX_CHUNK_EDGES = 10_200_000


def to_numpy(x):
    return x.detach().cpu().numpy()


def chunk_size(bs, n_masks, n_nodes, n_edges, max_edges=MAX_CHUNK_EDGES):
    """Leave-out graphs per forward: `bs`, but no more than there are masks, than `max_edges` edges in the batch
    (bs * E, the builder's capacity) and than int32 node / edge ids allow; at least 1."""
    bs = int(bs)
    if bs < 1:
        raise ValueError(f'bs must be a positive number of graphs per forward, got {bs}')
    limit = min(int(max_edges), 2 ** 31 - 1)
    fit = min(limit // max(int(n_edges), 1), (2 ** 31 - 2) // max(int(n_nodes), 1))
    return max(1, min(bs, max(int(n_masks), 1), fit))


def bond_mask_table(edge_indices, edge_attrs):
    """Which edges `bond_masking` visits and what each visit leaves out: (visited [M] edge ids with
    edge_attrs[i, 1] != 0 in list order, drop [M, 2] = (min, max) of the edge's two atoms; -1 in the second slot of a
    self loop). numpy in, numpy out."""
    edge_indices, edge_attrs = np.asarray(edge_indices), np.asarray(edge_attrs)
    visited = np.nonzero(edge_attrs[:, 1] != 0)[0]
    a, b = edge_indices[0, visited], edge_indices[1, visited]
    drop = np.stack([np.minimum(a, b), np.maximum(a, b)], axis=1).astype(np.int32).reshape(-1, 2)
    drop[drop[:, 0] == drop[:, 1], 1] = -1
    return visited, drop


def masked_edge_counts(edge_indices, drop, n_nodes):
    """Edges each leave-out graph keeps (host arithmetic on the COO list, no device work): E less the edges that touch
    a dropped atom. edge_indices [2, E], drop [M, 2] (second slot -1: one atom). Returns int64 [M]."""
    ei = np.asarray(edge_indices).astype(np.int64)
    drop = np.asarray(drop).astype(np.int64).reshape(-1, 2)
    a, b = ei[0], ei[1]
    loops = a == b
    touch = (np.bincount(a, minlength=n_nodes) + np.bincount(b, minlength=n_nodes)
             - np.bincount(a[loops], minlength=n_nodes))
    lost = touch[drop[:, 0]].copy()
    two = (drop[:, 1] >= 0) & (drop[:, 1] != drop[:, 0])
    if two.any():
        lo, hi = np.minimum(a, b)[~loops], np.maximum(a, b)[~loops]
        keys, counts = np.unique(lo * n_nodes + hi, return_counts=True)      # edges between each unordered pair
        want = np.minimum(drop[two, 0], drop[two, 1]) * n_nodes + np.maximum(drop[two, 0], drop[two, 1])
        at = np.searchsorted(keys, want)
        at_ok = np.minimum(at, max(len(keys) - 1, 0))
        both = np.where((at < len(keys)) & (keys[at_ok] == want), counts[at_ok], 0) if len(keys) else 0
        lost[two] += touch[drop[two, 1]] - both
    return ei.shape[1] - lost


def couples_graphs(model):
    """True for a model whose output for one graph depends on the other graphs of its batch: the reference's GraphNorm
    takes its mean and variance over ALL nodes of a batch (it is called without the batch vector, egnn_satorras.py:166),
    so leave-out copies scored together would normalise each other. Such a model is scored one copy per forward (the
    copies are still made on the GPU; nothing is rebuilt on the host)."""
    return any(getattr(layer, 'graphnorm', False) for layer in model.layers)


class MaskBatch:
    """One leave-out batch on the device: `.prepared` (PreparedGraph of the union), `.src_node` (int64 [total_nodes]:
    the parent node of each output node), `.graph_ptr` / `.graph_eptr` (int32 [B + 1]), `.status` (int32 [1])."""

    def __init__(self, prepared, src_node, graph_ptr, graph_eptr, status, n_graphs):
        self.prepared, self.src_node, self.graph_ptr, self.graph_eptr = prepared, src_node, graph_ptr, graph_eptr
        self.status, self.n_graphs = status, n_graphs

    def check_status(self):
        raise_for_status(int(self.status.item()))


def raise_for_status(code):
    if code & 1:
        raise IndexError('mask table contains node ids outside [0, n_nodes)')
    if code & 4:
        raise RuntimeError('leave-out batch: more edges than the buffers hold')
    if code & (8 | 16):
        raise RuntimeError('leave-out batch: the node or edge count worked out on the host does not match the graph '
                           '(was the edge list changed after the graph was prepared?)')


def build_mask_batch(parent, drop, n_edges=None):
    """The leave-out batch of `parent` (a PreparedGraph of ONE complex) for the mask table `drop` (host int array
    [B, 2]; second slot -1 for a single atom). n_edges: the surviving edge count when the caller has worked it out
    (`masked_edge_counts`): the result then is an ordinary graph every layer accepts. None: the arrays get room for
    B * E edges and the count stays on the device (`PvsGraph.n_edges_dev`, like the screening builder's graphs).
    No host synchronisation; call `.check_status()` where one is fine."""
    lib = _lib.lib()
    drop_host = torch.as_tensor(np.asarray(drop), dtype=torch.int32).reshape(-1, 2).contiguous()
    n_masks = int(drop_host.shape[0])
    if n_masks < 1:
        raise ValueError('empty mask table')
    n, e = parent.n_nodes, parent.n_edges
    single = (drop_host[:, 1] < 0) | (drop_host[:, 1] == drop_host[:, 0])
    total_nodes = n_masks * n - int((2 - single.long()).sum())
    if total_nodes < 0 or n_masks * n >= 2 ** 31 - 1 or n_masks * e >= 2 ** 31:
        raise ValueError(f'{n_masks} leave-out copies of a graph with {n} nodes / {e} edges do not fit int32')
    dev = parent.t['rowptr'].device
    capacity = n_masks * e if n_edges is None else int(n_edges)
    i32 = dict(dtype=torch.int32, device=dev)
    e_alloc, n_alloc = max(capacity, 1), max(total_nodes, 1)
    t = {'rowptr': torch.empty(total_nodes + 1, **i32), 'row': torch.empty(e_alloc, **i32),
         'col': torch.empty(e_alloc, **i32), 'inv_deg': torch.empty(n_alloc, dtype=torch.float32, device=dev),
         'status': torch.empty(1, **i32), 'graph_eptr': torch.empty(n_masks + 1, **i32)}
    if parent.n_edge_attr:
        t['etype'] = torch.empty(e_alloc, dtype=torch.uint8, device=dev)
    src_node, graph_ptr = torch.empty(n_alloc, **i32), torch.empty(n_masks + 1, **i32)
    drop_dev = drop_host.to(dev, non_blocking=True)
    ws_bytes = lib.pvs_mask_graph_workspace_bytes(n, n_masks)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    _lib.check(lib.pvs_mask_graph_build(
        C.byref(parent.c), _lib.ptr(drop_dev), n_masks, total_nodes, capacity, 0 if n_edges is None else 1,
        _lib.ptr(t['rowptr']), _lib.ptr(t['row']), _lib.ptr(t['col']), _lib.ptr(t.get('etype')),
        _lib.ptr(t['inv_deg']), _lib.ptr(src_node), _lib.ptr(graph_ptr), _lib.ptr(t['graph_eptr']),
        _lib.ptr(t['status']), _lib.ptr(ws), ws_bytes, _lib.stream(dev)), 'pvs_mask_graph_build')
    t['_inputs'] = (drop_dev, ws, parent)        # alive until the kernels have run
    pg = PreparedGraph.over_buffers(total_nodes, capacity, t, t['rowptr'][total_nodes:] if n_edges is None else None,
                                    parent.n_edge_attr)
    pg.c.graph_eptr, pg.c.n_graphs = _lib.ptr(t['graph_eptr']), n_masks
    return MaskBatch(pg, src_node[:total_nodes].long(), graph_ptr, t['graph_eptr'], t['status'], n_masks)


def _single_graph(model, p, v, edge_indices, edge_attrs):
    """(x [n, d], pos [n, 3], edge_index, edge_attr) on the model's device and dtype, as the reference's
    get_pyg_single_graph_for_inference(Data(x=v.squeeze(), ...)) hands them to the model."""
    if edge_indices is None:
        raise ValueError('the geometric models need edge_indices ([2, E] COO)')
    dtype = model._model_dtype()
    x = v.reshape(-1, v.shape[-1]).to(DEVICE, dtype)
    pos = p.reshape(-1, 3).to(DEVICE, dtype)
    if x.shape[0] != pos.shape[0]:
        raise ValueError(f'p has {pos.shape[0]} atoms but v has {x.shape[0]}')
    edge_indices = torch.as_tensor(edge_indices)
    if edge_indices.dim() != 2 or edge_indices.shape[0] != 2:
        raise ValueError(f'edge_indices must be [2, E], got {tuple(edge_indices.shape)}')
    if edge_attrs is not None:
        edge_attrs = torch.as_tensor(edge_attrs)
        if edge_attrs.dim() != 2 or edge_attrs.shape[0] != edge_indices.shape[1]:
            raise ValueError(f'edge_attrs must be [E, A] with E = {edge_indices.shape[1]}, '
                             f'got {tuple(edge_attrs.shape)}')
    return x, pos, edge_indices, edge_attrs


def _whole_graph(x, pos, edge_indices, edge_attrs, prepared=None):
    n = x.shape[0]
    g = Data(x=x, pos=pos, edge_index=edge_indices.to(DEVICE).long(),
             edge_attr=None if edge_attrs is None else edge_attrs.to(DEVICE),
             batch=torch.zeros(n, dtype=torch.long, device=x.device), num_graphs=1,
             ptr=torch.tensor([0, n], dtype=torch.long))
    if prepared is not None:
        g.prepared = prepared
    return g


class _Eval:
    """eval mode (no dropout) and no autograd for the duration; the model's mode is restored."""

    def __init__(self, model):
        self.model, self.grad = model, torch.no_grad()

    def __enter__(self):
        self.was_training = self.model.training
        self.model.eval()
        self.grad.__enter__()

    def __exit__(self, *exc):
        self.grad.__exit__(*exc)
        self.model.train(self.was_training)


def segments_refusal(model):
    """Why the model's GraphNorm layers cannot normalise per node segment (fp64, more than 128 channels): a string, or
    None. Autograd is not looked at: the callers run under no_grad."""
    with torch.no_grad():
        for layer in model.layers:
            if getattr(layer, 'graphnorm', False):
                why = layer.norm_segments_refusal()
                if why is not None:
                    return why
    return None


def masked_outputs(model, p, v, drop, bs=32, edge_indices=None, edge_attrs=None, per_graph_norm=False):
    """Raw model outputs of the unmasked complex and of every leave-out graph of the mask table `drop` (host int
    [M, 2], second slot -1: one atom): (original as the model returns it for one graph, masked [M, dim_output]), both
    device tensors in the model's dtype. This is what atom_masking / bond_masking reduce to scores.
    per_graph_norm (default False): a model with GraphNorm (`couples_graphs`) is scored `chunk_size(...)` copies per
    forward like any other model, every copy normalised by its own statistics (PreparedGraph.set_norm_segments on the
    leave-out batch: the values of one copy per forward). Where the layers cannot take segments (fp64, more than 128
    channels) the call keeps one copy per forward. Nothing changes for a model without GraphNorm."""
    if not isinstance(model, PNNGeometricBase):
        raise TypeError('pointvs_amd.attribution scores the geometric (EGNN) models only')
    x, pos, edge_indices, edge_attrs = _single_graph(model, p, v, edge_indices, edge_attrs)
    n = int(x.shape[0])
    drop = np.asarray(drop, dtype=np.int64).reshape(-1, 2)
    ei_host = to_numpy(edge_indices).astype(np.int64)
    if ei_host.size and (ei_host.min() < 0 or ei_host.max() >= n):
        raise IndexError('edge_indices contains node ids outside [0, n_nodes)')
    if drop.size and (drop[:, 0].min() < 0 or drop.max() >= n or drop[:, 1].min() < -1):
        raise IndexError('mask table contains node ids outside [0, n_nodes)')
    counts = masked_edge_counts(ei_host, drop, n)
    with _Eval(model):
        parent = prepare_graph(edge_indices.to(DEVICE).long(), None if edge_attrs is None else edge_attrs.to(DEVICE),
                               n, need_backward=False)
        parent.check_status()
        original = model(_whole_graph(x, pos, edge_indices, edge_attrs, prepared=parent))
        step = chunk_size(bs, len(drop), n, parent.n_edges)
        segments = bool(per_graph_norm) and couples_graphs(model) and segments_refusal(model) is None
        if couples_graphs(model) and not segments:
            step = 1
        outs, status = [], []
        for k in range(0, len(drop), step):
            mb = build_mask_batch(parent, drop[k:k + step], n_edges=int(counts[k:k + step].sum()))
            if segments:
                mb.prepared.set_norm_segments(mb.graph_ptr)
            total = mb.prepared.n_nodes
            batch = torch.searchsorted(mb.graph_ptr[1:].long(), torch.arange(total, device=x.device), right=True)
            g = Data(x=x.index_select(0, mb.src_node), pos=pos.index_select(0, mb.src_node), batch=batch,
                     ptr=mb.graph_ptr, num_graphs=mb.n_graphs, prepared=mb.prepared)
            outs.append(model(g).reshape(mb.n_graphs, -1))
            status.append(mb.status)
        if outs:
            raise_for_status(int(np.bitwise_or.reduce(to_numpy(torch.cat(status)))))
            masked = torch.cat(outs, 0)
        else:
            masked = original.new_empty((0, original.numel()))
    return original, masked


def _atom_scores(original, masked, sigmoid):
    """original: the model's output for the unmasked graph (numpy, as returned), masked [M, k]. The reference's
    arithmetic (:389-431): three outputs in a 2-D array are a multitask regression and are averaged; otherwise the
    output must be one number (the reference's float() raises for more, and so does this)."""
    if original.ndim == 2 and original.shape[1] == 3:
        return np.asarray(np.mean(original.squeeze()) - masked.mean(axis=1), dtype=np.float64)
    if original.size != 1 or (masked.size and masked.shape[1] != 1):
        raise TypeError('only length-1 arrays can be converted to Python scalars: atom_masking needs a model with one '
                        'output per graph (or a [1, 3] multitask regression output)')
    return float(original.reshape(())) - masked[:, 0].astype(np.float64)


def _bond_scores(original, masked):
    """Output 1 of several, or the single output of a one-output model (:42-48)."""
    original = original.reshape(-1)
    pick = 1 if original.size > 1 else 0
    return float(original[pick]) - masked[:, pick].astype(np.float64)


def atom_masking(model, p, v, m=None, bs=32, edge_indices=None, edge_attrs=None, resis=None, **kwargs):
    """Score change when each atom is removed: original - masked, numpy float64 [n_atoms].

    p [1, n, 3] positions, v [1, n, d] features, edge_indices [2, E] COO, edge_attrs [E, 3] one-hot. bs: leave-out
    graphs per forward (the reference ignores it for the EGNN models and runs one graph per forward; a model with
    graphnorm is scored one graph per forward here too - couples_graphs - unless per_graph_norm=True: then `bs` copies
    per forward, each normalised by its own statistics, masked_outputs). m and resis are
    accepted for the reference's signature and unused, as there. With SIGMOID the scores are differences of sigmoids."""
    if kwargs.get('synthpharm', False):
        p, v = p.reshape(1, *p.shape), v.reshape(1, *v.shape)
    n_atoms = int(p.shape[-2])
    drop = np.stack([np.arange(n_atoms), np.full(n_atoms, -1)], axis=1)
    original, masked = masked_outputs(model, p, v, drop, bs, edge_indices, edge_attrs,
                                      per_graph_norm=kwargs.get('per_graph_norm', False))
    regression = original.dim() == 2 and original.shape[1] == 3
    if SIGMOID and not regression:
        original, masked = torch.sigmoid(original), torch.sigmoid(masked)
    return _atom_scores(to_numpy(original), to_numpy(masked), SIGMOID)


def bond_masking(model, p, v, m=None, bs=32, edge_indices=None, edge_attrs=None, **kwargs):
    """Score change when the two atoms of each ligand-receptor contact are removed: numpy float64 [E], original -
    masked for the edges with edge_attrs[i, 1] != 0 and 0 for the others.

    A model with several outputs is scored by output 1, as in the reference. For a SINGLE-output model the reference
    raises (`len()` of a 0-d array); here the one output is the score. A type-1 self loop (which generate_edges never
    emits) removes its one atom. bs: leave-out graphs per forward. per_graph_norm: as in atom_masking."""
    if edge_indices is None or edge_attrs is None:
        raise ValueError('bond_masking needs edge_indices and edge_attrs')
    ei, ea = to_numpy(torch.as_tensor(edge_indices)), to_numpy(torch.as_tensor(edge_attrs))
    if ea.ndim != 2 or ea.shape[0] != ei.shape[1] or ea.shape[1] < 2:
        raise ValueError(f'edge_attrs must be [E, A >= 2] with E = {ei.shape[1]}, got {ea.shape}')
    visited, drop = bond_mask_table(ei, ea)
    original, masked = masked_outputs(model, p, v, drop, bs, edge_indices, edge_attrs,
                                      per_graph_norm=kwargs.get('per_graph_norm', False))
    if SIGMOID:
        original, masked = torch.sigmoid(original), torch.sigmoid(masked)
    scores = np.zeros(ei.shape[1], dtype=np.float64)
    scores[visited] = _bond_scores(to_numpy(original), to_numpy(masked))
    return scores


def _forward_whole(model, p, v, edge_indices, edge_attrs):
    x, pos, edge_indices, edge_attrs = _single_graph(model, p, v, edge_indices, edge_attrs)
    graph = _whole_graph(x, pos, edge_indices, edge_attrs)
    with _Eval(model):
        model(graph)
    return graph


def cam(model, p, v, m=None, edge_indices=None, edge_attrs=None, **kwargs):
    """Class activation mapping (:298-353): the head applied to every node's final embedding, numpy [n] (three
    outputs per node are averaged)."""
    x, pos, edge_indices, edge_attrs = _single_graph(model, p, v, edge_indices, edge_attrs)
    feats, edges, coords, edge_attributes, batch = model.unpack_graph(_whole_graph(x, pos, edge_indices, edge_attrs))
    with _Eval(model):
        feats, _ = model.get_embeddings(feats, edges, coords, edge_attributes, batch)
        out = to_numpy(model._run_head(model.feats_linear_layers, feats))
    if out.ndim == 2 and out.shape[1] == 3:
        out = np.mean(out, axis=1)
    return np.array(out)


def node_attention(model, p, v, edge_indices=None, edge_attrs=None, gnn_layer=-1, **kwargs):
    """Node attention weights of layer `gnn_layer` after one forward (:238-275), numpy [n]; logits with SIGMOID."""
    _forward_whole(model, p, v, edge_indices, edge_attrs)
    att = model.layers[gnn_layer].node_att_val.reshape((-1,))
    return np.log(att / (1 - att)) if SIGMOID else att


def edge_attention(model, p, v, edge_indices=None, edge_attrs=None, gnn_layer=-1, **kwargs):
    """Edge attention weights of layer `gnn_layer` after one forward (:278-295), numpy [E] in input edge order."""
    _forward_whole(model, p, v, edge_indices, edge_attrs)
    return model.layers[gnn_layer].att_val.reshape((-1,))
