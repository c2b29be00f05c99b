"""Data-root scoring through one captured step: complex batches at fixed capacities.

`PygPointCloudDataset.build_batch` asks the host twice per batch (node counts, edge offsets), allocates every table at a
data-dependent size and writes the int64 edge list that the model's forward then sorts back into the CSR the radius-graph
builder had already made. Scoring a types file needs none of that: `FixedShapeScorer` owns static buffers at host-chosen
capacities, `pvs_complex_batch_build_cap` + `pvs_radius_graph_build_cap` (csrc/complex_build.hip, radius_graph.hip) fill
them from a static `pairs` table without a host round trip, and the layers, GraphNorm, pooling and heads read the
batch's sizes where the builders left them on the device (`PvsGraph.n_edges_dev`, `n_norm_rows_dev`, `node_ptr`). No
host argument of the step depends on the batch, so one hipGraph serves every full batch of the file.

`score_batches` is the loop `PointNeuralNetworkBase.val(capture=True)` runs: the first batches eagerly (they size the
capacities), every further full batch as one `load` + one replay, its scores handed on one batch late - once its status
word has arrived - and rebuilt by the eager route where a capacity was too small.
"""
import collections
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from .nowait import LateQueue, StagingRing, capture_fixed_step, pinned
from .parquet_data import MAX_LIGAND_ATOMS, _raise_for_status

Capacities = collections.namedtuple('Capacities', 'node_cap graph_node_cap edge_cap atoms_in_cap')

# the builders' status bits that say "a capacity was too small": such a batch is scored by the eager route instead
OVERFLOW_BITS = _lib.CAP_NODE_OVERFLOW | _lib.CAP_GRAPH_OVERFLOW | _lib.CAP_EDGE_OVERFLOW
CAP_STATUS_TEXT = (
    (_lib.CAP_NODE_OVERFLOW, 'more nodes than the fixed-shape buffers hold (node_cap)'),
    (_lib.CAP_GRAPH_OVERFLOW, 'a complex of more nodes than the fixed-shape mask state holds (graph_node_cap)'),
    (_lib.CAP_EDGE_OVERFLOW, 'more edges than the fixed-shape buffers hold (edge_cap)'),
    (_lib.CAP_EMPTY_SAMPLE, 'a sample has no atom left after the hydrogen filter'),
)
MAX_GRAPH_NODE_CAP = 4096 + MAX_LIGAND_ATOMS     # a cropped receptor of 4,096 atoms and the largest ligand the builder takes
PROBE_BATCHES, HEADROOM = 4, 1.5


def _round_up(value, to):
    return -(-int(value) // to) * to


def plan_capacities(observed, atoms_in_cap, headroom=HEADROOM, batch_size=None):
    """Capacities of the fixed-shape buffers from what the probe batches held. observed: (nodes, nodes of the largest
    graph, edges[, edges of the largest graph]) of every probe batch; atoms_in_cap: the most input atoms of any batch
    (`batch_input_atoms`, exact). Largest value times `headroom`, rounded up to multiples of 64 / 64 / 1024. With
    batch_size (and the fourth entry) the batch totals count as no less than batch_size copies of the largest complex
    seen: a types file lists a receptor's poses together, so later batches can consist of the largest one alone.
    graph_node_cap sizes the neighbour-mask state (node_cap * graph_node_cap / 32 bytes) and stops at
    MAX_GRAPH_NODE_CAP; a probe graph above that is refused. Pure host arithmetic."""
    observed = [tuple(int(v) for v in o) for o in observed]
    if not observed:
        raise ValueError('plan_capacities needs at least one probe batch')
    if headroom < 1:
        raise ValueError(f'headroom {headroom} < 1: the probe batches themselves would not fit')
    nodes, graph_nodes, edges = (max(o[k] for o in observed) for k in range(3))
    if batch_size is not None:
        graph_edges = max((o[3] for o in observed if len(o) > 3), default=0)
        nodes = max(nodes, int(batch_size) * graph_nodes)
        edges = max(edges, int(batch_size) * graph_edges)
    if graph_nodes > MAX_GRAPH_NODE_CAP:
        raise ValueError(f'a complex of {graph_nodes} nodes: the fixed-shape builder takes graphs of up to '
                         f'{MAX_GRAPH_NODE_CAP} (score this file without capture)')
    node_cap = _round_up(max(math.ceil(nodes * headroom), 1), 64)
    graph_node_cap = min(_round_up(max(math.ceil(graph_nodes * headroom), 1), 64), MAX_GRAPH_NODE_CAP)
    edge_cap = _round_up(max(math.ceil(edges * headroom), 1), 1024)
    if edge_cap >= 2 ** 31 or node_cap >= 2 ** 31 - 1:
        raise ValueError(f'{node_cap} nodes / {edge_cap} edges do not fit int32: use a smaller batch size')
    return Capacities(node_cap, graph_node_cap, edge_cap, int(atoms_in_cap))


def batch_input_atoms(dataset, batches):
    """The most input atoms (ligand + whole receptor, before the crop) of any of `batches` (lists of sample indices):
    the host knows every file's atom count, so this capacity is exact."""
    rec_n, lig_n = np.diff(dataset.rec_pool['ptr']), np.diff(dataset.lig_pool['ptr'])
    most = 0
    for indices in batches:
        indices = np.asarray(list(indices), dtype=np.int64)
        most = max(most, int(rec_n[dataset.rec_ids[indices]].sum() + lig_n[dataset.lig_ids[indices]].sum()))
    return most


def observed_sizes(batch):
    """(nodes, nodes of the largest graph, edges, edges of the largest graph) of a batch `build_batch` made: one entry
    of plan_capacities' input."""
    return (sum(batch.graph_node_counts), max(batch.graph_node_counts), sum(batch.graph_edge_counts),
            max(batch.graph_edge_counts))


def raise_for_status(code):
    """The loader's ValueError for the bits it names, extended by the capacity builders' bits."""
    if code & ~(OVERFLOW_BITS | _lib.CAP_EMPTY_SAMPLE):
        _raise_for_status(code & ~(OVERFLOW_BITS | _lib.CAP_EMPTY_SAMPLE))
    if code:
        raise ValueError('complex batch: ' + '; '.join(text for bit, text in CAP_STATUS_TEXT if code & bit))


def _kernel_width(hidden):
    """The width a layer of `hidden` channels runs at (EGNNLayer._KERNEL_WIDTHS: zero-padded to the next one)."""
    return next((w for w in (16, 32, 64, 128) if w >= hidden), None)


def model_refusal(model):
    """Why no step that leaves its edge count on the device can run `model`, or None: the model's part of `refusal`,
    which the cropped library screen asks as well. Host checks only."""
    if any(p.dtype == torch.float64 for p in model.parameters()):
        return 'fp64 models (no fp64 layer takes a device-side edge count): score them without capture'
    layers = list(model.layers)[1:]
    if not layers:
        return 'a model without EGNN layers'
    for layer in layers:
        if getattr(layer, 'edge_residual', False):
            return ('edge_residual=True: the edge messages travel between layers, and a layer that returns them needs a '
                    'host-known edge count')
        width = _kernel_width(layer.hidden_nf)
        if (width not in (32, 64, 128) or os.environ.get('PVS_EGNN_KERNELS', '')[:1] == 'g'
                or (layer.hidden_nf > 64 and os.environ.get('PVS_WIDE') == 'decomposed')):
            return (f'hidden size {layer.hidden_nf} runs on the generic edge kernels, which need a host-known edge count '
                    '(the MFMA kernels cover 17..128 channels)')
    return None


def refusal(model, dataset):
    """Why the fixed-shape step cannot score `dataset` with `model`, or None. Host checks only."""
    why = model_refusal(model)
    if why is not None:
        return why
    if getattr(dataset, 'rot', False):
        return 'a dataset with rot=True (scoring loaders do not rotate)'
    if len(dataset) and dataset.is_augmented(len(dataset) - 1):
        return 'a dataset with augmented actives (scoring loaders have none)'
    if dataset.edge_radius is not None and dataset.edge_radius < 0:
        return 'edge_radius < 0 (no edge list) is not built on the data-root path'
    return None


class FixedShapeScorer:
    """scores = FixedShapeScorer(model, dataset, batch_size, capacities)(indices)      # [batch_size, ...] raw outputs

    The eager fixed-shape step on `batch_size` samples of a `PygPointCloudDataset`: the capacity builders, the model's
    layers on the one PreparedGraph over node_cap rows (per-layer `forward_prepared`, edge count and GraphNorm's row count
    on the device), pooling and the model's current task head by the device node offsets; eval mode, no autograd, the
    sigmoid left to the caller. `capture()` records that step once; `replay(indices)` loads another composition - any
    `batch_size` indices, repeats allowed - and replays it; `check()` raises for the status word of an earlier step, one
    step late, as the screens do. capacities: a `Capacities`, or None for a probe of the first PROBE_BATCHES batches
    in index order through `build_batch`. Lives as long as the weights' addresses do (pointers are not tracked).

    A scorer is eager or captured, never both: `capture()` is refused once the scorer has run a step of its own, and a
    captured scorer takes `replay()` only. The launches of a captured scorer are therefore capture's two warm-up steps
    and its replays, which is the sequence `val(capture=True)` runs. (Capturing on a scorer that had run some hundred
    eager steps, then replaying it synchronously, once did not return on an MI355X, and the cause was not found; the
    eager reference of a captured scorer is a second scorer of the same capacities, whose bits are the same.)"""

    RING = 2      # status words / pairs tables in flight: the step just launched and the one before it

    def __init__(self, model, dataset, batch_size, capacities=None, device=None):
        from .global_objects import DEVICE
        why = refusal(model, dataset)
        if why is not None:
            raise NotImplementedError(f'FixedShapeScorer: {why}')
        dev = torch.device(device or dataset.device or DEVICE)
        if dev.type != 'cuda':
            raise RuntimeError('complex batches are built by HIP kernels on a GPU; there is no CPU path')
        if dev.index is None:
            dev = torch.device('cuda', torch.cuda.current_device())
        self.model, self.dataset, self.device, self.b = model, dataset, dev, int(batch_size)
        if self.b < 1:
            raise ValueError('batch_size must be positive')
        if capacities is None:
            capacities = self._probe()
        self.capacities = cap = Capacities(*(int(v) for v in capacities))
        if cap.graph_node_cap > MAX_GRAPH_NODE_CAP or min(cap.node_cap, cap.graph_node_cap, cap.edge_cap) < 1:
            raise ValueError(f'{cap}: capacities must be positive, graph_node_cap at most {MAX_GRAPH_NODE_CAP}')
        layers = list(model.layers)
        self.embed, self.egnn = layers[0], layers[1:]
        self.graphnorm = any(getattr(layer, 'graphnorm', False) for layer in self.egnn)
        from .screening import _resolve_tasks
        tasks = _resolve_tasks(model, None)
        self.head = model.feats_linear_layers if tasks is None else model.task_heads(tasks)[0]
        edge_radius = dataset.edge_radius if dataset.edge_radius and dataset.edge_radius > 0 else 4
        self.r_inter, self.r_intra = float(edge_radius), 2.0 if dataset.estimate_bonds else float(edge_radius)
        self._buffers()
        self._graph, self._static_out = None, None
        self._late = LateQueue(ring=self.RING)      # the steps' status words, oldest first
        self._launched = 0                          # steps of its own so far: capture() wants none

    def _probe(self):
        n, batches = len(self.dataset), []
        for k in range(0, n, self.b):
            batches.append(list(range(k, min(k + self.b, n))))
        observed = [observed_sizes(self.dataset.build_batch(indices, device=self.device))
                    for indices in batches[:PROBE_BATCHES]]
        return plan_capacities(observed, batch_input_atoms(self.dataset, batches), batch_size=self.b)

    def _buffers(self):
        lib, dev, cap, ds = _lib.lib(), self.device, self.capacities, self.dataset
        i32, f32 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.float32, device=dev)
        u8 = dict(dtype=torch.uint8, device=dev)
        self.pool_t, self.pool_c = ds._pool_on(dev)
        ws_bytes = lib.pvs_complex_batch_workspace_bytes(self.b, cap.atoms_in_cap)
        st_bytes = lib.pvs_radius_graph_state_bytes(cap.node_cap, self.b, cap.graph_node_cap)
        self.t = t = dict(
            pairs=torch.zeros((self.b, 3), **i32), counts=torch.zeros((self.b, 2), **i32),
            node_ptr=torch.zeros(self.b + 1, **i32), x=torch.zeros((cap.node_cap, ds.feature_dim), **f32),
            pos=torch.zeros((cap.node_cap, 3), **f32), bp=torch.zeros(cap.node_cap, **u8),
            node_graph=torch.full((cap.node_cap,), -1, **i32), rowptr=torch.zeros(cap.node_cap + 1, **i32),
            row=torch.zeros(cap.edge_cap, **i32), col=torch.zeros(cap.edge_cap, **i32),
            etype=torch.zeros(cap.edge_cap, **u8), inv_deg=torch.ones(cap.node_cap, **f32),
            n_edges_fwd=torch.zeros(1, **i32), status=torch.zeros(1, **i32), workspace=torch.empty(ws_bytes, **u8), state=torch.empty(st_bytes, **u8))
        self._stage = StagingRing(self.RING, lambda: pinned((self.b, 3), torch.int32))
        from .graph import PreparedGraph
        # (the builders' own status word is read through check() / take_status(); the edge count is not
        # rowptr[node_cap]: on an edge overflow that is the true count, beside row / col / etype of an earlier batch)
        pg = PreparedGraph.over_buffers(
            cap.node_cap, cap.edge_cap, {k: t[k] for k in ('rowptr', 'row', 'col', 'etype', 'inv_deg', 'status')},
            t['n_edges_fwd'])
        if self.graphnorm:
            pg.set_norm_rows(t['node_ptr'][self.b:])
        self.pg = pg

    # ---- loading a batch ----
    def load(self, indices):
        """Rewrites the static `pairs` table for `batch_size` sample indices: an asynchronous copy from pinned staging
        (a staging buffer is not rewritten while the copy that reads it may be pending)."""
        ds = self.dataset
        indices = np.asarray([int(i) for i in indices], dtype=np.int64)
        if len(indices) != self.b:
            raise ValueError(f'FixedShapeScorer of batch size {self.b} was given {len(indices)} samples')
        if len(indices) and (indices.min() < 0 or indices.max() >= len(ds)):
            raise IndexError(f'sample index outside the dataset of {len(ds)}')
        rec_id, lig_id = ds.rec_ids[indices], ds.lig_ids[indices]
        n_in = (np.diff(ds.rec_pool['ptr'])[rec_id] + np.diff(ds.lig_pool['ptr'])[lig_id]).astype(np.int64)
        flag_off = np.concatenate([[0], np.cumsum(n_in)])
        if int(flag_off[-1]) > self.capacities.atoms_in_cap:
            raise ValueError(f'the batch has {int(flag_off[-1])} input atoms, the scorer was built for '
                             f'{self.capacities.atoms_in_cap} (atoms_in_cap)')
        host = self._stage.acquire()
        host.copy_(torch.from_numpy(np.stack([rec_id, lig_id, flag_off[:-1]], axis=1).astype(np.int32)))
        self.t['pairs'].copy_(host, non_blocking=True)
        self._stage.release(self.device)
        self.indices = [int(i) for i in indices]

    # ---- the step ----
    def build(self):
        """The two capacity builders on the loaded `pairs`, into the static buffers."""
        lib, t, cap, ds = _lib.lib(), self.t, self.capacities, self.dataset
        stream = _lib.stream(self.device)
        _lib.check(lib.pvs_complex_batch_build_cap(
            C.byref(self.pool_c), _lib.ptr(t['pairs']), None, None, self.b, cap.atoms_in_cap, cap.node_cap,
            float(ds.radius), 1 if ds.polar_hydrogens else 0, 1 if ds.use_atomic_numbers else 0, ds.n_features,
            1 if ds.compact else 0, _lib.ptr(self.pool_t['class_of_z']), _lib.ptr(t['counts']), _lib.ptr(t['node_ptr']),
            _lib.ptr(t['x']), _lib.ptr(t['pos']), None, _lib.ptr(t['bp']), _lib.ptr(t['node_graph']),
            _lib.ptr(t['status']), _lib.ptr(t['workspace']), t['workspace'].numel(), stream),
            'pvs_complex_batch_build_cap')
        _lib.check(lib.pvs_radius_graph_build_cap(
            _lib.ptr(t['pos']), _lib.ptr(t['bp']), _lib.ptr(t['node_ptr']), self.b, cap.node_cap, cap.graph_node_cap,
            self.r_inter, self.r_intra, 0, cap.edge_cap, _lib.ptr(t['rowptr']), _lib.ptr(t['row']), _lib.ptr(t['col']),
            _lib.ptr(t['etype']), _lib.ptr(t['inv_deg']), _lib.ptr(t['n_edges_fwd']), _lib.ptr(t['status']), 0,
            _lib.ptr(t['state']), t['state'].numel(), stream), 'pvs_radius_graph_build_cap')

    def _step(self):
        model, t = self.model, self.t
        self.build()
        x = t['pos']
        h = self.embed.embed(t['x'], x).contiguous()
        for layer in self.egnn:
            h, x, _ = layer.forward_prepared(self.pg, h, x, None, need_m=False, need_coords=layer is not self.egnn[-1])
        if self.head is None:
            return h
        return model._pool_and_head_padded(self.head, h, t['node_ptr'], self.b)

    def __call__(self, indices=None):
        if self._graph is not None:
            raise RuntimeError('FixedShapeScorer: a captured scorer takes replay() only (see the class docstring); '
                               'make a second scorer of the same capacities for eager steps')
        return self._run(indices)

    @torch.no_grad()
    def _run(self, indices=None):
        if indices is not None:
            self.load(indices)
        was_training = self.model.training
        self.model.eval()
        try:
            y = self._step()
        finally:
            self.model.train(was_training)
        if not torch.cuda.is_current_stream_capturing():
            self._queue_status()
        return y

    # ---- the late status word ----
    def _queue_status(self):
        """Queues the copy of the step's status word into a pinned word of the ring; with RING words in flight the
        oldest is checked first (its word is the one about to be reused)."""
        if len(self._late) >= self.RING:
            raise_for_status(self.take_status())
        self._launched += 1
        self._late.put(self.t['status'])

    def take_status(self):
        """The status word of the oldest step not yet asked about (waits for that step only), or 0 when there is none."""
        taken = self._late.take()
        return 0 if taken is None else taken[0]

    def check(self):
        """Raises for the status words of the steps launched so far (call once more after the last batch)."""
        while len(self._late):
            raise_for_status(self.take_status())

    # ---- capture / replay ----
    def capture(self, indices=None):
        """Captures one whole step (builders + layers + pooling + head) in a hipGraph after two eager warm-up calls. Only
        on a scorer that has launched nothing yet (see the class docstring)."""
        if self._graph is not None or self._launched:
            raise RuntimeError('FixedShapeScorer.capture(): the scorer has already run steps of its own; capture on a '
                               'fresh scorer (see the class docstring)')
        if indices is not None:
            self.load(indices)

        def drain():      # (a capacity overflow of the warm-up batch is its replay's to report)
            while len(self._late):
                raise_for_status(self.take_status() & ~OVERFLOW_BITS)

        self._graph, self._static_out = capture_fixed_step(self._run, self.device, drain)
        return self

    def replay(self, indices=None, check=True):
        """Loads `indices` (None: what is loaded) and replays the captured step; returns the static output. check=True
        raises first for the step before, as the screens do; a caller that passes False reads every step's word itself
        (`take_status`, oldest first)."""
        if self._graph is None:
            raise RuntimeError('replay() before capture()')
        if check:
            self.check()
        if indices is not None:
            self.load(indices)
        self._graph.replay()
        self._queue_status()
        return self._static_out


def score_batches(batches, batch_size, eager, make_scorer, replayed, emit, probe_batches=PROBE_BATCHES):
    """The deferred-submission loop of `val(capture=True)`; pure host logic over four callables.

    batches: lists of sample indices, in file order. The first `probe_batches` (all, if fewer) go through
    `eager(indices) -> (payload, observed sizes)`; `make_scorer(observed of the probes, batches)` then gives the captured
    scorer (`replay(indices, check=False)` -> static scores, `take_status()` -> the oldest unread status word). Every
    further full batch is one replay; its scores are cloned, and `replayed(indices, scores) -> payload` is emitted only
    after the NEXT batch has been launched, when its status word is read: 0 emits it, capacity-overflow bits alone
    rebuild it through `eager`, any other bit raises the loader's ValueError. A short last batch takes `eager`.
    `emit(payload)` is called in file order. Returns {'eager', 'replayed', 'fallback'}: batches scored eagerly by
    plan, from a replay, and eagerly because their replay overflowed."""
    stats = dict(eager=0, replayed=0, fallback=0)
    batches = [list(b) for b in batches]
    n_probe = min(max(int(probe_batches), 1), len(batches))
    observed = []
    for indices in batches[:n_probe]:
        payload, sizes = eager(indices)
        observed.append(sizes)
        emit(payload)
        stats['eager'] += 1
    rest = batches[n_probe:]
    scorer = make_scorer(observed, batches) if any(len(b) == batch_size for b in rest) else None
    waiting = None       # (indices, cloned scores) of the replay whose status word has not been read yet

    def settle():
        nonlocal waiting
        if waiting is None:
            return
        (indices, scores), waiting = waiting, None
        code = scorer.take_status()
        if code == 0:
            emit(replayed(indices, scores))
            stats['replayed'] += 1
        elif code & ~OVERFLOW_BITS:
            raise_for_status(code)
        else:
            emit(eager(indices)[0])
            stats['fallback'] += 1

    for indices in rest:
        if len(indices) != batch_size:
            settle()
            emit(eager(indices)[0])
            stats['eager'] += 1
            continue
        scores = scorer.replay(indices, check=False).clone()
        launched = (indices, scores)
        settle()                  # the batch before this one: its word arrived while this one was being loaded
        waiting = launched
    settle()
    return stats
