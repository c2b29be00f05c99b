"""train_model(capture=True): whole training steps replayed from hipGraphs, one per batch that comes back."""
import collections
import contextlib
import itertools

import torch

from . import graph as pgraph
from .global_objects import DEVICE
from .optim import FusedClipSGD
from .pnn_geometric_base import batch_tables


# One captured step: the hipGraph and the loss it writes, and what the captured launches read and must outlive - the batch
# (its addresses stay unique), the draw's buffers, which every replay rewrites (model.last_dropout of the capture), and the
# batch's dropout plan (a plan replaced on the batch later stays alive here). draw, plan: None without dropout.
CapturedBatch = collections.namedtuple('CapturedBatch', 'graph loss batch draw plan')


class StepReplayer:
    """A context manager around the training loop; `step(batch)` takes the place of the eager step
    (model.training_step). A batch runs eagerly on its first visit (which also warms up whatever its shapes need), is
    captured - graph preparation, forward, loss, backward, clip + optimiser - and replayed on its second, replayed from
    then on; at most `max_graphs` batches are captured, the rest stay eager. Everything - eager steps too - runs on ONE
    side stream, remembered on the model: autograd's AccumulateGrad nodes remember the stream of their first backward,
    and a capture on another stream than earlier eager steps faults in hipStreamEndCapture (ROCm 7.2 / torch 2.10;
    bench.py --graph 1 does the same).
    For its lifetime the optimiser is in its capturable form (model.optimiser_capturable) and, with dropout > 0, the
    model draws into a fixed shape from keys written here (DropoutKeys.external). What changes from step to step - the
    scheduler's rates, the dropout key - is no part of a capture: step() has both written to device memory outside it
    (`push_hyperparameters`, `push_dropout_key`), before the capture and before every replay."""

    def __init__(self, model, max_graphs=64):
        if not torch.cuda.is_available():
            raise RuntimeError('train_model(capture=True) needs a GPU')
        if torch.distributed.is_available() and torch.distributed.is_initialized() and torch.distributed.get_world_size() > 1:
            raise NotImplementedError('train_model(capture=True) is single-process (the gradient exchange is not captured)')
        if not isinstance(model.optimiser, (torch.optim.Adam, FusedClipSGD)):
            raise TypeError(f'train_model(capture=True) replays FusedClipAdam, FusedClipSGD or torch.optim.Adam steps, '
                            f'not {type(model.optimiser).__name__}')
        self._push = getattr(model.optimiser, 'push_hyperparameters', None)
        if model.scheduler is not None and self._push is None:
            raise TypeError("train_model(capture=True) with a learning-rate scheduler needs one of the project's fused "
                            'optimisers (torch.optim.Adam bakes a float rate into the captured step)')
        if any(p.dtype == torch.float64 for p in model.parameters()):
            raise NotImplementedError('train_model(capture=True) is fp32 only (fp64 trains eagerly)')
        self._dropout = float(getattr(model, 'dropout_p', 0) or 0) > 0
        if self._dropout and any(getattr(m, 'graphnorm', False) for m in model.modules()):
            raise NotImplementedError('train_model(capture=True) does not cover edge dropout in a model with GraphNorm: a '
                                      'captured step draws into an edge list of fixed shape whose unused slots join '
                                      'padding nodes appended to the batch, and GraphNorm normalises over every row of the '
                                      'batch, so the padding rows would enter its statistics (dropout > 0 with GraphNorm '
                                      'trains eagerly; without GraphNorm it is captured)')
        self.model, self.max_graphs = model, max_graphs
        # one side stream per model, kept across calls (AccumulateGrad nodes remember the stream of their first backward)
        if getattr(model, '_capture_stream', None) is None:
            model._capture_stream = torch.cuda.Stream(DEVICE)
        self.stream = model._capture_stream
        self.seen, self.graphs = {}, {}
        self.stats = model.last_capture_stats = {'eager': 0, 'captured': 0, 'replayed': 0}

    def __enter__(self):
        with contextlib.ExitStack() as stack:
            stack.enter_context(self.model.optimiser_capturable(self.max_graphs))
            if self._dropout:
                # the static-shape draw for the replayer's lifetime (eager visits too: one arithmetic for every step of
                # the run), keyed from the model's device table, which step() rewrites before every step
                stack.enter_context(self.model.dropout_keys.external(self.model))
            # (last in, first out: leaving waits on the side stream first, then drops the graphs, then closes the windows)
            stack.callback(self.graphs.clear)
            stack.callback(lambda: torch.cuda.current_stream(DEVICE).wait_stream(self.stream))
            self._windows = stack.pop_all()
        return self

    def __exit__(self, *exc):
        self._windows.close()

    _batch_ids = itertools.count(1)

    @classmethod
    def _key(cls, graph, task):
        """A batch is 'the same batch again' when it is the same OBJECT with the same device tensors at the same
        versions: the object carries an id stamped on its first visit (a streaming loader that yields fresh batch
        objects whose tensors happen to reuse freed addresses is never taken for a second visit)."""
        try:
            bid = graph.__dict__.get('_pvs_batch_id')
            if bid is None:
                bid = graph.__dict__['_pvs_batch_id'] = next(cls._batch_ids)
        except AttributeError:
            return None
        key = [task, bid]
        for name in ('x', 'pos', 'edge_index', 'edge_attr', 'batch', 'y'):
            t = getattr(graph, name, None)
            if t is None:
                key.append(None)
                continue
            if not torch.is_tensor(t) or not t.is_cuda:
                return None                  # host tensors are copied to new device tensors every step: nothing to replay
            key.append((t.data_ptr(), t._version, tuple(t.shape)))
        return tuple(key)

    @staticmethod
    def _make_capturable(graph, model=None):
        """What the forward would otherwise derive from the batch vector with data-dependent ops (a bincount, a
        maximum read on the host): done once, outside any capture, and left on the batch object. With a model that
        draws its edge dropout into a fixed shape, the draw's plan as well (plan_static_dropout: its count of
        row <= col edges is the one host read of that path)."""
        if getattr(graph, 'batch', None) is None:
            return
        graph.num_graphs, graph.ptr = batch_tables(graph, graph.batch)
        if model is not None and model.training and getattr(model, 'static_dropout', None) \
                and float(getattr(model, 'dropout_p', 0) or 0) > 0:
            model.plan_static_dropout(graph)

    def step(self, graph):
        key = self._key(graph, self.model.model_task)
        hit = self.graphs.get(key) if key is not None else None
        # the key the eager step would draw with now (the model's own schedule: every step of the run advances it once, as
        # the eager loop does), into the device table the captured draw reads: on the replayer's stream, outside the
        # capture - as push_hyperparameters does for the rates
        drawn = (self.model.push_dropout_key(next(self.model.parameters()).device)
                 if self._dropout and self.model.training else None)
        if hit is not None:
            if self._push is not None:
                self._push()
            hit.graph.replay()
            self.stats['replayed'] += 1
            if hit.draw is not None and drawn is not None:      # the captured step's buffers, drawn with this step's key
                self.model.last_dropout = dict(hit.draw, seed=drawn[0], step=drawn[1])
            return hit.loss.clone()
        visits = self.seen.get(key, 0) if key is not None else 0
        if key is None or visits == 0 or len(self.graphs) >= self.max_graphs:
            if key is not None:
                self.seen[key] = visits + 1
                self._make_capturable(graph, self.model)
            self.stats['eager'] += 1
            return self.model.training_step(graph)
        # second visit: capture. The batch's CSR / CSC preparation is captured too (its tensors then live in the
        # graph's private pool: a cached PreparedGraph could be evicted and freed under the captured launches).
        cache_was, pgraph.CACHE_ENABLED = pgraph.CACHE_ENABLED, False
        try:
            self.stream.synchronize()
            if self._push is not None:
                self._push()                 # (outside the capture: what the replay just below runs at)
            hip_graph = torch.cuda.CUDAGraph()
            self.model.last_dropout = None
            with torch.cuda.graph(hip_graph, stream=self.stream):
                static_loss = self.model.training_step(graph)
        finally:
            pgraph.CACHE_ENABLED = cache_was
        self.graphs[key] = CapturedBatch(hip_graph, static_loss, graph,
                                         self.model.last_dropout if self._dropout else None,
                                         getattr(graph, '_pvs_static_dropout', None) if self._dropout else None)
        hip_graph.replay()
        self.stats['captured'] += 1
        return static_loss.clone()
