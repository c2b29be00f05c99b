"""How a device word reaches the host without a wait, how pinned staging is reused, how a fixed-shape step is captured.

No host loop of this package waits for the device. A kernel leaves a status word on the GPU; the host queues a copy of
it into pinned memory, records an event, and reads the word one call later, when it has long arrived (`LateCopy`, and
`LateQueue` for the words in flight). Inputs travel the other way through pinned staging that is not rewritten while the
copy that reads it may be pending (`StagingRing`). A step whose host arguments do not depend on the batch is recorded
once (`capture_fixed_step`) and replayed for every batch. Every site of the package goes through these four; the
optimiser's pointer-table ring (optim.py), graph.prefetch_graph's stream event and captured_step.StepReplayer, which
captures at a batch's second visit on one stream per model, follow protocols of their own.
"""
import torch


def pinned(shape, dtype):
    """Zeroed page-locked host memory: what a StagingRing's `make()` builds its slot from."""
    return torch.zeros(shape, dtype=dtype).pin_memory()


class LateCopy:
    """copy = LateCopy(src); ...; copy.ready(); value = copy.wait()

    Queues `src` into pinned memory on the current stream of src.device and records an event behind the copy. host: a
    pinned buffer to reuse (default: a fresh one of src's dtype and shape); keep: whatever must outlive the copy.
    `ready()` never blocks; `wait()` waits for this copy alone and returns the host tensor. A CPU `src` is taken at once
    (itself, or copied into `host`), has no event and is always ready."""

    def __init__(self, src, host=None, keep=None):
        self.keep, self.tag, self.event = keep, None, None
        if not src.is_cuda:
            self.host = src if host is None else host.copy_(src)
            return
        self.host = torch.empty(src.shape, dtype=src.dtype, pin_memory=True) if host is None else host
        self.host.copy_(src, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record(torch.cuda.current_stream(src.device))

    def ready(self):
        return self.event is None or self.event.query()

    def wait(self):
        if self.event is not None:
            self.event.synchronize()
        return self.host


class LateQueue:
    """The one-element words in flight, in launch order. `put(src, tag, keep)` queues a LateCopy and returns it;
    `take()` waits for the oldest and returns (value, tag), or None when nothing is pending; `take(entry)` does so for
    the given entry alone (None if it was handed out already); `landed()` yields (value, tag) of every entry that has
    arrived, without waiting. An entry leaves the queue before its value is handed out, so an error is raised once.

    ring=n: the queue owns n pinned int32 words, allocated here, and `put` on a full ring raises (the caller takes
    first). Without a ring every `put` allocates its own word."""

    def __init__(self, ring=None):
        self._entries = []
        # (a host without a GPU has nothing to pin for: its words are taken at once)
        self._free = None if ring is None else [torch.empty(1, dtype=torch.int32, pin_memory=torch.cuda.is_available())
                                                for _ in range(ring)]

    def __len__(self):
        return len(self._entries)

    def put(self, src, tag=None, keep=None):
        host = None
        if self._free is not None:
            if not self._free:
                raise RuntimeError('LateQueue: every word of the ring is in flight; take() before the next put()')
            host = self._free.pop(0)
        entry = LateCopy(src, host, keep)
        entry.tag = tag
        self._entries.append(entry)
        return entry

    def _hand_out(self, entry):
        self._entries.remove(entry)
        value = entry.wait().item()
        if self._free is not None:
            self._free.append(entry.host)
        return value, entry.tag

    def take(self, entry=None):
        if entry is None:
            entry = self._entries[0] if self._entries else None
        if entry is None or entry not in self._entries:
            return None
        return self._hand_out(entry)

    def landed(self):
        # all entries, not only the head: they can belong to different streams
        for entry in list(self._entries):
            if entry.ready():
                yield self._hand_out(entry)


class StagingRing:
    """`n` sets of pinned staging tensors, handed out in rotation; `make()` builds one set, at the first `acquire()`
    that needs it. `acquire()` waits for the event of the slot it hands out (the copy that read it last may still be
    pending); `release(device)` records that event on the current stream of `device`, behind the copies just queued."""

    def __init__(self, n, make):
        self._n, self._make, self._slots, self._events, self._at = int(n), make, [], [], -1

    def acquire(self):
        if len(self._slots) < self._n:
            self._slots.append(self._make())
            self._events.append(None)
        self._at = (self._at + 1) % self._n
        if self._events[self._at] is not None:
            self._events[self._at].synchronize()
        return self._slots[self._at]

    def release(self, device):
        self._events[self._at] = torch.cuda.Event()
        self._events[self._at].record(torch.cuda.current_stream(device))


def capture_fixed_step(step, device, drain):
    """(hipGraph, static output) of `step()` on `device`: on a side stream of its own, two eager warm-up calls (lazy
    allocations, parameter structs), `drain()` for the status words they queued, then one recorded call. `step` must
    queue no status word and allocate no pinned memory while the stream is capturing."""
    stream = torch.cuda.Stream(device)
    stream.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(stream):
        for _ in range(2):
            step()
        drain()
        torch.cuda.synchronize(device)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            static_out = step()
    torch.cuda.current_stream(device).wait_stream(stream)
    return graph, static_out
