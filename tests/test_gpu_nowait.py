"""GPU checks of pointvs_amd/nowait.py at the smallest shapes: one-element words through the ring and across two streams,
a [2, 3] staging slot through three rounds, a captured step that adds and counts."""
import pytest
import torch

from pointvs_amd.nowait import LateQueue, StagingRing, capture_fixed_step, pinned

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)


def test_a_ring_of_two_hands_the_words_out_in_order_and_reuses_them():
    q = LateQueue(ring=2)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    status.fill_(5)
    first = q.put(status, tag='a')
    status.fill_(9)
    second = q.put(status, tag='b')
    assert first.host.is_pinned() and second.host.is_pinned() and first.host.data_ptr() != second.host.data_ptr()
    with pytest.raises(RuntimeError, match='take'):
        q.put(status)
    assert q.take() == (5, 'a') and q.take() == (9, 'b') and q.take() is None
    status.fill_(12)
    third = q.put(status)
    assert third.host.data_ptr() == first.host.data_ptr()
    assert q.take() == (12, None) and len(q) == 0


def test_words_of_two_streams_have_both_landed_after_a_synchronise():
    q = LateQueue()
    entries = []
    for value in (3, 4):
        stream = torch.cuda.Stream(DEV)
        with torch.cuda.stream(stream):
            status = torch.full((1,), value, dtype=torch.int32, device=DEV)
            entries.append(q.put(status, tag=value, keep=status))
    assert entries[0].host.is_pinned() and entries[0].host.data_ptr() != entries[1].host.data_ptr()
    torch.cuda.synchronize()
    assert all(e.ready() for e in entries)
    assert list(q.landed()) == [(3, 3), (4, 4)]
    assert list(q.landed()) == [] and len(q) == 0


def test_three_rounds_through_two_staging_slots():
    made = []

    def make():
        made.append(pinned((2, 3), torch.int32))
        return made[-1]

    ring = StagingRing(2, make)
    assert made == []
    results, slots = [], []
    for k in range(3):
        host = ring.acquire()
        slots.append(host.data_ptr())
        host.copy_(torch.arange(6, dtype=torch.int32).reshape(2, 3) + 10 * k)
        results.append(torch.empty((2, 3), dtype=torch.int32, device=DEV))
        results[-1].copy_(host, non_blocking=True)
        ring.release(DEV)
    assert len(made) == 2 and all(h.is_pinned() for h in made)
    assert slots[0] != slots[1] and slots[2] == slots[0]
    torch.cuda.synchronize()
    for k, got in enumerate(results):
        assert got.cpu().tolist() == [[10 * k, 10 * k + 1, 10 * k + 2], [10 * k + 3, 10 * k + 4, 10 * k + 5]]


def test_a_captured_step_warms_up_twice_drains_once_and_replays():
    static_in = torch.tensor([1.0, 2.0, 3.0], device=DEV)
    static_out = torch.zeros(3, device=DEV)
    count = torch.zeros(1, dtype=torch.int32, device=DEV)
    order = []

    def step():
        order.append('capturing' if torch.cuda.is_current_stream_capturing() else 'eager')
        static_out.add_(static_in)
        count.add_(1)
        return static_out

    def drain():
        order.append('drain')
        assert int(count.item()) == 2                          # both warm-ups have run, nothing was recorded yet

    graph, out = capture_fixed_step(step, DEV, drain)
    assert order == ['eager', 'eager', 'drain', 'capturing']
    assert out is static_out
    torch.cuda.synchronize()
    assert int(count.item()) == 2 and static_out.tolist() == [2.0, 4.0, 6.0]      # the recorded call has not run
    expected = [2.0, 4.0, 6.0]
    for k, values in enumerate(([10.0, 20.0, 30.0], [0.5, 0.25, -1.0])):
        static_in.copy_(torch.tensor(values))
        graph.replay()
        torch.cuda.synchronize()
        expected = [a + b for a, b in zip(expected, values)]
        assert static_out.tolist() == expected and int(count.item()) == 3 + k
