"""Host checks of pointvs_amd/nowait.py with CPU words (a CPU word is taken at once and is always ready): the order and
the bookkeeping of LateQueue, its ring, and the rotation and laziness of StagingRing."""
import pytest
import torch

from pointvs_amd.nowait import LateCopy, LateQueue, StagingRing


def word(value):
    return torch.tensor([value], dtype=torch.int32)


def test_a_cpu_word_is_taken_at_once_and_keeps_what_it_was_given():
    src, kept = word(7), object()
    copy = LateCopy(src, keep=kept)
    assert copy.event is None and copy.ready() and copy.wait() is src and copy.keep is kept
    host = word(0)
    into = LateCopy(src, host=host)
    src.fill_(8)                                      # a reused host word holds the value of the time of the copy
    assert into.wait() is host and int(host) == 7 and into.ready()


def test_take_returns_the_oldest_first_with_its_tag():
    q = LateQueue()
    assert q.take() is None and len(q) == 0
    for value, tag in ((5, 'a'), (9, 'b'), (2, None)):
        q.put(word(value), tag=tag)
    assert len(q) == 3
    assert q.take() == (5, 'a') and len(q) == 2
    assert q.take() == (9, 'b')
    assert q.take() == (2, None)
    assert q.take() is None and len(q) == 0


def test_landed_removes_an_entry_before_it_yields_it():
    q = LateQueue()
    q.put(word(1), tag='first')
    q.put(word(2), tag='second')
    seen = []
    with pytest.raises(ValueError, match='first'):
        for value, tag in q.landed():
            seen.append((value, tag, len(q)))         # the entry has left the queue when its value is handed out
            raise ValueError(tag)
    assert seen == [(1, 'first', 1)]
    assert list(q.landed()) == [(2, 'second')]        # the error was raised once; the entry behind it is still there
    assert list(q.landed()) == [] and len(q) == 0


def test_a_full_ring_refuses_and_takes_again_after_a_take():
    q = LateQueue(ring=2)
    words = list(q._free)
    first, second = q.put(word(5)), q.put(word(9))
    assert [first.host.data_ptr(), second.host.data_ptr()] == [w.data_ptr() for w in words]
    with pytest.raises(RuntimeError, match='take'):
        q.put(word(1))
    assert len(q) == 2                                # the refused put queued nothing
    assert q.take() == (5, None)
    third = q.put(word(4))
    assert third.host.data_ptr() == words[0].data_ptr()      # the word of the entry that was taken
    assert q.take() == (9, None) and q.take() == (4, None) and q.take() is None
    assert sorted(w.data_ptr() for w in q._free) == sorted(w.data_ptr() for w in words)


def test_without_a_ring_every_put_has_a_word_of_its_own():
    q = LateQueue()
    entries = [q.put(word(k)) for k in range(3)] + [q.put(word(7), tag='given')]
    assert q._free is None and len({e.host.data_ptr() for e in entries}) == 4


def test_waiting_for_one_entry_leaves_the_others_pending():
    q = LateQueue()
    entries = [q.put(word(value), tag=value) for value in (10, 11, 12)]
    assert q.take(entries[1]) == (11, 11)             # a backward waits for its own word only
    assert len(q) == 2 and q._entries == [entries[0], entries[2]]
    assert q.take(entries[1]) is None                 # handed out already: nothing, and nothing else is touched
    assert len(q) == 2
    assert q.take() == (10, 10) and q.take(entries[2]) == (12, 12) and len(q) == 0


def test_staging_slots_rotate_and_none_exists_before_the_first_acquire():
    made = []

    def make():
        made.append(torch.zeros((2, 3), dtype=torch.int32))
        return made[-1]

    ring = StagingRing(2, make)
    assert made == []
    first = ring.acquire()
    assert len(made) == 1 and first is made[0]        # one slot per acquire until the ring is full
    second = ring.acquire()
    assert len(made) == 2 and second is made[1]
    assert [id(ring.acquire()) for _ in range(4)] == [id(first), id(second), id(first), id(second)]
    assert len(made) == 2
