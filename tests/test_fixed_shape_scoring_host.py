"""Host logic of data-root scoring through the fixed-shape step (pointvs_amd/captured_scoring.py): the capacity plan,
the deferred-submission loop of val(capture=True) driven by a fake scorer, the new status bits and the declarations of
the two new entry points. No GPU."""
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
import torch

ROOT = Path(__file__).resolve().parent.parent


# ---- plan_capacities ----------------------------------------------------------------------------------------------

def test_plan_capacities_rounds_up_with_headroom():
    from pointvs_amd.captured_scoring import Capacities, plan_capacities
    cap = plan_capacities([(1000, 300, 9000), (900, 400, 12000), (1100, 100, 100)], atoms_in_cap=7777)
    # largest of each, times 1.5, up to 64 / 64 / 1024: 1650 -> 1664, 600 -> 640, 18000 -> 18432
    assert cap == Capacities(1664, 640, 18432, 7777)
    assert plan_capacities([(64, 64, 1024)], 5, headroom=1.0) == Capacities(64, 64, 1024, 5)      # multiples stay
    assert plan_capacities([(65, 1, 1025)], 5, headroom=1.0) == Capacities(128, 64, 2048, 5)
    assert plan_capacities([(1, 1, 0)], 3) == Capacities(64, 64, 1024, 3)                          # never zero room
    assert plan_capacities([(100, 100, 1000)], 0, headroom=2.0) == Capacities(256, 256, 2048, 0)
    with pytest.raises(ValueError):
        plan_capacities([], 10)
    with pytest.raises(ValueError):
        plan_capacities([(10, 10, 10)], 10, headroom=0.9)


def test_plan_capacities_counts_a_batch_as_copies_of_the_largest_complex():
    from pointvs_amd.captured_scoring import Capacities, observed_sizes, plan_capacities
    probe = [(637, 341, 7106, 3832)]                                  # chembl6.types, its first batch of two
    assert plan_capacities(probe, 9, batch_size=None) == Capacities(960, 512, 11264, 9)
    # 2 x 341 = 682 nodes and 2 x 3,832 = 7,664 edges before the headroom: 1,023 -> 1,024 and 11,496 -> 12,288
    assert plan_capacities(probe, 9, batch_size=2) == Capacities(1024, 512, 12288, 9)
    assert plan_capacities([(900, 341, 9000, 3832)], 9, batch_size=2) == Capacities(1408, 512, 14336, 9)     # totals win
    assert plan_capacities([(637, 341, 7106)], 9, batch_size=2).edge_cap == 11264                  # no per-graph edges
    batch = SimpleNamespace(graph_node_counts=[341, 296], graph_edge_counts=[3832, 3274])
    assert observed_sizes(batch) == (637, 341, 7106, 3832)


def test_plan_capacities_stops_at_the_per_graph_limit_and_refuses_above_it():
    from pointvs_amd.captured_scoring import MAX_GRAPH_NODE_CAP, plan_capacities
    from pointvs_amd.parquet_data import MAX_LIGAND_ATOMS
    assert MAX_GRAPH_NODE_CAP == 4096 + MAX_LIGAND_ATOMS
    assert plan_capacities([(9000, 4000, 10)], 1).graph_node_cap == MAX_GRAPH_NODE_CAP      # 6000 with headroom: capped
    assert plan_capacities([(9000, MAX_GRAPH_NODE_CAP, 10)], 1).graph_node_cap == MAX_GRAPH_NODE_CAP
    with pytest.raises(ValueError, match='graphs of up to'):
        plan_capacities([(9000, MAX_GRAPH_NODE_CAP + 1, 10)], 1)


def test_atoms_in_cap_is_the_largest_batch_by_file_sizes():
    from pointvs_amd.captured_scoring import batch_input_atoms
    ds = SimpleNamespace(rec_pool=dict(ptr=np.array([0, 100, 350])), lig_pool=dict(ptr=np.array([0, 10, 30, 35])),
                         rec_ids=np.array([0, 0, 1, 1, 1]), lig_ids=np.array([0, 1, 2, 0, 1]))
    # samples: 110, 120, 255, 260, 270 input atoms
    assert batch_input_atoms(ds, [[0, 1], [2, 3], [4]]) == 515
    assert batch_input_atoms(ds, [[0], [1]]) == 120
    assert batch_input_atoms(ds, [[4, 4, 4]]) == 810                 # repeats count every time


# ---- the deferred-submission loop ------------------------------------------------------------------------------------

class FakeScorer:
    """replay / take_status of a FixedShapeScorer in pure Python: the score of sample i is 10 * i; `overflow` / `broken`
    name the batches (by first index) whose status word reports a capacity overflow / another bit. The static output is
    ONE tensor, overwritten by every replay - a loop that does not clone it writes the next batch's scores."""

    def __init__(self, batch_size, overflow=(), broken=()):
        self.static = torch.zeros(batch_size)
        self.overflow, self.broken, self.words, self.log = set(overflow), set(broken), [], []

    def replay(self, indices, check=True):
        from pointvs_amd import _lib
        assert check is False                                         # the loop reads every word itself
        assert len(self.words) <= 1, 'more than two steps in flight'
        self.log.append(('replay', tuple(indices)))
        self.static.copy_(torch.tensor([10.0 * i for i in indices]))
        code = _lib.CAP_EDGE_OVERFLOW if indices[0] in self.overflow else 4 if indices[0] in self.broken else 0
        self.words.append(code)
        return self.static

    def take_status(self):
        self.log.append(('status',))
        return self.words.pop(0)


def run_loop(n_samples, batch_size, probe_batches, overflow=(), broken=()):
    from pointvs_amd.captured_scoring import score_batches
    order = list(range(n_samples))
    batches = [order[k:k + batch_size] for k in range(0, n_samples, batch_size)]
    made, lines, calls = [], [], []

    def eager(indices):
        calls.append(('eager', tuple(indices)))
        return [('eager', i, 10.0 * i) for i in indices], (len(indices), 1, 0)

    def make_scorer(observed, all_batches):
        assert len(observed) == min(probe_batches, len(batches)) and all_batches == batches
        made.append(FakeScorer(batch_size, overflow, broken))
        return made[-1]

    def replayed(indices, scores):
        return [('replayed', i, float(s)) for i, s in zip(indices, scores)]

    stats = score_batches(batches, batch_size, eager, make_scorer, replayed, lines.extend, probe_batches=probe_batches)
    return stats, lines, made, calls


def assert_file_order(lines, n_samples):
    assert [i for _, i, _ in lines] == list(range(n_samples))
    assert all(score == 10.0 * i for _, i, score in lines)           # cloned: never the next batch's scores


@pytest.mark.parametrize('where', ('first', 'middle', 'last'))
def test_a_fallback_keeps_its_place_in_the_file(where):
    first_index = dict(first=4, middle=12, last=20)[where]            # batches of 4, one probe: replays are samples 4..23
    stats, lines, made, calls = run_loop(24, 4, 1, overflow={first_index})
    assert_file_order(lines, 24)
    assert stats == dict(eager=1, replayed=4, fallback=1)
    assert [kind for kind, i, _ in lines if i in range(first_index, first_index + 4)] == ['eager'] * 4
    assert ('eager', tuple(range(first_index, first_index + 4))) in calls
    assert sum(kind == 'replayed' for kind, _, _ in lines) == 16 and len(made) == 1


def test_statuses_are_read_one_batch_late():
    _, _, made, _ = run_loop(16, 4, 1)
    log = made[0].log
    assert [entry[0] for entry in log] == ['replay', 'replay', 'status', 'replay', 'status', 'status']


def test_a_short_last_batch_takes_the_eager_route():
    stats, lines, made, calls = run_loop(14, 4, 1, overflow={8})
    assert_file_order(lines, 14)
    assert stats == dict(eager=2, replayed=1, fallback=1)
    assert calls[-1] == ('eager', (12, 13)) and [kind for kind, i, _ in lines if i >= 12] == ['eager'] * 2


def test_fewer_batches_than_probe_batches_never_builds_a_scorer():
    stats, lines, made, _ = run_loop(10, 4, 4)
    assert_file_order(lines, 10)
    assert stats == dict(eager=3, replayed=0, fallback=0) and made == []
    stats, lines, made, _ = run_loop(9, 4, 2)                         # only a short batch is left after the probes
    assert stats == dict(eager=3, replayed=0, fallback=0) and made == []
    assert_file_order(lines, 9)


def test_another_status_bit_raises_the_loaders_error():
    with pytest.raises(ValueError, match='outside the feature encoding'):
        run_loop(16, 4, 1, broken={8})


# ---- status bits and declarations ---------------------------------------------------------------------------------------

def test_new_status_bits_do_not_collide_with_the_loaders():
    from pointvs_amd import _lib
    from pointvs_amd.captured_scoring import CAP_STATUS_TEXT, OVERFLOW_BITS, raise_for_status
    from pointvs_amd.parquet_data import _STATUS_TEXT
    old = [bit for bit, _ in _STATUS_TEXT]
    new = [bit for bit, _ in CAP_STATUS_TEXT]
    assert new == [_lib.CAP_NODE_OVERFLOW, _lib.CAP_GRAPH_OVERFLOW, _lib.CAP_EDGE_OVERFLOW, _lib.CAP_EMPTY_SAMPLE]
    assert all(bit > 0 and bit & (bit - 1) == 0 for bit in new) and len(set(old + new)) == len(old) + len(new)
    assert OVERFLOW_BITS == sum(new[:3]) and not OVERFLOW_BITS & _lib.CAP_EMPTY_SAMPLE
    header = (ROOT / 'include' / 'pvs_egnn.h').read_text()
    for name, bit in zip(('NODE_OVERFLOW', 'GRAPH_OVERFLOW', 'EDGE_OVERFLOW', 'EMPTY_SAMPLE'), new):
        assert re.search(rf'#define PVS_CAP_{name} {bit}\b', header), name
    raise_for_status(0)
    with pytest.raises(ValueError, match='no atom left'):
        raise_for_status(_lib.CAP_EMPTY_SAMPLE)
    with pytest.raises(ValueError, match='edge_cap'):
        raise_for_status(_lib.CAP_EDGE_OVERFLOW)
    with pytest.raises(ValueError, match='outside the pool'):
        raise_for_status(1 | _lib.CAP_EMPTY_SAMPLE)


def test_new_entry_points_are_declared_and_bound():
    from pointvs_amd import _lib
    header = (ROOT / 'include' / 'pvs_egnn.h').read_text()
    for name in ('pvs_complex_batch_build_cap', 'pvs_radius_graph_build_cap'):
        assert re.search(rf'\bint {name}\s*\(', header), name
        assert name in _lib._PROTOTYPES and name in _lib.EXPORTED_SYMBOLS
        declared = re.search(rf'\bint {name}\s*\(([^;]*)\);', header).group(1)
        assert len(declared.split(',')) == len(_lib._PROTOTYPES[name][1]), name     # one ctypes type per parameter
    assert _lib.MIN_VERSION == 113


def test_capture_val_flag_is_additive():
    from point_vs.parse_args import build_parser, command_line_parser, parse_args
    base = ['egnn', '/tmp/x']
    assert '--capture_val' in command_line_parser().format_help()      # listed by --help,
    assert '--capture_val' not in build_parser().format_help()         # beside the reference's flag surface, not in it
    assert parse_args(base).capture_val is False and parse_args(base + ['--capture_val']).capture_val is True
    with_flag, without = vars(parse_args(base + ['--capture_val', '-b', '8'])), vars(parse_args(base + ['-b', '8']))
    assert {k: v for k, v in with_flag.items() if k != 'capture_val'} == {k: v for k, v in without.items()
                                                                          if k != 'capture_val'}
