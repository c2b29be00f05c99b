"""The fixed-shape edge dropout, the host side (no GPU): the padded numpy reference (tests/_dropout_padded_ref.py) is
pinned to dropout_adj_ref and to the padding rule written out slot by slot, PF.static_dropout_plan to hand-computed
cases, the model's key function to the eager schedule, and the three new exports to header, prototypes and version.
tests/test_gpu_captured_dropout.py then holds the kernels, the model and the replayer to this reference exactly.
"""
import types
from pathlib import Path

import numpy as np
import pytest
import torch

from tests._dropout_padded_ref import dropout_adj_padded_ref, half_count
from tests._dropout_ref import SEED_STEPS, dropout_adj_ref
from tests.test_dropout_ref_host import HAND, HAND_ATTR

ROOT = Path(__file__).resolve().parents[1]
N_HAND = 10       # HAND names the nodes 0 .. 9


@pytest.mark.parametrize('p', [0.0, 0.3, 0.9, 0.999])
@pytest.mark.parametrize('n_pad', [2, 4, 6])
def test_the_padded_reference_is_the_dropped_list_then_the_padding_rule(p, n_pad):
    cap = 2 * half_count(HAND)
    assert cap == 18      # nine row <= col copies, three of them self-loops
    seen_dead = False
    for seed, step in SEED_STEPS + [(11, s) for s in range(6)]:
        oi, oa, k = dropout_adj_padded_ref(HAND, HAND_ATTR, p, seed, step, cap, N_HAND, n_pad)
        ref_i, ref_a = dropout_adj_ref(HAND, HAND_ATTR, p, seed, step)
        assert oi.dtype == np.int64 and oa.dtype == np.int64 and oi.shape == (2, cap) and oa.shape == (cap, 3)
        assert 2 * k == ref_i.shape[1] and np.array_equal(oi[:, :2 * k], ref_i) and np.array_equal(oa[:2 * k], ref_a)
        assert (cap - 2 * k) % 2 == 0
        for j in range(2 * k, cap):       # the rule, slot by slot
            d = j - 2 * k
            a = N_HAND + 2 * ((d // 2) % (n_pad // 2))
            assert tuple(oi[:, j]) == ((a, a + 1) if d % 2 == 0 else (a + 1, a)), (j, d)
            assert list(oa[j]) == [1, 0, 0]
        pad = oi[:, 2 * k:]
        assert pad.size == 0 or (N_HAND <= pad.min() and pad.max() < N_HAND + n_pad)
        for pair in range(n_pad // 2):    # both directions of every pair, equally often
            a = N_HAND + 2 * pair
            assert int(((pad[0] == a) & (pad[1] == a + 1)).sum()) == int(((pad[0] == a + 1) & (pad[1] == a)).sum())
        # the dead slots are dealt round the pairs: no pair is more than one edge pair ahead of another
        per_pair = [int((pad[0] == N_HAND + 2 * pair).sum()) for pair in range(n_pad // 2)]
        assert max(per_pair) - min(per_pair) <= 1
        seen_dead |= 2 * k < cap
        if p == 0.0:
            assert 2 * k == cap
    assert seen_dead or p == 0.0
    oi, oa, k = dropout_adj_padded_ref(HAND, None, p, 5, 1, cap, N_HAND, n_pad)
    assert oa is None and np.array_equal(oi, dropout_adj_padded_ref(HAND, HAND_ATTR, p, 5, 1, cap, N_HAND, n_pad)[0])


def test_a_capacity_above_the_bound_and_a_list_without_candidates():
    oi, oa, k = dropout_adj_padded_ref(HAND, HAND_ATTR, 0.3, 5, 1, 26, N_HAND, 4)
    tight = dropout_adj_padded_ref(HAND, HAND_ATTR, 0.3, 5, 1, 18, N_HAND, 4)
    assert oi.shape == (2, 26) and np.array_equal(oi[:, :18], tight[0]) and np.array_equal(oa[:18], tight[1])
    down = np.stack([np.maximum(HAND[0], HAND[1]) + 1, np.minimum(HAND[0], HAND[1])])      # every edge has row > col
    assert half_count(down) == 0
    oi, oa, k = dropout_adj_padded_ref(down, HAND_ATTR, 0.3, 5, 1, 0, N_HAND + 1, 2)
    assert k == 0 and oi.shape == (2, 0) and oa.shape == (0, 3)
    oi, oa, k = dropout_adj_padded_ref(down, HAND_ATTR, 0.3, 5, 1, 4, N_HAND + 1, 2)
    assert k == 0 and oi.tolist() == [[11, 12, 11, 12], [12, 11, 12, 11]]
    with pytest.raises(AssertionError):
        dropout_adj_padded_ref(HAND, HAND_ATTR, 0.0, 5, 1, 16, N_HAND, 2)


def test_static_dropout_plan_on_hand_computed_cases():
    from pointvs_amd.functional import static_dropout_plan
    # the two-graph batch of the GPU tests: 207 nodes, 1,235 candidates; 0.25 * 207 / 2 = 25.875 -> 26 pairs
    assert static_dropout_plan(207, 1235, 0.25) == (2470, 52)
    assert static_dropout_plan(207, 1235, 1e-9) == (2470, 2)
    assert static_dropout_plan(207, 1235, 0.0) == (2470, 2)
    assert static_dropout_plan(30, 40, 0.999) == (80, 30)             # 29.97 / 2 = 14.985 -> 15 pairs
    assert static_dropout_plan(8, 3, 0.5) == (6, 4)                   # exactly two pairs: no rounding up
    assert static_dropout_plan(9, 3, 0.5) == (6, 6)                   # 2.25 -> 3 pairs
    # self-loops are candidates like any row <= col copy (a surviving one is listed twice)
    assert half_count(HAND) == 9 and static_dropout_plan(N_HAND, half_count(HAND), 0.3) == (18, 4)
    loops = np.stack([np.arange(5), np.arange(5)])
    assert static_dropout_plan(5, half_count(loops), 0.5) == (10, 4)
    assert static_dropout_plan(207, 0, 0.25) == (0, 52)
    assert static_dropout_plan(0, 0, 0.25) == (0, 2)
    for cap, n_pad in (static_dropout_plan(n, h, p) for n in (1, 7, 1000) for h in (0, 1, 999) for p in (0.0, 0.3, 0.999)):
        assert cap % 2 == 0 and n_pad % 2 == 0 and n_pad >= 2
    for bad in ((-1, 0, 0.1), (3, -1, 0.1), (3, 1, 1.0), (3, 1, -0.1)):
        with pytest.raises(ValueError):
            static_dropout_plan(*bad)


def _schedule_owner(**counters):
    return types.SimpleNamespace(p_epoch=0, a_epoch=0, global_iter=0, **counters)


def test_the_key_function_is_the_eager_schedule(monkeypatch):
    """DropoutKeys.next (model.next_dropout_key forwards to it): seed = torch.initial_seed() (+ the rank's multiple of the golden ratio), step =
    _mix64(_mix64(base) + calls) with base = (epochs << 24) + global_iter and calls counted from 1 under one base."""
    from pointvs_amd.egnn_satorras import DropoutKeys, _mix64
    torch.manual_seed(77)
    owner, keys = _schedule_owner(), DropoutKeys()
    got, want, calls, base_was = [], [], 0, None
    for bump in (None, None, None, 'global_iter', 'p_epoch', 'a_epoch', 'global_iter', None):
        if bump:
            setattr(owner, bump, getattr(owner, bump) + 1)
        base = ((owner.p_epoch + owner.a_epoch) << 24) + owner.global_iter
        calls = calls + 1 if base == base_was else 1
        base_was = base
        got.append(keys.next(owner))
        want.append((77, _mix64(_mix64(base) + calls)))
    assert got == want and len({s for _, s in got}) == len(got)
    assert (keys.base, keys.calls) == ((2 << 24) + 2, 2)
    # a training loop: one draw per optimiser step
    owner, keys = _schedule_owner(), DropoutKeys()
    loop = []
    for _ in range(4):
        loop.append(keys.next(owner))
        owner.global_iter += 1
    assert loop == [(77, _mix64(_mix64(it) + 1)) for it in range(4)]
    # the same counters give the same keys again; another torch seed another seed, the same steps
    assert DropoutKeys().next(_schedule_owner()) == loop[0]
    torch.manual_seed(78)
    assert DropoutKeys().next(_schedule_owner()) == (78, loop[0][1])
    monkeypatch.setattr(torch.distributed, 'is_initialized', lambda: True)
    monkeypatch.setattr(torch.distributed, 'get_rank', lambda *a, **k: 3)
    seed, step = DropoutKeys().next(_schedule_owner())
    assert seed == (78 + 3 * 0x9E3779B97F4A7C15) % 2 ** 64 and step == loop[0][1]


def test_new_exports_are_declared_bound_and_versioned():
    from pointvs_amd import _lib
    header = (ROOT / 'include' / 'pvs_egnn.h').read_text()
    source = (ROOT / 'pointvs_amd' / 'csrc' / 'dropout_adj.hip').read_text()
    for name, n_args in (('pvs_dropout_key_write', 4), ('pvs_dropout_adj_mark_dev', 8), ('pvs_dropout_adj_fill_padded', 11)):
        assert f'int {name}(' in header and f'extern "C" int {name}(' in source, name
        assert name in _lib.EXPORTED_SYMBOLS and len(_lib._PROTOTYPES[name][1]) == n_args, name
        assert hasattr(_lib.lib(), name), name
    assert len(_lib._PROTOTYPES['pvs_dropout_adj_mark'][1]) == 9 and len(_lib._PROTOTYPES['pvs_dropout_adj_fill'][1]) == 9
    assert source.count('philox_round(c, k0, k1)') == 1, 'one copy of the Philox rounds'
    assert _lib.MIN_VERSION >= 111 and _lib.lib().pvs_version() >= 111


def test_the_switch_is_off_by_default():
    from pointvs_amd.egnn_multitask import MultitaskSatorrasEGNN
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    assert SartorrasEGNN.static_dropout is None and MultitaskSatorrasEGNN.static_dropout is None
