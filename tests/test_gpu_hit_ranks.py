"""Per-hit ranks on the device (PF.hit_value_ranks, pvs_hit_value_ranks) and the accumulation kernel by itself
(PF.hit_rows_accumulate, pvs_hit_rows_accumulate), bit for bit against their numpy restatement (tests/_hit_rank_ref.py):
small integers plus specials as values, so every rank and every float64 sum is exact and ties are everywhere. Shapes:
n_rec at the wavefront, workgroup and LDS-tile (T = HIT_RANK_TILE) boundaries, ligands of 0, 1, 64, 65 and 1024 atoms
mixed in one call of 7 hits, the last one empty."""
import numpy as np
import pytest
import torch

from tests import _hit_rank_ref as ref

pytestmark = pytest.mark.gpu

SIZES = [1, 0, 64, 65, 1024, 5, 0]          # ligand atoms per hit; the last hit is empty
PAD, SENTINEL = 9, -7.0
NAN, INF = np.float32(np.nan), np.float32(np.inf)


def _tile():
    from pointvs_amd import functional as PF
    return PF.HIT_RANK_TILE


def _n_recs():
    t = _tile()
    return [1, 63, 64, 65, t - 1, t, t + 1, 2 * t + 3]


def _inputs(n_rec):
    """rows [7, n_rec], lig_val [sum(SIZES) + PAD], lig_ptr: integers in -8..8 with NaN among them, and per hit:
    0 an all-NaN row; 1 a row without NaN; 2 one repeated value, ligand and receptor; 3 signed zeros and both
    infinities; 4 - 6 as drawn."""
    rng = np.random.default_rng(1000 + n_rec)
    rows = rng.integers(-8, 9, size=(len(SIZES), n_rec)).astype(np.float32)
    rows[rng.random(rows.shape) < 0.3] = NAN
    lig_ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    lig_val = rng.integers(-8, 9, size=int(lig_ptr[-1]) + PAD).astype(np.float32)
    lig_val[rng.random(lig_val.shape) < 0.1] = NAN
    rows[0] = NAN
    rows[1] = rng.integers(-8, 9, size=n_rec).astype(np.float32)
    rows[2] = 3.0
    lig_val[lig_ptr[2]:lig_ptr[3]] = 3.0
    specials = np.array([-0.0, 0.0, INF, -INF, 0.0, -0.0, NAN, INF, -INF], dtype=np.float32)
    rows[3, :min(n_rec, len(specials))] = specials[:n_rec]
    lig_val[lig_ptr[3]:lig_ptr[3] + len(specials)] = specials[::-1]
    return rows, lig_val, lig_ptr


_WANT = {}


def _want(n_rec):
    """The reference after one and after two calls into the same accumulators, with and without the ligand."""
    if n_rec not in _WANT:
        rows, lig_val, lig_ptr = _inputs(n_rec)
        both, alone = [], []
        acc_b, acc_a = ref.fresh_accumulators(n_rec), ref.fresh_accumulators(n_rec)
        for _ in range(2):
            got = ref.hit_value_ranks(rows, lig_val, lig_ptr, np.full(len(lig_val), SENTINEL, dtype=np.float32), *acc_b)
            both.append(got)
            acc_b = got[2:]
            got = ref.hit_value_ranks(rows, None, None, None, *acc_a)
            alone.append(got)
            acc_a = got[2:]
        _WANT[n_rec] = (both, alone)
    return _WANT[n_rec]


def _run(n_rec, with_lig):
    """Two calls into sentinel-filled outputs and the same fresh accumulators; the outputs as numpy after each."""
    from pointvs_amd import functional as PF
    rows, lig_val, lig_ptr = (torch.from_numpy(a).cuda() for a in _inputs(n_rec))
    out = (torch.full_like(rows, SENTINEL), torch.full_like(lig_val, SENTINEL) if with_lig else None)
    acc = PF.new_contact_accumulators(n_rec, 'cuda')
    after = []
    for _ in range(2):
        got = PF.hit_value_ranks(rows, *((lig_val, lig_ptr) if with_lig else ()), out=out, acc=acc)
        assert got[0] is out[0] and got[1] is out[1] and all(g is a for g, a in zip(got[2:], acc))
        after.append(tuple(None if t is None else t.cpu().numpy() for t in got))
    return after


NAMES = ('row_rank', 'lig_rank', 'rank_sum', 'rank_count', 'rank_max')


def _same_bits(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        if w is None:
            assert g is None, (what, name)
            continue
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert g.tobytes() == w.tobytes(), (what, name, np.nonzero(~((g == w) | (np.isnan(g) & np.isnan(w)))))


@pytest.mark.parametrize('k', range(8))
def test_ranks_are_exact_with_and_without_the_ligand(k):
    n_rec = _n_recs()[k]
    rows, lig_val, lig_ptr = _inputs(n_rec)
    both, alone = _want(n_rec)
    # the inputs hold the cases
    assert np.isnan(rows[0]).all() and not np.isnan(rows[1]).any() and (rows[2] == 3).all()
    assert np.isnan(both[0][0][0]).all() and not np.isnan(both[0][0][1]).any()
    m = SIZES[2] + n_rec
    assert np.array_equal(np.concatenate([both[0][1][lig_ptr[2]:lig_ptr[3]], both[0][0][2]]), np.arange(m))
    assert np.signbit(rows[3, 0]) and rows[3, 0] == 0 and not np.isnan(lig_val[:lig_ptr[-1]]).all()
    assert both[0][1][0] == 0 or np.isnan(lig_val[0])                       # one ligand atom beside an all-NaN row
    got = _run(n_rec, True)
    for call in range(2):
        _same_bits(got[call], both[call], f'n_rec {n_rec} call {call}')
        assert (got[call][1][int(lig_ptr[-1]):] == SENTINEL).all()       # behind lig_ptr[n_hits]: left alone
    assert got[0][0].tobytes() == got[1][0].tobytes() and got[0][1].tobytes() == got[1][1].tobytes()
    assert np.array_equal(got[1][2], 2 * got[0][2]) and np.array_equal(got[1][3], 2 * got[0][3])
    again = _run(n_rec, True)                                               # the same bits every time
    assert all(a.tobytes() == b.tobytes() for x, y in zip(got, again) for a, b in zip(x, y))
    # the receptor-only form: three NULLs
    got = _run(n_rec, False)
    for call in range(2):
        _same_bits(got[call], alone[call], f'n_rec {n_rec} receptor only, call {call}')
    if n_rec > 9:
        assert not np.array_equal(alone[0][0], both[0][0], equal_nan=True)


def test_a_hit_that_is_none_writes_nan_and_adds_nothing():
    from pointvs_amd import functional as PF
    n_rec = 70
    rng = np.random.default_rng(5)
    rows = rng.integers(-8, 9, size=(6, n_rec)).astype(np.float32)
    lig_val = rng.integers(-8, 9, size=1040).astype(np.float32)
    # hit 0: 3 atoms; 1: 1,025 atoms; 2: descends; 3: empty; 4: descends below zero; 5: starts below zero
    lig_ptr = np.array([0, 3, 1028, 1020, 1020, -4, 2], dtype=np.int32)
    want = ref.hit_value_ranks(rows, lig_val, lig_ptr, np.full(1040, SENTINEL, dtype=np.float32),
                               *ref.fresh_accumulators(n_rec))
    assert np.isnan(want[0][[1, 2, 4, 5]]).all() and not np.isnan(want[0][[0, 3]]).any()
    assert (want[1][3:] == SENTINEL).all() and (want[3] == 2).all()
    out = (torch.full((6, n_rec), SENTINEL).cuda(), torch.full((1040,), SENTINEL).cuda())
    got = PF.hit_value_ranks(torch.from_numpy(rows).cuda(), torch.from_numpy(lig_val).cuda(),
                             torch.from_numpy(lig_ptr).cuda(), out=out)
    _same_bits([t.cpu().numpy() for t in got], want, 'invalid hits')


def test_refusals_return_non_zero_and_write_nothing():
    from pointvs_amd import _lib
    from pointvs_amd import functional as PF
    lib = _lib.lib()
    n_hits, n_rec = 3, 40
    rows = torch.ones((n_hits, n_rec)).cuda()
    lig_val, lig_ptr = torch.ones(6).cuda(), torch.tensor([0, 2, 4, 6], dtype=torch.int32).cuda()
    row_rank, lig_rank = torch.full((n_hits, n_rec), SENTINEL).cuda(), torch.full((6,), SENTINEL).cuda()
    acc = PF.new_contact_accumulators(n_rec, 'cuda')
    stream = _lib.stream(rows.device)
    p = _lib.ptr

    def ranks(rows=rows, n_hits=n_hits, n_rec=n_rec, lig_val=lig_val, lig_ptr=lig_ptr, row_rank=row_rank,
              lig_rank=lig_rank, acc=acc):
        return lib.pvs_hit_value_ranks(p(rows), n_hits, n_rec, p(lig_val), p(lig_ptr), p(row_rank), p(lig_rank),
                                       *(p(t) for t in acc), stream)
    assert ranks(rows=None) != 0 and ranks(row_rank=None) != 0
    for k in range(3):
        assert ranks(acc=[None if i == k else t for i, t in enumerate(acc)]) != 0
    assert ranks(n_hits=-1) != 0 and ranks(n_rec=-1) != 0
    assert ranks(lig_val=None) != 0 and ranks(lig_ptr=None) != 0 and ranks(lig_rank=None) != 0   # all or none
    assert ranks(n_rec=(1 << 24) - 1024) != 0                                 # a rank would not be exact in fp32
    assert b'2^24' in lib.pvs_last_error()
    assert lib.pvs_hit_rows_accumulate(None, n_hits, n_rec, *(p(t) for t in acc), stream) != 0
    assert lib.pvs_hit_rows_accumulate(p(rows), -1, n_rec, *(p(t) for t in acc), stream) != 0
    assert lib.pvs_hit_rows_accumulate(p(rows), n_hits, n_rec, None, p(acc[1]), p(acc[2]), stream) != 0
    # nothing to do: 0 without a launch, whatever the pointers
    assert ranks(n_hits=0, rows=None) == 0 and ranks(n_rec=0, rows=None) == 0
    assert lib.pvs_hit_rows_accumulate(None, 0, n_rec, None, None, None, stream) == 0
    torch.cuda.synchronize()
    assert bool((row_rank == SENTINEL).all()) and bool((lig_rank == SENTINEL).all())
    assert not acc[0].any() and not acc[1].any() and bool(torch.isnan(acc[2]).all())
    # the wrapper
    with pytest.raises(ValueError):
        PF.hit_value_ranks(rows, lig_val)                                      # lig_val without lig_ptr
    with pytest.raises(ValueError):
        PF.hit_value_ranks(rows, lig_val, lig_ptr[:-1])
    with pytest.raises(TypeError):
        PF.hit_value_ranks(rows.double())
    with pytest.raises(ValueError, match='out ='):
        PF.hit_value_ranks(rows, lig_val, lig_ptr, out=(row_rank, None))
    with pytest.raises(ValueError, match='out ='):
        PF.hit_value_ranks(rows, out=(rows, None))                             # in place
    with pytest.raises(ValueError, match='acc ='):
        PF.hit_value_ranks(rows, acc=PF.new_contact_accumulators(n_rec + 1, 'cuda'))
    with pytest.raises(ValueError, match='acc ='):
        PF.hit_rows_accumulate(rows, (acc[0].float(), acc[1], acc[2]))
    with pytest.raises(RuntimeError):
        PF.hit_value_ranks(rows.cpu())
    empty = PF.hit_value_ranks(torch.empty((0, n_rec)).cuda())
    assert empty[0].shape == (0, n_rec) and empty[1] is None and not empty[3].any()
    assert ranks() == 0                                                        # (the arguments above: fine)


def test_rows_accumulate_is_the_accumulation_of_slot_node_values():
    from pointvs_amd import functional as PF
    n_rec, sizes = 70, [3, 0, 65, 1]
    rng = np.random.default_rng(9)
    lig_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    node_ptr = (lig_ptr + np.arange(len(sizes) + 1) * n_rec).astype(np.int32)
    y = torch.from_numpy(rng.integers(-8, 9, size=(int(node_ptr[-1]), 2)).astype(np.float32)).cuda()
    node_ptr, lig_ptr = torch.from_numpy(node_ptr).cuda(), torch.from_numpy(lig_ptr).cuda()
    acc = None
    for _ in range(2):          # two calls: the accumulators are read and updated
        out = None if acc is None else (lig_val, slot_rec_val) + acc
        lig_val, slot_rec_val, *acc = PF.slot_node_values(y, node_ptr, lig_ptr, n_rec, column=1, out=out)
        acc = tuple(acc)
    assert bool(torch.isnan(slot_rec_val[1]).all()) and not bool(torch.isnan(slot_rec_val[0]).any())
    mine = PF.new_contact_accumulators(n_rec, 'cuda')
    for _ in range(2):
        got = PF.hit_rows_accumulate(slot_rec_val, mine)
        assert all(g is m for g, m in zip(got, mine))
    for g, w in zip(mine, acc):
        assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes()
    rows = slot_rec_val.cpu().numpy()
    want = ref.accumulate(rows, *ref.accumulate(rows, *ref.fresh_accumulators(n_rec)))
    for g, w in zip(mine, want):
        assert g.cpu().numpy().tobytes() == w.tobytes()
    assert int(mine[1].max()) == 6                  # three slots with atoms, twice
