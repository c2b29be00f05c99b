"""The host reference of the edge dropout (tests/_dropout_ref.py) is pinned here, without a GPU: Philox4x32-10 to the
published Random123 known-answer vectors, the 24-bit uniform to its range, the stream to its statistics (each 32-bit
half of seed and step changes it), dropout_adj_ref to the properties of dropout_adj(force_undirected=True), and the
model's step mix to being a bijection. tests/test_gpu_edge_dropout.py then holds the kernels to this reference exactly.
"""
import numpy as np
import pytest

from tests._dropout_ref import MAX_DRAW, SEED_STEPS, ZERO_DRAW, dropout_adj_ref, philox4x32_10, uniform24

N = 1 << 20


def _words(hex_words):
    return [int(w, 16) for w in hex_words.split()]


@pytest.mark.parametrize('counter,key,output', [
    ('00000000 00000000 00000000 00000000', '00000000 00000000', '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
    ('ffffffff ffffffff ffffffff ffffffff', 'ffffffff ffffffff', '408f276d 41c83b0e a20bc7c6 6d5451fd'),
    ('243f6a88 85a308d3 13198a2e 03707344', 'a4093822 299f31d0', 'd16cfe09 94fdcceb 5001e420 24126ea1'),
])
def test_philox_known_answer_vectors(counter, key, output):
    """Random123's kat_vectors for philox4x32 with 10 rounds, as scalars and as one lane of a vectorised call."""
    got = philox4x32_10(_words(counter), _words(key))
    assert [int(w) for w in got] == _words(output)
    lanes = [np.array([1, c, 2], dtype=np.uint64) for c in _words(counter)]
    got = philox4x32_10(lanes, _words(key))
    assert [int(w[1]) for w in got] == _words(output)
    assert all(w.dtype == np.uint64 and int(w.max()) < 2 ** 32 for w in got)


def test_uniform24_is_word0_of_the_counter_and_key_layout():
    """counter (e_lo, e_hi, step_lo, step_hi), key (seed_lo, seed_hi), word 0, >> 8: the third known-answer vector read
    as (seed, step, e)."""
    seed, step, e = (0x299f31d0 << 32) | 0xa4093822, (0x03707344 << 32) | 0x13198a2e, (0x85a308d3 << 32) | 0x243f6a88
    u = uniform24(seed, step, e)
    assert u.dtype == np.float32 and float(u) == (0xd16cfe09 >> 8) / 2.0 ** 24
    assert float(uniform24(0, 0, 0)) == (0x6627e8d5 >> 8) / 2.0 ** 24
    assert float(uniform24(2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1)) == (0x408f276d >> 8) / 2.0 ** 24


_STREAMS = {}


def _stream(seed, step):
    """uniform24 of the counters 0 .. 2**20 - 1: computed once per (seed, step), never written to."""
    if (seed, step) not in _STREAMS:
        u = uniform24(seed, step, np.arange(N))
        u.setflags(write=False)
        _STREAMS[seed, step] = u
    return _STREAMS[seed, step]


@pytest.mark.parametrize('seed,step', SEED_STEPS)
def test_uniform24_range(seed, step):
    u = _stream(seed, step)
    assert u.dtype == np.float32 and u.shape == (N,)
    assert float(u.min()) >= 0.0 and float(u.max()) <= 1.0 - 2.0 ** -24
    scaled = u.astype(np.float64) * 2.0 ** 24
    assert np.array_equal(scaled, np.round(scaled)), 'every value is a multiple of 2**-24'
    assert len(np.unique(u)) > N // 2


def test_the_boundary_draws_are_what_they_are_named():
    assert float(uniform24(*ZERO_DRAW)) == 0.0
    assert float(uniform24(*MAX_DRAW)) == 1.0 - 2.0 ** -24
    assert np.float32(1.0 - 2.0 ** -24) == np.float32(0xFFFFFF) * np.float32(2.0 ** -24) < np.float32(1.0)


@pytest.mark.parametrize('seed,step', SEED_STEPS)
def test_kept_count_of_the_reference(seed, step):
    """kept ~ Binomial(n, 1 - p) (the 24-bit grid moves the probability by less than 2**-24: 1/16 of a count at this
    n), so |kept - n (1 - p)| <= 4 sigma with sigma = sqrt(n p (1 - p))."""
    u = _stream(seed, step)
    for p in (0.1, 0.3, 0.5, 0.9):
        kept = int((u >= np.float32(p)).sum())
        sigma = np.sqrt(N * p * (1 - p))
        assert abs(kept - N * (1 - p)) <= 4 * sigma, (p, kept, (kept - N * (1 - p)) / sigma)


@pytest.mark.parametrize('seed,step', [(7, 8), (8, 7), (7, 7 + 2 ** 32), (7 + 2 ** 32, 7)])
def test_each_half_of_seed_and_step_changes_the_stream(seed, step):
    """Two independent p = 0.5 masks agree in Binomial(n, 1/2) places: n/2 +- 4 sqrt(n)/2. A half that did not reach the
    generator would give n agreements."""
    base = _stream(7, 7) >= np.float32(0.5)
    agree = int((base == (_stream(seed, step) >= np.float32(0.5))).sum())
    assert abs(agree - N / 2) <= 4 * np.sqrt(N) / 2, (agree, (agree - N / 2) / (np.sqrt(N) / 2))


# ---- dropout_adj_ref on a hand-made list ----------------------------------------------------------------------------
#                 pair both ways  duplicate    pair, far apart  self-loops   row > col only  duplicate pair
HAND = np.array([[0, 1, 0, 3, 3, 2, 6, 7, 6, 9, 5, 1, 0],
                 [1, 0, 1, 4, 4, 5, 6, 7, 6, 8, 2, 0, 1]], dtype=np.int64)
HAND_ATTR = np.stack([np.arange(13) * 10 + 1, -np.arange(13) - 1, np.arange(13) + 2 ** 33], 1).astype(np.int64)


def _padded(n_edges, pattern=HAND, attr=HAND_ATTR):
    reps = -(-n_edges // pattern.shape[1])
    return np.tile(pattern, (1, reps))[:, :n_edges].copy(), np.tile(attr, (reps, 1))[:n_edges].copy()


@pytest.mark.parametrize('p', [0.0, 0.3, 0.5, 0.9])
def test_properties_of_the_reference_list(p):
    seen_self_loop = seen_drop = False
    for seed, step in SEED_STEPS + [(11, s) for s in range(10)]:
        oi, oa = dropout_adj_ref(HAND, HAND_ATTR, p, seed, step)
        assert oi.dtype == np.int64 and oa.dtype == np.int64 and oi.shape[0] == 2 and oi.shape[1] % 2 == 0
        k = oi.shape[1] // 2
        assert oa.shape == (2 * k, 3)
        assert np.array_equal(oi[:, k:], oi[::-1, :k]), 'the second half is the reverse of the first'
        assert np.array_equal(oa[k:], oa[:k])
        assert (oi[0, :k] <= oi[1, :k]).all()
        assert not ((oi[0] == 9) | (oi[1] == 9)).any(), 'the edge whose only copy has row > col never survives'
        # the survivors are input edges in input order, each with its own attribute row (column 0 names the edge)
        ids = (oa[:k, 0] - 1) // 10
        assert (np.diff(ids) > 0).all() and np.array_equal(HAND[:, ids], oi[:, :k]) and np.array_equal(HAND_ATTR[ids], oa[:k])
        u = uniform24(seed, step, np.arange(HAND.shape[1]))
        assert set(ids) == {e for e in range(HAND.shape[1]) if HAND[0, e] <= HAND[1, e] and u[e] >= np.float32(p)}
        for loop in (6, 7, 8):        # edges 6, 7, 8 are self-loops: their own reverse, so twice in the output
            if loop in ids:
                seen_self_loop = True
                node = HAND[0, loop]
                assert ((oi[0] == node) & (oi[1] == node)).sum() == 2 * (HAND[:, ids] == node).all(0).sum()
        seen_drop |= k < 9
        if p == 0.0:
            assert k == 9       # all row <= col copies
    assert seen_self_loop and (seen_drop or p == 0.0)
    oi, oa = dropout_adj_ref(HAND, None, p, 5, 1)
    assert oa is None and np.array_equal(oi, dropout_adj_ref(HAND, HAND_ATTR, p, 5, 1)[0])


def test_smallest_and_largest_probability():
    """p = 2**-24 drops exactly the counters whose 24-bit value is 0; p = float32(1 - 2**-24) keeps exactly the maximal
    value. Counter 196 (value 0) and counter 65 (maximal) of the searched draws sit on row <= col edges."""
    ei, ea = _padded(200)
    for e in (ZERO_DRAW[2], MAX_DRAW[2]):
        ei[:, e] = (4, 8)
    ea[:, 0] = np.arange(200)
    cand = np.flatnonzero(ei[0] <= ei[1])
    oi, oa = dropout_adj_ref(ei, ea, 2.0 ** -24, *ZERO_DRAW[:2])
    assert list(oa[:len(oa) // 2, 0]) == [e for e in cand if e != ZERO_DRAW[2]]
    oi, oa = dropout_adj_ref(ei, ea, 2.0 ** -24, *MAX_DRAW[:2])
    assert list(oa[:len(oa) // 2, 0]) == list(cand)
    oi, oa = dropout_adj_ref(ei, ea, np.float32(1.0 - 2.0 ** -24), *MAX_DRAW[:2])
    assert list(oa[:, 0]) == [MAX_DRAW[2]] * 2 and np.array_equal(oi, [[ei[0, 65], ei[1, 65]], [ei[1, 65], ei[0, 65]]])
    oi, oa = dropout_adj_ref(ei, ea, np.float32(1.0 - 2.0 ** -24), *ZERO_DRAW[:2])
    assert oi.shape == (2, 0) and oa.shape == (0, 3)


# ---- the model's step mix -------------------------------------------------------------------------------------------
M64 = 2 ** 64 - 1


def _unmix64(y):
    """Inverse of splitmix64's finaliser, step by step: x ^ (x >> s) is undone by repeating the shift, an odd multiplier
    by its inverse modulo 2**64."""
    y = y ^ (y >> 31) ^ (y >> 62)
    y = (y * pow(0x94D049BB133111EB, -1, 2 ** 64)) & M64
    y = y ^ (y >> 27) ^ (y >> 54)
    y = (y * pow(0xBF58476D1CE4E5B9, -1, 2 ** 64)) & M64
    y = y ^ (y >> 30) ^ (y >> 60)
    return (y - 0x9E3779B97F4A7C15) & M64


def test_mix64_is_a_bijection_with_live_high_words():
    from pointvs_amd.egnn_satorras import _mix64
    rng = np.random.default_rng(3)
    sample = list(range(300)) + [(1 << 24) * e + i for e in range(4) for i in range(4)] \
        + [int(v) for v in rng.integers(0, 2 ** 64, 300, dtype=np.uint64)] + [M64, 2 ** 63, 2 ** 32]
    out = [_mix64(x) for x in sample]
    assert all(0 <= y <= M64 for y in out) and len(set(out)) == len(set(sample))
    assert [_unmix64(y) for y in out] == sample
    assert all(y >> 32 for y in out), 'a step without a high word'
    # the model's step: _mix64(_mix64(base) + calls)
    steps = [_mix64(_mix64(base) + calls) for base in (0, 1, 1 << 24) for calls in (1, 2, 3)]
    assert len(set(steps)) == 9 and all(s >> 32 and s & 0xFFFFFFFF for s in steps)
