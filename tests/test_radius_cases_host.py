"""The hand-made radius-graph cases (tests/_radius_cases.py) are what they claim to be: the blocked reference equals
the oracle, the 1e-7 band pairs lie on both sides of the decision, and every wrong decision rule a builder could take
fails on at least one committed case. No GPU."""
import numpy as np
import pytest

from tests import _radius_cases as rc
from tests._golden import GOLDEN_DIR

EDGE_FILES = sorted(p.stem for p in GOLDEN_DIR.glob('edges_*.npz'))


def _same_as_oracle(pos, bp, inter, intra):
    from oracle.generate_edges_oracle import generate_edges
    _, (rows, cols), attrs = generate_edges(pos, bp, inter, intra, prune=False)
    got = rc.reference_edges(pos, bp, inter, intra, block=48)      # several row blocks, the last one partial
    assert np.array_equal(got[0], rows) and np.array_equal(got[1], cols) and np.array_equal(got[2], attrs)
    return len(rows)


@pytest.mark.parametrize('name', EDGE_FILES)
def test_reference_edges_equals_the_oracle_on_the_golden_structures(name):
    z = np.load(GOLDEN_DIR / f'{name}.npz')
    _same_as_oracle(z['xyz'], z['bp'], float(z['inter']), float(z['intra']))


@pytest.mark.parametrize('seed,inter,intra', [(1, 4.0, 2.0), (2, 2.5, 3.5)])
def test_reference_edges_equals_the_oracle_on_random_structures(seed, inter, intra):
    rng = np.random.RandomState(seed)
    pos = (rng.rand(130, 3) * 8.0).astype(np.float32)
    bp = (rng.rand(130) < 0.8).astype(np.int64)
    assert _same_as_oracle(pos, bp, inter, intra) > 100


def test_sqdist_accumulates_like_the_oracles_cdist():
    from oracle.generate_edges_oracle import cdist_euclidean
    pos = rc.upper_band_graph()[0]
    assert np.array_equal(np.sqrt(rc.sqdist(pos, pos)), cdist_euclidean(pos))
    assert all(i // 64 != j // 64 for _, i, j in rc.UPPER_PROBES)      # every probe pair spans two 64-column chunks
    bp = rc.upper_band_graph()[1]
    assert [(int(bp[i]), int(bp[j])) for _, i, j in rc.UPPER_PROBES] == [(0, 1), (1, 1), (0, 0)]
    assert rc.ulps(1.0, 3) == 1.0 + 3 * 2.0 ** -52 and rc.ulps(1.0, -2) == 1.0 - 2 * 2.0 ** -53 and rc.ulps(2.5, 0) == 2.5


def test_zero_band_pairs_lie_in_the_band_on_both_sides_of_the_decision():
    triples, decision, s, n_band, n_differ = rc.zero_band_pairs()
    assert triples.dtype == np.float32 and len(triples) <= 24
    again = rc.sqdist(np.zeros((1, 3), dtype=np.float32), triples)[0]
    assert np.array_equal(again, s)
    assert ((s >= 1e-14 * (1 - rc.BAND)) & (s <= 1e-14 * (1 + rc.BAND))).all()
    assert np.array_equal(decision, np.sqrt(s) > 1e-7)
    assert decision.any() and (~decision).any()
    differs = decision != (s > rc.ZERO * rc.ZERO)
    print(f'1e-7 band: {n_band} triples on the grid, {n_differ} differ from s > 1e-7*1e-7; kept {len(triples)}, '
          f'{int(differs.sum())} of them differ')
    assert differs.sum() >= 1
    assert len(np.unique(s)) >= 20          # not one double over and over


def test_the_literal_1e_14_is_not_a_wrong_rule():
    """Why naive_rules squares the bound instead of writing 1e-14: sqrt(s) > 1e-7 and s > 1e-14 agree at every double
    (both are monotone in s, and they switch between the same two neighbours), whereas fl(1e-7 * 1e-7) is one ulp
    below 1e-14, so `s > r*r` admits s == 1e-14, whose square root rounds to exactly 1e-7."""
    s = np.array([rc.ulps(1e-14, k) for k in range(-64, 65)])
    assert np.array_equal(np.sqrt(s) > 1e-7, s > 1e-14)
    assert 1e-7 * 1e-7 == rc.ulps(1e-14, -1) and np.sqrt(np.float64(1e-14)) == 1e-7


def _committed_decisions():
    """(s, r) of every probed decision of the GPU tests' radius sweeps (tests/test_gpu_radius_decisions.py a, b, d)."""
    pos, bp = rc.upper_band_graph()
    sweeps = list(rc.upper_band_sweeps(pos, bp))
    for n_lig, n_rec in rc.POSE_SHAPES:
        sweeps += rc.pose_sweeps(*rc.pose_case(n_lig, n_rec))
    s = [sw[2] for sw in sweeps]
    r = [sw[3] if sw[1] == 'inter' else sw[4] for sw in sweeps]
    zs = rc.zero_band_batch()[3]
    s += list(zs)
    r += [rc.ZERO_BATCH_RADIUS] * len(zs)
    return np.array(s, dtype=np.float64), np.array(r, dtype=np.float64)


@pytest.mark.parametrize('rule', sorted(rc.naive_rules))
def test_every_naive_rule_fails_on_a_committed_case(rule):
    s, r = _committed_decisions()
    want = rc.oracle_rule(s, r)
    got = rc.naive_rules[rule](s, r)
    wrong = int((got != want).sum())
    print(f'{rule}: wrong on {wrong} of {len(s)} committed decisions')
    assert want.any() and (~want).any()
    assert wrong >= 1
