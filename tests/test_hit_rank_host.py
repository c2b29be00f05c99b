"""Per-hit ranks, the host side (CPU): the numpy restatement (tests/_hit_rank_ref.py) against the reference's own
construction - a descending sort, then range(len) - on tie-free values, hand-written expectations for ties, signed
zeros, infinities and NaN, the order relation of csrc/hit_ranks.h compiled alone with the host compiler against the
numpy one, and the new exports, wrappers and keywords."""
import inspect
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _hit_rank_ref as ref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'pointvs_amd' / 'csrc'
CXX = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
NAN, INF = float('nan'), float('inf')


def _sorted_positions(values):
    """The reference's construction (hotspot.py:183-191): sort the atoms of one structure by value, descending, and
    number them 0.. in that order; NaN atoms are not part of the frame. pandas where it imports, else a stable
    argsort - on tie-free values the two agree."""
    values = np.asarray(values, dtype=np.float32)
    have = np.nonzero(~np.isnan(values))[0]
    try:
        import pandas as pd
        df = pd.DataFrame({'atom': have, 'value': values[have]}).sort_values(by='value', ascending=False)
        df['rank'] = range(len(df))
        order = df['atom'].to_numpy()
    except ImportError:
        order = have[np.argsort(-values[have], kind='stable')]
    out = np.full(len(values), np.nan, dtype=np.float32)
    out[order] = np.arange(len(order), dtype=np.float32)
    return out


@pytest.mark.parametrize('n_lig, n_rec, nan_share', [(0, 1, 0.0), (5, 40, 0.0), (17, 130, 0.4), (64, 7, 0.9)])
def test_tie_free_ranks_are_the_positions_of_the_descending_sort(n_lig, n_rec, nan_share):
    rng = np.random.default_rng(n_lig * 1000 + n_rec)
    values = rng.permutation(n_lig + n_rec).astype(np.float32) - 20          # distinct
    values[n_lig:][rng.random(n_rec) < nan_share] = np.nan
    lig, row = values[:n_lig], values[n_lig:]
    # the edge_attention form: protein atoms alone
    alone = ref.hit_value_ranks(row[None], None, None, None, *ref.fresh_accumulators(n_rec))
    assert alone[1] is None and np.array_equal(alone[0][0], _sorted_positions(row), equal_nan=True)
    # the cam / atom_masking form: ranked over the whole complex, the ligand rows dropped afterwards
    ptr = np.array([0, n_lig], dtype=np.int32)
    both = ref.hit_value_ranks(row[None], lig, ptr, np.full(n_lig, -7, dtype=np.float32), *ref.fresh_accumulators(n_rec))
    whole = _sorted_positions(values)
    assert np.array_equal(both[1], whole[:n_lig]) and np.array_equal(both[0][0], whole[n_lig:], equal_nan=True)
    have = ~np.isnan(row)
    assert np.array_equal(both[3], have.astype(np.int32)) and np.array_equal(both[2][have], whole[n_lig:][have])


def test_ties_zeros_infinities_and_nan():
    r = ref.ranks_of
    assert r([]).shape == (0,)
    assert np.array_equal(r([3, 3, 3, 3]), [0, 1, 2, 3])                                  # one value: by position
    assert np.array_equal(r([1, 5, 1, 5, 2]), [3, 0, 4, 1, 2])
    assert np.array_equal(r([-0.0, 0.0, -1, 0.0, -0.0]), [0, 1, 4, 2, 3])                # -0.0 == +0.0
    assert np.array_equal(r([-INF, INF, 0, INF, -INF]), [3, 0, 2, 1, 4])                 # ordinary values
    assert np.array_equal(r([NAN, 2, NAN, 2, 7]), [NAN, 1, NAN, 2, 0], equal_nan=True)   # a NaN is no candidate
    assert np.isnan(r([NAN, NAN])).all()
    # the ligand stands before the receptor at equal values; an invalid hit is a row of NaN
    rows = np.array([[1, 2, NAN], [1, 2, 3], [4, 4, 4]], dtype=np.float32)
    lig_val = np.array([2, 1, 9, 9], dtype=np.float32)
    lig_ptr = np.array([0, 2, 1, 1], dtype=np.int32)                                      # hit 1 descends, hit 2 is empty
    got = ref.hit_value_ranks(rows, lig_val, lig_ptr, np.full(4, -7, dtype=np.float32), *ref.fresh_accumulators(3))
    assert np.array_equal(got[0], [[3, 1, NAN], [NAN] * 3, [0, 1, 2]], equal_nan=True)
    assert np.array_equal(got[1], [0, 2, -7, -7])
    assert np.array_equal(got[2], [3, 2, 2]) and np.array_equal(got[3], [2, 2, 1]) and np.array_equal(got[4], [3, 1, 2])
    too_wide = np.array([0, ref.MAX_LIGAND + 1], dtype=np.int32)
    assert not ref.hit_ok(too_wide, 0) and ref.hit_ok(np.array([0, ref.MAX_LIGAND]), 0)
    assert not ref.hit_ok(np.array([-1, 3]), 0)


# Prints "<i> <j> <before(i at 0, j at 1)> <before(i at 1, j at 0)>" for every pair of the table, the tile and the
# verdicts on three ligand tables.
PROGRAM = r'''
#include "hit_ranks.h"
#include <math.h>
#include <stdio.h>
int main() {
    const float table[] = {0.0f, -0.0f, 1.0f, -1.0f, 2.5f, INFINITY, -INFINITY, NAN, 1e-45f, 3.4e38f};
    const int n = (int)(sizeof(table) / sizeof(table[0]));
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j)
            printf("%d %d %d %d\n", i, j, pvs_rank_before(table[i], 0, table[j], 1) ? 1 : 0,
                   pvs_rank_before(table[i], 1, table[j], 0) ? 1 : 0);
    printf("tile %d\n", (int)kPvsRankTile);
    const int32_t ptr[] = {0, 1024, 2049, 2040, -3, 5};
    for (int h = 0; h < 5; ++h) {
        const PvsRankHit hit = pvs_rank_hit(ptr, h);
        printf("hit %d %d %d\n", h, hit.a0, hit.n);
    }
    const PvsRankHit none = pvs_rank_hit(nullptr, 3);
    printf("null %d %d\n", none.a0, none.n);
    return 0;
}
'''
TABLE = [0.0, -0.0, 1.0, -1.0, 2.5, INF, -INF, NAN, 1e-45, 3.4e38]


def test_the_header_alone_gives_the_numpy_relation(tmp_path):
    assert CXX is not None, 'the order relation is checked with the host C++ compiler; none found'
    (tmp_path / 'main.cpp').write_text(PROGRAM)
    exe = tmp_path / 'hit_ranks_probe'
    out = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', str(CSRC), str(tmp_path / 'main.cpp'),
                          '-o', str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    res = subprocess.run([str(exe)], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    lines = res.stdout.splitlines()
    n = len(TABLE)
    values = np.array(TABLE, dtype=np.float32)
    for line in lines[:n * n]:
        i, j, first, second = map(int, line.split())
        assert first == ref.before(values[i], 0, values[j], 1), line
        assert second == ref.before(values[i], 1, values[j], 0), line
    from pointvs_amd import functional as PF
    assert lines[n * n] == f'tile {PF.HIT_RANK_TILE}'
    # 1024 atoms: a hit; 1025: none; descending: none; negative: none
    assert lines[n * n + 1:] == ['hit 0 0 1024', 'hit 1 0 -1', 'hit 2 0 -1', 'hit 3 0 -1', 'hit 4 0 -1', 'null 0 0']
    header = (CSRC / 'hit_ranks.h').read_text()
    assert 'hip/' not in header and 'common.h' not in header


def test_exports_wrappers_and_keywords():
    from pointvs_amd import _lib
    from pointvs_amd import functional as PF
    from pointvs_amd.screening import ScreeningSweep
    header = (ROOT / 'include' / 'pvs_egnn.h').read_text()
    declared = set(re.findall(r'\b(pvs_[a-z0-9_]+)\s*\(', header))
    for name, n_args in (('pvs_hit_value_ranks', 11), ('pvs_hit_rows_accumulate', 7)):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name), name
        assert len(_lib._PROTOTYPES[name][1]) == n_args
    assert _lib.lib().pvs_version() == 113 and _lib.MIN_VERSION == 113
    assert callable(PF.hit_value_ranks) and callable(PF.hit_rows_accumulate)
    assert isinstance(PF.HIT_RANK_TILE, int) and PF.HIT_RANK_TILE >= 256 and PF.HIT_RANK_TILE % 256 == 0
    assert re.search(r'kPvsRankTile\s*=\s*%d\b' % PF.HIT_RANK_TILE, (CSRC / 'hit_ranks.h').read_text())
    params = inspect.signature(ScreeningSweep.receptor_hotspots).parameters
    want = dict(gnn_layer=1, scores_file=None, per_hit=False, attribution='edge_attention', column=None,
                ligand_scores_file=None, atoms='contacts', sigmoid=None, use_rank=False, top=None)
    assert {k: p.default for k, p in params.items() if k not in ('self', 'items')} == want
    assert list(params)[:2] == ['self', 'items'] and list(params)[2:] == list(want)
    makefile = (CSRC / 'Makefile').read_text()
    assert 'hit_ranks.hip' in makefile and 'hit_ranks.h ' in makefile
