"""Test helper: a numpy restatement of the per-hit ranks (pvs_hit_value_ranks, PF.hit_value_ranks) and of the
accumulation over rows (pvs_hit_rows_accumulate). The candidates of a hit are its ligand values (position = packed
order), then its receptor values (position = n_lig + j), NaN left out; u stands before v iff u > v, or u == v and u's
position is lower; a candidate's rank is the number of candidates of its hit that stand before it."""
import numpy as np

MAX_LIGAND = 1024


def before(u, pu, v, pv):
    """Does (u at position pu) stand before (v at position pv)? Plain IEEE comparisons: NaN never, -0.0 == +0.0."""
    u, v = np.float32(u), np.float32(v)
    return bool(u > v or (u == v and pu < pv))


def ranks_of(values):
    """float32 ranks of one hit's candidates in position order (NaN where the value is NaN). One loop over the
    candidates, the count over the others as an array expression of `before`."""
    values = np.asarray(values, dtype=np.float32)
    pos = np.arange(len(values))
    out = np.full(len(values), np.nan, dtype=np.float32)
    with np.errstate(invalid='ignore'):
        for c in range(len(values)):
            if not np.isnan(values[c]):
                out[c] = np.float32(int(((values > values[c]) | ((values == values[c]) & (pos < c))).sum()))
    return out


def accumulate(rows, rec_sum, rec_count, rec_max):
    """Copies of the three accumulators updated with rows [n_hits, n_rec] in hit order (the contact-attention rule:
    NaN skipped, float64 sums, +0.0 above -0.0 in the maximum)."""
    rec_sum, rec_count = np.array(rec_sum, dtype=np.float64), np.array(rec_count, dtype=np.int32)
    rec_max = np.array(rec_max, dtype=np.float32)
    for j in range(rows.shape[1]):
        for p in range(rows.shape[0]):
            v = rows[p, j]
            if not np.isnan(v):
                rec_sum[j] = rec_sum[j] + np.float64(v)
                rec_count[j] += 1
                if np.isnan(rec_max[j]) or v > rec_max[j] or (v == rec_max[j] and np.signbit(rec_max[j])):
                    rec_max[j] = v
    return rec_sum, rec_count, rec_max


def fresh_accumulators(n_rec):
    return np.zeros(n_rec, dtype=np.float64), np.zeros(n_rec, dtype=np.int32), np.full(n_rec, np.nan, dtype=np.float32)


def hit_ok(lig_ptr, h):
    a0, a1 = int(lig_ptr[h]), int(lig_ptr[h + 1])
    return a0 >= 0 and a1 >= a0 and a1 - a0 <= MAX_LIGAND


def hit_value_ranks(rows, lig_val, lig_ptr, lig_rank, rec_sum, rec_count, rec_max):
    """Returns (row_rank, lig_rank, rec_sum, rec_count, rec_max) after one call; lig_rank and the accumulators are
    copies of the arrays given, updated. lig_val / lig_ptr / lig_rank None: the receptor atoms alone (lig_rank None)."""
    rows = np.asarray(rows, dtype=np.float32)
    n_hits, n_rec = rows.shape
    row_rank = np.full((n_hits, n_rec), np.nan, dtype=np.float32)
    lig_rank = None if lig_val is None else np.array(lig_rank, dtype=np.float32)
    for h in range(n_hits):
        if lig_val is None:
            row_rank[h] = ranks_of(rows[h])
        elif hit_ok(lig_ptr, h):
            a0, a1 = int(lig_ptr[h]), int(lig_ptr[h + 1])
            got = ranks_of(np.concatenate([lig_val[a0:a1], rows[h]]))
            lig_rank[a0:a1], row_rank[h] = got[:a1 - a0], got[a1 - a0:]
    return (row_rank, lig_rank) + accumulate(row_rank, rec_sum, rec_count, rec_max)
