"""PF.segment_argmax (pvs_segment_argmax): the best pose of every ligand. Segments around the wavefront's 64 lanes,
planted ties (same lane, neighbouring lanes, first and last row) and non-finite scores, against a numpy restatement of
the rules; two calls give the same bits."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 63, 64, 65, 129, 1000)


def _reference(scores, seg_ptr, column):
    """The larger value wins, equal values go to the lower row (np.argmax: the first of the maxima; -0.0 == +0.0), a NaN
    never beats a number (masked out first), -inf is a score; no usable row: -1 and NaNs."""
    n_seg = len(seg_ptr) - 1
    best = np.full(n_seg, -1, dtype=np.int32)
    rows = np.full((n_seg, scores.shape[1]), np.nan, dtype=np.float32)
    for s in range(n_seg):
        col = scores[seg_ptr[s]:seg_ptr[s + 1], column]
        usable = np.flatnonzero(~np.isnan(col))
        if usable.size:
            best[s] = usable[np.argmax(col[usable])]
            rows[s] = scores[seg_ptr[s] + best[s]]
    return best, rows


def _check(scores, seg_ptr, column):
    from pointvs_amd import functional as PF
    dev_scores, dev_ptr = torch.from_numpy(scores).cuda(), torch.from_numpy(seg_ptr).cuda()
    best, rows = PF.segment_argmax(dev_scores, dev_ptr, column)
    again = PF.segment_argmax(dev_scores, dev_ptr, column)
    want_best, want_rows = _reference(scores, seg_ptr, column)
    assert best.dtype == torch.int32 and rows.shape == (len(seg_ptr) - 1, scores.shape[1])
    assert np.array_equal(best.cpu().numpy(), want_best)
    got_rows = rows.cpu().numpy()
    assert np.array_equal(np.isnan(got_rows), np.isnan(want_rows))
    assert np.array_equal(got_rows.view(np.int32)[~np.isnan(want_rows)], want_rows.view(np.int32)[~np.isnan(want_rows)])
    assert torch.equal(best, again[0]) and torch.equal(rows.view(torch.int32), again[1].view(torch.int32))
    return want_best


def _random(lengths, n_cols, seed):
    rng = np.random.default_rng(seed)
    seg_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    return rng.standard_normal((int(seg_ptr[-1]), n_cols)).astype(np.float32), seg_ptr


@pytest.mark.parametrize('column', [0, 1])
@pytest.mark.parametrize('n_cols', [1, 2, 4])
def test_lengths_around_the_wavefront(n_cols, column):
    if column >= n_cols:
        column = n_cols - 1
    scores, seg_ptr = _random(LENGTHS, n_cols, seed=10 * n_cols + column)
    best = _check(scores, seg_ptr, column)
    assert best[0] == -1 and best[1] == 0 and (best[1:] >= 0).all()


@pytest.mark.parametrize('n_cols,column', [(1, 0), (2, 1), (4, 0), (4, 1)])
def test_planted_ties_go_to_the_lower_row(n_cols, column):
    """Eight segments of 1000 rows and more: the maximum twice in one lane (rows i, i + 64), in neighbouring lanes
    (i, i + 1), in the first and the last row, in every row (all equal), as -0.0 before +0.0."""
    lengths = (1000, 1000, 1000, 129, 65, 64, 200, 3)
    scores, seg_ptr = _random(lengths, n_cols, seed=77 + n_cols + column)
    col = scores[:, column]
    top = np.float32(50.0)
    col[seg_ptr[0] + 137], col[seg_ptr[0] + 137 + 64] = top, top
    col[seg_ptr[1] + 700], col[seg_ptr[1] + 701] = top, top
    col[seg_ptr[2]], col[seg_ptr[3] - 1] = top, top
    col[seg_ptr[3] + 64], col[seg_ptr[3] + 128], col[seg_ptr[3] + 65] = top, top, top
    col[seg_ptr[4]:seg_ptr[5]] = np.float32(-3.5)
    col[seg_ptr[5] + 63], col[seg_ptr[5] + 62] = top, top
    col[seg_ptr[6]:seg_ptr[7]] = np.float32(-7.0)
    col[seg_ptr[6] + 150], col[seg_ptr[6] + 90] = np.float32(0.0), np.float32(-0.0)
    best = _check(scores, seg_ptr, column)
    assert best.tolist()[:7] == [137, 700, 0, 64, 0, 62, 90]


@pytest.mark.parametrize('n_cols,column', [(1, 0), (2, 1), (4, 0), (4, 1)])
def test_non_finite_scores(n_cols, column):
    """All -inf (a score: row 0 wins), +inf present, NaNs before and after the maximum, all NaN (no best pose), NaNs
    and -inf only (-inf beats a NaN), an empty segment between them."""
    lengths = (130, 70, 300, 65, 0, 129, 1)
    scores, seg_ptr = _random(lengths, n_cols, seed=5 + n_cols + column)
    col = scores[:, column]
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    col[seg_ptr[0]:seg_ptr[1]] = -inf
    col[seg_ptr[1] + 66], col[seg_ptr[1] + 3] = inf, np.float32(1e30)
    seg2 = col[seg_ptr[2]:seg_ptr[3]]
    seg2[:] = np.minimum(seg2, 3.0)
    seg2[[0, 5, 63, 64, 199, 201, 299]] = nan
    seg2[200] = np.float32(9.0)
    col[seg_ptr[3]:seg_ptr[4]] = nan
    col[seg_ptr[5]:seg_ptr[6]] = nan
    col[seg_ptr[5] + 100], col[seg_ptr[5] + 128] = -inf, -inf
    col[seg_ptr[6]] = nan
    if n_cols > 1:          # NaNs in the other columns neither win nor lose anything: they are copied
        scores[seg_ptr[2] + 200, 1 - column] = nan
    best = _check(scores, seg_ptr, column)
    assert best.tolist() == [0, 66, 200, -1, -1, 100, -1]


def test_refusals_and_an_empty_call():
    from pointvs_amd import functional as PF
    scores = torch.randn(5, 2).cuda()
    ptr = torch.tensor([0, 5], dtype=torch.int32).cuda()
    for column in (-1, 2):
        with pytest.raises(RuntimeError, match='column'):
            PF.segment_argmax(scores, ptr, column)
    with pytest.raises(TypeError, match='fp32 only'):
        PF.segment_argmax(scores.double(), ptr)
    with pytest.raises(ValueError, match='int32'):
        PF.segment_argmax(scores, ptr.long())
    best, rows = PF.segment_argmax(scores[:0], torch.zeros(4, dtype=torch.int32).cuda())
    assert best.tolist() == [-1, -1, -1] and bool(torch.isnan(rows).all()) and rows.shape == (3, 2)
    best, rows = PF.segment_argmax(scores, ptr[:1])
    assert best.shape == (0,) and rows.shape == (0, 2)
