"""fp64 torch restatement of GraphNorm per node segment (the layer flag PVS_GRAPHNORM_SEGMENTS), shared by
tests/test_graphnorm_segments_host.py (pinned there against tests/_graphnorm_rows_ref.py applied per segment and
against the oracle's GraphNorm on each graph alone) and the GPU tests.

y [N_cap, H], seg_ptr [S + 1] integers. Every entry is clamped to [0, N_cap]; segment s = rows [a_s, e_s) with
a_s = clamp(seg_ptr[s]), e_s = clamp(seg_ptr[s + 1]), length n_s = max(0, e_s - a_s):
    mean[s, c] = mean of y[a_s:e_s, c]                                       (n_s = 0: 0)
    var[s, c]  = mean of (y[a_s:e_s, c] - mean_scale[c] * mean[s, c])^2      (n_s = 0: 0)
    out[r]     = weight * (y[r] - mean_scale * mean[s]) / sqrt(var[s] + eps) + bias     for r in segment s
    out[r]     = weight * y[r] / sqrt(eps) + bias                                       for r in no segment (padding:
                 the rows in front of a_0 and at / behind e_{S-1}), the n = 0 contract of the row-count route
Rows of no segment are never read for the statistics (NaN there stays there and reaches no segment).
"""
import torch

EPS = 1e-5      # torch_geometric GraphNorm's default


def clamped(seg_ptr, n_cap):
    """The table as the kernels read it: a list of (start, length) per segment."""
    ptr = [min(max(int(v), 0), int(n_cap)) for v in seg_ptr]
    return [(ptr[s], max(0, ptr[s + 1] - ptr[s])) for s in range(len(ptr) - 1)]


def stats(y, mean_scale, seg_ptr):
    """[S, 2H] in the dtype of y: per segment the mean, then the variance around mean_scale * mean; zeros for an
    empty segment."""
    hidden = y.shape[1]
    out = torch.zeros((len(seg_ptr) - 1, 2 * hidden), dtype=y.dtype, device=y.device)
    for s, (a, n) in enumerate(clamped(seg_ptr, y.shape[0])):
        if n == 0:
            continue
        rows = y[a:a + n]
        mean = rows.mean(dim=0)
        out[s, :hidden] = mean
        out[s, hidden:] = (rows - mean_scale * mean).pow(2).mean(dim=0)
    return out


def forward(y, weight, bias, mean_scale, seg_ptr, eps=EPS):
    """GraphNorm of every row with its own segment's statistics; rows of no segment with mean = var = 0. Segments are
    expected non-overlapping (a node offset table); where two overlap the later one wins here, which nothing relies on."""
    hidden = y.shape[1]
    st = stats(y, mean_scale, seg_ptr)
    mean = torch.zeros_like(y)
    var = torch.zeros_like(y)
    for s, (a, n) in enumerate(clamped(seg_ptr, y.shape[0])):
        mean[a:a + n] = st[s, :hidden]
        var[a:a + n] = st[s, hidden:]
    return weight * (y - mean_scale * mean) / (var + eps).sqrt() + bias


def owned(seg_ptr, n_cap):
    """bool [N_cap]: the rows that belong to a segment."""
    mask = torch.zeros(n_cap, dtype=torch.bool)
    for a, n in clamped(seg_ptr, n_cap):
        mask[a:a + n] = True
    return mask
