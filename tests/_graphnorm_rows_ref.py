"""fp64 torch restatement of GraphNorm over a leading row range (PvsGraph.n_norm_rows_dev), shared by
tests/test_graphnorm_rows_host.py (pinned there against the oracle and against autograd) and the GPU tests.

y [N_cap, H], n with 0 <= n <= N_cap:
    mean[c] = mean of y[:n, c]                                   (n = 0: 0)
    var[c]  = mean of (y[:n, c] - mean_scale[c] * mean[c])^2     (n = 0: 0)
    out     = weight * (y - mean_scale * mean) / sqrt(var + eps) + bias        for ALL N_cap rows
Rows >= n are never read for the statistics (they are sliced away, not multiplied by zero: NaN there stays there).
"""
import torch

EPS = 1e-5      # torch_geometric GraphNorm's default


def stats(y, mean_scale, n):
    """(mean [H], var [H]) in the dtype of y; zeros for n = 0."""
    if n == 0:
        zero = torch.zeros(y.shape[1], dtype=y.dtype, device=y.device)
        return zero, zero.clone()
    head = y[:n]
    mean = head.mean(dim=0)
    var = (head - mean_scale * mean).pow(2).mean(dim=0)
    return mean, var


def forward(y, weight, bias, mean_scale, n, eps=EPS):
    mean, var = stats(y, mean_scale, n)
    return weight * (y - mean_scale * mean) / (var + eps).sqrt() + bias


def closed_form_backward(y, weight, mean_scale, n, g_out, eps=EPS):
    """The gradient as the kernels form it: S1 / S2 over ALL rows, the coefficients with n, the two statistics terms for
    rows < n only. Returns dict(y, weight, bias, mean_scale, bias_in_front): bias_in_front = the column sums of g_y (the
    gradient of a bias added to y), in closed form."""
    n_cap, hidden = y.shape
    mean, var = stats(y, mean_scale, n)
    shift = mean * mean_scale
    rstd = 1.0 / (var + eps).sqrt()
    s1 = g_out.sum(dim=0)
    s2 = (g_out * y).sum(dim=0) - shift * s1
    g_var = -0.5 * weight * rstd ** 3 * s2
    inv_n = 1.0 / n if n > 0 else 0.0
    sum_cc = n * (mean - shift)
    sum_gc = weight * rstd * s1 + g_var * 2.0 * sum_cc * inv_n
    g_shift = -sum_gc
    g_mean = g_shift * mean_scale if n > 0 else torch.zeros_like(s1)
    coef_a, coef_b, coef_c = weight * rstd, 2.0 * g_var * inv_n, g_mean * inv_n
    g_y = g_out * coef_a
    g_y[:n] = g_y[:n] + (y[:n] - shift) * coef_b + coef_c
    return dict(y=g_y, weight=s2 * rstd, bias=s1, mean_scale=g_shift * mean,
                bias_in_front=sum_gc * (1.0 - mean_scale) if n > 0 else sum_gc)


def autograd_backward(y, weight, bias, mean_scale, n, g_out, eps=EPS):
    """The same gradients through torch.autograd."""
    leaves = [t.detach().clone().requires_grad_(True) for t in (y, weight, bias, mean_scale)]
    out = forward(leaves[0], leaves[1], leaves[2], leaves[3], n, eps)
    g = torch.autograd.grad(out, leaves, g_out, allow_unused=True)
    g = [torch.zeros_like(t) if gi is None else gi for gi, t in zip(g, leaves)]
    return dict(y=g[0], weight=g[1], bias=g[2], mean_scale=g[3], bias_in_front=g[0].sum(dim=0))


def case(n_cap, hidden, seed=0):
    """(y, weight, bias, mean_scale, g_out) fp64, away from the defaults (weight 1, bias 0, mean_scale 1) and from zero
    means, so that no term of the gradient vanishes."""
    gen = torch.Generator().manual_seed(1000 * n_cap + hidden + seed)
    rnd = lambda *shape: torch.randn(*shape, generator=gen, dtype=torch.float64)
    y = rnd(n_cap, hidden) * 1.5 + rnd(hidden)
    return y, 1.0 + 0.3 * rnd(hidden), 0.2 * rnd(hidden), 1.0 + 0.25 * rnd(hidden), rnd(n_cap, hidden)
