"""Host-side checks of tests/_dense_ref.py, the references and bounds of the dense / segment operator sweep
(tests/test_gpu_dense_ops.py): the numpy references agree with torch CPU fp64 autograd, every integer case of the sweep
stays inside the exactness domain, and the bounds are not tighter than correct fp32 arithmetic in any summation order."""
import numpy as np
import pytest
import torch

from tests import _dense_ref as R

F32, F64 = np.float32, np.float64


def _close(ref, want, what):
    """Within 1e-12 relative to S = sum |terms| (plus a denormal's worth where S is 0)."""
    err = np.abs(np.asarray(ref.value, dtype=F64) - want.detach().numpy())
    assert np.all(err <= 1e-12 * np.asarray(ref.S) + 1e-300), f'{what}: {float(err.max())}'


def test_long_double_is_wider_than_double():
    """The fp64 references are evaluated in long double: its unit roundoff must leave the fp64 bound its meaning."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63


@pytest.mark.parametrize('shape', [(1, 3, 2), (5, 1, 1), (17, 12, 7), (33, 40, 9)])
@pytest.mark.parametrize('bias', [True, False])
def test_linear_ref_matches_torch_autograd(shape, bias):
    x, w, b, g_y = R.linear_case(shape, bias, integer=False, dtype=F64)
    ref = R.linear_ref(x, w, b, g_y)
    tx, tw = (torch.from_numpy(a).requires_grad_(True) for a in (x, w))
    tb = torch.from_numpy(b).requires_grad_(True) if bias else None
    y = torch.nn.functional.linear(tx, tw, tb)
    y.backward(torch.from_numpy(g_y))
    _close(ref['y'], y, 'y')
    _close(ref['g_x'], tx.grad, 'g_x')
    _close(ref['g_w'], tw.grad, 'g_w')
    if bias:
        _close(ref['g_b'], tb.grad, 'g_b')
    assert ref['y'].n == shape[1] + bias and ref['g_x'].n == shape[2] and ref['g_w'].n == shape[0]


@pytest.mark.parametrize('sizes,lead,tail', [([0, 0, 5, 0, 1, 9, 2, 0], 0, 0), ([3], 0, 0), ([4, 11], 5, 5)])
def test_mean_pool_ref_matches_torch_autograd(sizes, lead, tail):
    h, ptr, g = R.pool_case(sizes, 6, integer=False, dtype=F64, lead=lead, tail=tail)
    ref = R.mean_pool_ref(h, ptr, g)
    th = torch.from_numpy(h).requires_grad_(True)
    rows = [th[ptr[k]:ptr[k + 1]].sum(0) / max(int(ptr[k + 1] - ptr[k]), 1) for k in range(len(sizes))]
    pooled = torch.stack(rows)
    pooled.backward(torch.from_numpy(g))
    _close(ref['pooled'], pooled, 'pooled')
    _close(ref['g_h'], th.grad, 'g_h')
    if lead:
        assert not ref['g_h'].value[:lead].any() and not ref['g_h'].value[-tail:].any()


@pytest.mark.parametrize('variant', ['sparse', 'single_segment', 'no_rows', 'pow2_counts'])
@pytest.mark.parametrize('mean', [False, True])
def test_segment_ref_matches_torch_autograd(variant, mean):
    data, ids, n_seg, g_out = R.segment_case(variant, 5, integer=False, dtype=F64)
    ref = R.segment_ref(data, ids, n_seg, mean, g_out)
    td, tid = torch.from_numpy(data).requires_grad_(True), torch.from_numpy(ids)
    out = torch.zeros((n_seg, 5), dtype=torch.float64).index_add_(0, tid, td)
    if mean:
        cnt = torch.zeros(n_seg, dtype=torch.float64).index_add_(0, tid, torch.ones(len(ids), dtype=torch.float64))
        out = out / cnt.clamp(min=1)[:, None]
    out.backward(torch.from_numpy(g_out))
    _close(ref['out'], out, 'out')
    _close(ref['g_data'], td.grad, 'g_data')
    if variant == 'pow2_counts' and mean:
        cnt = np.asarray(ref['out'].cnt)
        assert np.all((cnt & (cnt - 1)) == 0) and cnt.max() > 1


# ---- every integer case of the GPU sweep is inside the exactness domain (the references assert it themselves) --------
@pytest.mark.parametrize('shape', R.LINEAR_F32 + R.LINEAR_F32_LARGE)
def test_linear_f32_integer_cases_are_exact(shape):
    for bias in (True, False):
        x, w, b, g_y = R.linear_case(shape, bias, integer=True)
        ref = R.linear_ref(x, w, b, g_y, integer=True, values=False)
        assert max(float(r.S.max()) for r in ref.values()) < 2.0 ** 24
        assert np.abs(x).max() <= 4 and np.abs(w).max() <= 4 and np.abs(g_y).max() <= 4


@pytest.mark.parametrize('shape', R.LINEAR_F64)
def test_linear_f64_integer_cases_are_exact(shape):
    x, w, b, g_y = R.linear_case(shape, True, integer=True, dtype=F64)
    ref = R.linear_ref(x, w, b, g_y, integer=True, values=False)
    assert max(float(r.S.max()) for r in ref.values()) < 2.0 ** 53


@pytest.mark.parametrize('dtype', [F32, F64])
def test_pool_and_segment_integer_cases_are_exact(dtype):
    limit = R.EXACT_LIMIT[np.dtype(dtype)]
    for sizes in R.POOL_GRAPHS:
        for width in R.POOL_WIDTHS:
            h, ptr, g = R.pool_case(sizes, width, True, dtype)
            ref = R.mean_pool_ref(h, ptr, g, integer=True)
            assert ref['pooled'].S_sum.max() < limit
    h, ptr, g = R.pool_case(R.POOL_STRIDE_CASE['sizes'], R.POOL_STRIDE_CASE['width'], True, dtype)
    assert R.mean_pool_ref(h, ptr, g, integer=True)['pooled'].S_sum.max() < limit
    for variant in R.SEGMENT_VARIANTS:
        for width in R.SEGMENT_WIDTHS:
            data, ids, n_seg, g_out = R.segment_case(variant, width, True, dtype)
            assert R.segment_ref(data, ids, n_seg, True, g_out, integer=True)['out'].S_sum.max(initial=0.0) < limit
    for shape in R.SEGMENT_LOOPS:
        data, ids, n_seg, g_out = R.segment_loop_case(shape, True, dtype)
        assert R.segment_ref(data, ids, n_seg, False, g_out, integer=True)['out'].S_sum.max() < limit


def test_exact_domain_is_enforced():
    """A case outside the domain cannot pass as an exact one: the reference refuses it."""
    x = np.full((1, 2 ** 21), 4, dtype=F32)
    with pytest.raises(AssertionError, match='exactness limit'):
        R.linear_ref(x, x.copy(), None, np.ones((1, 1), dtype=F32), integer=True, values=False)


# ---- the bounds hold for correct fp32 arithmetic in several summation orders ----------------------------------------
def _sum_orders(prod, first=None):
    """fp32 sums of `prod` (fp32 terms, reduced over the last axis) forward, reversed and pairwise; `first`: a bias."""
    fwd = np.zeros(prod.shape[:-1], dtype=F32) if first is None else first.astype(F32).copy()
    for k in range(prod.shape[-1]):
        fwd = fwd + prod[..., k]
    rev = np.zeros(prod.shape[:-1], dtype=F32)
    for k in reversed(range(prod.shape[-1])):
        rev = rev + prod[..., k]
    pair = np.sum(prod, axis=-1, dtype=F32)
    if first is not None:
        rev, pair = rev + first.astype(F32), pair + first.astype(F32)
    return {'forward': fwd, 'reversed': rev, 'pairwise': pair}


@pytest.mark.parametrize('shape', R.LINEAR_F32_ROUNDED)
def test_gamma_bound_holds_for_fp32_sums_in_any_order(shape):
    x, w, b, g_y = R.linear_case(shape, True, integer=False)
    ref = R.linear_ref(x, w, b, g_y)
    evals = {
        'y': _sum_orders(x[:, None, :] * w[None, :, :], np.broadcast_to(b, (shape[0], shape[2]))),
        'g_x': _sum_orders(g_y[:, None, :] * w.T[None, :, :]),
        'g_w': _sum_orders(g_y.T[:, None, :] * x.T[None, :, :]),
        'g_b': _sum_orders(np.ascontiguousarray(g_y.T)),
    }
    for name, by_order in evals.items():
        for order, got in by_order.items():
            assert got.dtype == F32
            R.assert_rounded(got, ref[name], f'{shape} {name} {order}')


def test_gamma_bound_is_not_vacuous():
    """One dropped row of a 1100-row column sum is outside the bound (the gap of a max-norm tolerance)."""
    x, w, b, g_y = R.linear_case((1100, 12, 64), True, integer=False)
    ref = R.linear_ref(x, w, b, g_y)
    dropped = (g_y[:-1].astype(F64).T @ x[:-1].astype(F64)).astype(F32)
    with pytest.raises(AssertionError, match='outside gamma'):
        R.assert_rounded(dropped, ref['g_w'], 'one row dropped')


def test_mean_bounds_hold_for_fp32_division_and_reciprocal():
    """Integer rows through a mean: x / cnt and x * (1 / cnt) in fp32 are bit-exact for power-of-two counts and within
    3u of the exact mean elsewhere; standard-normal rows stay within gamma(n + 3) S in each summation order."""
    h, ptr, g = R.pool_case([0, 0, 37, 0, 1, 500, 2, 0], 33, True, F32)
    ref = R.mean_pool_ref(h, ptr, g, integer=True)
    total, cnt = ref['pooled'].total.astype(F32), np.asarray(ref['pooled'].cnt).astype(F32)
    R.assert_mean_exact(total / cnt, ref['pooled'], 'divide')
    R.assert_mean_exact(total * (F32(1) / cnt), ref['pooled'], 'reciprocal')
    gt, gc = ref['g_h'].total.astype(F32), np.asarray(ref['g_h'].cnt).astype(F32)
    R.assert_mean_exact(gt / gc, ref['g_h'], 'backward divide')
    R.assert_mean_exact(gt * (F32(1) / gc), ref['g_h'], 'backward reciprocal')
    with pytest.raises(AssertionError):
        R.assert_mean_exact(total / cnt * F32(1 + 2.0 ** -20), ref['pooled'], 'scaled')

    h, ptr, g = R.pool_case([37, 500, 2], 7, False, F32)
    ref = R.mean_pool_ref(h, ptr, g)
    for k in range(3):
        rows = np.ascontiguousarray(h[ptr[k]:ptr[k + 1]].T)
        for order, s in _sum_orders(rows).items():
            one = R.Ref(ref['pooled'].value[k], ref['pooled'].n[k], ref['pooled'].S[k])
            R.assert_rounded(s / F32(ptr[k + 1] - ptr[k]), one, f'graph {k} {order} divide')
            R.assert_rounded(s * (F32(1) / F32(ptr[k + 1] - ptr[k])), one, f'graph {k} {order} reciprocal')
