"""Plain numpy references, error bounds and the shared shape tables of the operator-level tests of the dense and
segment operators (tests/test_gpu_dense_ops.py on the GPU, tests/test_dense_ref_host.py without one).

Every reference returns, per output element, the value, the number of addends `n` and `S = sum |terms|`; the two
kinds of comparison are derived from those alone, never from a measured error:

exact    Inputs are integers in [-4, 4] stored as floats. While S < 2**24 (fp32; 2**53 for fp64) every product and every
         partial sum is an integer below the limit, so it is exactly representable whatever the summation order, with or
         without FMA or MFMA: the kernel must return the reference bit for bit. A mean of `cnt` rows is exact too where
         cnt is a power of two (or <= 1); elsewhere the sum is exact and the result carries the roundings of 1/cnt and of
         the multiply or divide: |got - sum/cnt| <= 3 u |sum/cnt|.
rounded  Standard-normal inputs: |got - ref| <= gamma(n + 3) S per element, gamma(k) = k u / (1 - k u): the bound of a
         dot product in any order, with or without FMA (Higham, Accuracy and Stability of Numerical Algorithms, 3.1);
         the + 3 covers the bias, the rounding of 1/cnt and the final scale.

u = 2**-24 (fp32), 2**-53 (fp64). The references are evaluated one precision up (fp64 for fp32 data, long double for
fp64 data; integers go through int64), so their own error is far below the bound.
"""
from collections import namedtuple

import numpy as np

U = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
EXACT_LIMIT = {np.dtype(np.float32): 2.0 ** 24, np.dtype(np.float64): 2.0 ** 53}

# value: the reference (fp64 or long double); n: addends per element (array or int); S: sum of |terms| of `value`;
# S_sum / total / cnt (mean operators only): sum of |terms| and value of the un-divided sum, and the divisor
Ref = namedtuple('Ref', 'value n S S_sum total cnt', defaults=(None, None, None))


def unit(dtype):
    return U[np.dtype(dtype)]


def gamma(k, u):
    k = np.asarray(k, dtype=np.float64)
    return k * u / (1.0 - k * u)


def wide_dtype(dtype):
    """The precision the reference of `dtype` data is evaluated in."""
    return np.float64 if np.dtype(dtype) == np.float32 else np.longdouble


def make_data(rng, shape, dtype, integer):
    """Uniform integers in [-4, 4] stored as floats (exact mode) or standard-normal values (rounded mode)."""
    if integer:
        return rng.integers(-4, 5, size=shape).astype(dtype)
    return rng.standard_normal(size=shape).astype(dtype)


def _assert_exact_domain(S, dtype, what):
    limit = EXACT_LIMIT[np.dtype(dtype)]
    top = float(np.max(S)) if np.size(S) else 0.0
    assert top < limit, f'{what}: S = {top} reaches the exactness limit {limit}: not an exact-mode case'


def _mm(a, b, integer, wide):
    if integer:                                    # exact whatever the size: no floating point in the reference
        return np.matmul(a.astype(np.int64), b.astype(np.int64)).astype(wide)
    return np.matmul(a.astype(wide), b.astype(wide))


def _abs_mm(a, b):
    return np.matmul(np.abs(a).astype(np.float64), np.abs(b).astype(np.float64))


# ---- linear: y = x W^T + b ------------------------------------------------------------------------------------------
def linear_ref(x, w, b, g_y, integer=False, values=True):
    """x [N, K], w [C, K], b [C] or None, g_y [N, C] -> {'y', 'g_x', 'g_w', 'g_b'}: Ref each ('g_b' only with a bias).
    integer=True: int64 products, and every S is asserted to stay below the exactness limit of x.dtype.
    values=False: only n and S (the products of the values are skipped)."""
    wide = wide_dtype(x.dtype)
    n_rows, k_in = x.shape
    c_out = w.shape[0]
    out = {}
    S = _abs_mm(x, w.T) + (0.0 if b is None else np.abs(b).astype(np.float64)[None, :])
    v = None
    if values:
        v = _mm(x, w.T, integer, wide) + (0 if b is None else b.astype(wide)[None, :])
    out['y'] = Ref(v, k_in + (b is not None), S)
    out['g_x'] = Ref(_mm(g_y, w, integer, wide) if values else None, c_out, _abs_mm(g_y, w))
    out['g_w'] = Ref(_mm(g_y.T, x, integer, wide) if values else None, n_rows, _abs_mm(g_y.T, x))
    if b is not None:
        out['g_b'] = Ref(g_y.astype(np.int64 if integer else wide).sum(axis=0).astype(wide) if values else None, n_rows,
                         np.abs(g_y).astype(np.float64).sum(axis=0))
    if integer:
        for name, r in out.items():
            _assert_exact_domain(r.S, x.dtype, f'linear {x.shape} x {w.shape} {name}')
    return out


def linear_case(shape, bias, integer, dtype=np.float32):
    """(x, w, b, g_y) of one table entry (N, K, C): the same arrays wherever the case is built."""
    n, k, c = shape
    rng = np.random.default_rng([n, k, c, int(bias), int(integer), np.dtype(dtype).itemsize])
    x = make_data(rng, (n, k), dtype, integer)
    w = make_data(rng, (c, k), dtype, integer)
    b = make_data(rng, (c,), dtype, integer) if bias else None
    g_y = make_data(rng, (n, c), dtype, integer)
    return x, w, b, g_y


# ---- mean pool over contiguous node ranges --------------------------------------------------------------------------
def mean_pool_ref(h, graph_ptr, g_pooled, integer=False):
    """h [N, W], graph_ptr [B + 1] (rows outside [graph_ptr[0], graph_ptr[B]) belong to no graph), g_pooled [B, W] ->
    {'pooled', 'g_h'}. pooled[g] = sum(h[p[g]:p[g+1]]) / max(cnt, 1); g_h[n] = g_pooled[g(n)] / max(cnt, 1), zero for a
    row outside every range."""
    wide = wide_dtype(h.dtype)
    ptr = np.asarray(graph_ptr, dtype=np.int64)
    n_graphs, width = len(ptr) - 1, h.shape[1]
    cnt = np.diff(ptr)
    div = np.maximum(cnt, 1)
    total = np.zeros((n_graphs, width), dtype=wide)
    S_sum = np.zeros((n_graphs, width), dtype=np.float64)
    hw = h.astype(wide)
    for g in range(n_graphs):
        total[g] = hw[ptr[g]:ptr[g + 1]].sum(axis=0)
        S_sum[g] = np.abs(h[ptr[g]:ptr[g + 1]]).astype(np.float64).sum(axis=0)
    n_of = np.broadcast_to(cnt[:, None], total.shape)
    d_of = np.broadcast_to(div[:, None], total.shape)
    fwd = Ref(total / div[:, None].astype(wide), n_of, S_sum / div[:, None], S_sum, total, d_of)
    gtot = np.zeros(h.shape, dtype=wide)
    gcnt = np.ones(h.shape, dtype=np.int64)
    for g in range(n_graphs):
        gtot[ptr[g]:ptr[g + 1]] = g_pooled[g].astype(wide)
        gcnt[ptr[g]:ptr[g + 1]] = div[g]
    S_b = np.abs(gtot).astype(np.float64)
    bwd = Ref(gtot / gcnt.astype(wide), 1, S_b / gcnt, S_b, gtot, gcnt)
    if integer:
        _assert_exact_domain(S_sum, h.dtype, f'mean_pool {h.shape}')
        _assert_exact_domain(S_b, h.dtype, f'mean_pool backward {h.shape}')
    return {'pooled': fwd, 'g_h': bwd}


# ---- unsorted segment sum / mean ------------------------------------------------------------------------------------
def segment_ref(data, ids, num_segments, mean, g_out, integer=False):
    """data [E, C], ids [E] in [0, num_segments), g_out [num_segments, C] -> {'out', 'g_data'}.
    out[s] = sum(data[ids == s]) (/ max(cnt, 1)); g_data[e] = g_out[ids[e]] (/ max(cnt, 1))."""
    wide = wide_dtype(data.dtype)
    ids = np.asarray(ids, dtype=np.int64)
    n_rows, width = data.shape
    cnt = np.bincount(ids, minlength=num_segments).astype(np.int64)
    div = np.maximum(cnt, 1) if mean else np.ones_like(cnt)
    total = np.zeros((num_segments, width), dtype=wide)
    S_sum = np.zeros((num_segments, width), dtype=np.float64)
    if n_rows:
        order = np.argsort(ids, kind='stable')
        filled = np.flatnonzero(cnt)
        starts = (np.cumsum(cnt) - cnt)[filled]        # empty segments hold no rows: consecutive starts delimit the rest
        total[filled] = np.add.reduceat(data[order].astype(wide), starts, axis=0)
        S_sum[filled] = np.add.reduceat(np.abs(data[order]).astype(np.float64), starts, axis=0)
    n_of = np.broadcast_to(cnt[:, None], total.shape)
    d_of = np.broadcast_to(div[:, None], total.shape)
    fwd = Ref(total / div[:, None].astype(wide), n_of, S_sum / div[:, None], S_sum, total, d_of)
    gtot = g_out[ids].astype(wide).reshape(n_rows, width)
    gcnt = np.broadcast_to(div[ids][:, None], gtot.shape)
    S_b = np.abs(gtot).astype(np.float64)
    bwd = Ref(gtot / gcnt.astype(wide), 1, S_b / gcnt, S_b, gtot, gcnt)
    if integer:
        _assert_exact_domain(S_sum, data.dtype, f'segment {data.shape}')
        _assert_exact_domain(S_b, data.dtype, f'segment backward {data.shape}')
    return {'out': fwd, 'g_data': bwd}


# ---- the comparisons ------------------------------------------------------------------------------------------------
def assert_exact(got, ref, what):
    """Bit for bit (np.array_equal: the sign of a zero aside). `ref.value` holds integers below the exactness limit."""
    want = np.asarray(ref.value).astype(got.dtype)
    assert got.shape == want.shape, f'{what}: shape {got.shape} != {want.shape}'
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f'{what}: {len(bad)} of {got.size} elements differ from the exact result; first at '
                             f'{bad[:8].tolist()}: got {got[tuple(bad[0])]!r}, want {want[tuple(bad[0])]!r}')


def assert_mean_exact(got, ref, what):
    """Integer data through a mean: bit for bit where the divisor is a power of two (or <= 1), elsewhere the exact sum
    divided once: |got - total/cnt| <= 3 u |total/cnt|."""
    u = unit(got.dtype)
    cnt = np.asarray(ref.cnt)
    assert got.shape == np.shape(ref.value), f'{what}: shape {got.shape} != {np.shape(ref.value)}'
    pow2 = (cnt & (cnt - 1)) == 0
    want = np.asarray(ref.value)
    same = got == want.astype(got.dtype)
    if not np.all(same[pow2]):
        bad = np.argwhere(pow2 & ~same)
        raise AssertionError(f'{what}: {len(bad)} elements with a power-of-two count differ from the exact mean; first '
                             f'at {bad[:8].tolist()}')
    err = np.abs(got.astype(want.dtype) - want)
    bound = 3.0 * u * np.abs(want)
    if not np.all(err <= bound):
        bad = np.argwhere(err > bound)
        i = tuple(bad[0])
        raise AssertionError(f'{what}: {len(bad)} elements off the exact mean by more than 3u; first at {bad[:8].tolist()}: '
                             f'err {float(err[i]):.3e} > {float(bound[i]):.3e}')


def assert_rounded(got, ref, what):
    """|got - ref| <= gamma(n + 3) S for every element."""
    u = unit(got.dtype)
    want = np.asarray(ref.value)
    assert got.shape == want.shape, f'{what}: shape {got.shape} != {want.shape}'
    assert np.all(np.isfinite(got)), f'{what}: non-finite output'
    err = np.abs(got.astype(want.dtype) - want).astype(np.float64)
    bound = gamma(np.asarray(ref.n) + 3, u) * ref.S
    if not np.all(err <= bound):
        bad = np.argwhere(err > bound)
        i = tuple(bad[0])
        raise AssertionError(f'{what}: {len(bad)} of {got.size} elements outside gamma(n+3) S; first at '
                             f'{bad[:8].tolist()}: err {float(err[i]):.3e} > {float(bound[i]):.3e}')


def assert_matches(got, ref, integer, what, mean=False):
    if not integer:
        assert_rounded(got, ref, what)
    elif mean:
        assert_mean_exact(got, ref, what)
    else:
        assert_exact(got, ref, what)


# ---- shape tables: (N, K_in, C_out), shared by the GPU sweep and the host checks -------------------------------------
# The route per shape (forward / g_x / g_w / g_b) is pinned by test_dispatch_routes for one shape per route.
LINEAR_F32 = [
    # MFMA linear <KB, CB>, all six instantiations (the g_x of (K, C) is the forward of (C, K)); square MFMA tsgemm
    (33, 32, 32), (129, 64, 32), (127, 128, 32), (128, 32, 64), (1, 64, 64), (31, 128, 64),
    # 64-output chunks, wide tsgemm
    (130, 64, 128), (65, 128, 128), (40, 128, 256), (40, 32, 128),
    # more than 256 outputs: 256-chunks (then 64-chunks), colreduce chunks
    (37, 64, 320), (37, 16, 300), (37, 300, 16),
    # generic k_linear, unaligned rows, degenerate widths, k_tsgemm_tn<32>, tsgemm column chunks (kc = 84, kc = 24)
    (257, 12, 32), (257, 13, 32), (64, 1, 1), (64, 7, 5), (64, 33, 100), (9, 96, 96), (9, 40, 300),
    # narrow-K MFMA weight gradient from N >= 1024, the bias gradient from its ones column
    (1023, 12, 32), (1024, 12, 32), (1025, 13, 64), (1500, 31, 32), (1100, 1, 64), (1100, 12, 64),
    # the head at the widest supported width: 160 KB of LDS forward, 16 (C + K) floats of LDS in k_tsgemm_tn
    (7, 1024, 2), (7, 1024, 1),
]
# row-count edges of the slab split (512-row blocks, rpb = ceil(N / blocks), 128-row colreduce blocks)
LINEAR_F32 += [(n, 32, 32) for n in (1, 511, 512, 513, 1025)] + [(n, 7, 5) for n in (1, 511, 512, 513, 1025)]
# grid-stride and block-cap paths (256-row blocks with two tiles per wave; the 1024- / 512-block caps)
LINEAR_F32_LARGE = [(32768 + 33, 32, 64), (262144 + 37, 32, 32)]
LINEAR_F32_ROUNDED = [(1, 64, 64), (65, 128, 128), (64, 33, 100), (1100, 12, 64)]
LINEAR_F32_REFUSED = [(4, 300, 200)]
LINEAR_F64 = [(1, 3, 2), (1024, 12, 32), (1025, 33, 20), (3000, 64, 64), (7, 1024, 2)]

POOL_WIDTHS = [1, 7, 32, 33, 1024, 1025]
POOL_GRAPHS = [[0, 0, 37, 0, 1, 500, 2, 0], [64], [1], [4, 8, 16, 2048]]
POOL_STRIDE_CASE = dict(width=200, sizes=[1000, 2000])           # 600000 elements: the backward's 2048 blocks loop
POOL_OUTSIDE_CASE = dict(graph_ptr=[5, 9, 20], rows=25)

SEGMENT_WIDTHS = [1, 3, 64, 65, 130]
# name -> (E, num_segments, how the ids are drawn)
SEGMENT_VARIANTS = {
    'sparse': (300, 1000, 'uniform'),             # many empty segments, unsorted ids with repeats
    'one_segment_of_many': (4096, 5, 'single'),   # one segment holds every row
    'single_segment': (77, 1, 'uniform'),
    'no_rows': (0, 4, 'uniform'),
    'pow2_counts': (0, 37, 'pow2'),               # every count a power of two (or 0): an exact mean (E follows)
}
SEGMENT_LOOPS = [(30000, 20000, 3), (30000, 700, 80)]            # (E, num_segments, C): wave loop; backward block cap


def pool_case(sizes, width, integer, dtype, lead=0, tail=0):
    """(h, graph_ptr, g_pooled): graphs of `sizes` rows behind `lead` rows (and before `tail` rows) of no graph."""
    ptr = lead + np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = int(ptr[-1]) + tail
    rng = np.random.default_rng([len(sizes), int(sum(sizes)), width, int(integer), np.dtype(dtype).itemsize, lead])
    h = make_data(rng, (rows, width), dtype, integer)
    g = make_data(rng, (len(sizes), width), dtype, integer)
    return h, ptr, g


def segment_ids(variant, rng):
    n_rows, n_seg, how = SEGMENT_VARIANTS[variant]
    if how == 'single':
        return np.full(n_rows, n_seg - 2, dtype=np.int64), n_seg
    if how == 'pow2':
        counts = 2 ** rng.integers(0, 6, size=n_seg)
        counts[rng.random(n_seg) < 0.3] = 0
        ids = np.repeat(np.arange(n_seg), counts)
        return rng.permutation(ids).astype(np.int64), n_seg
    return rng.integers(0, n_seg, size=n_rows).astype(np.int64), n_seg


def segment_case(variant, width, integer, dtype):
    """(data, ids, num_segments, g_out) of one variant at one width."""
    rng = np.random.default_rng([sorted(SEGMENT_VARIANTS).index(variant), width, int(integer), np.dtype(dtype).itemsize])
    ids, n_seg = segment_ids(variant, rng)
    data = make_data(rng, (len(ids), width), dtype, integer)
    g_out = make_data(rng, (n_seg, width), dtype, integer)
    return data, ids, n_seg, g_out


def segment_loop_case(shape, integer, dtype):
    n_rows, n_seg, width = shape
    rng = np.random.default_rng([n_rows, n_seg, width, int(integer), np.dtype(dtype).itemsize])
    ids = rng.integers(0, n_seg, size=n_rows).astype(np.int64)
    return make_data(rng, (n_rows, width), dtype, integer), ids, n_seg, make_data(rng, (n_seg, width), dtype, integer)
