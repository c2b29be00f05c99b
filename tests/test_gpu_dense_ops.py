"""Operator-level sweep of the dense and segment operators through their public surface (PF.linear, PF.mean_pool,
PF.segment_reduce, unsorted_segment_sum / unsorted_segment_mean), forward and backward, against the plain numpy
references of tests/_dense_ref.py.

Exact mode (integers in [-4, 4]): the kernel must return the reference bit for bit, whatever route the launcher picks -
one dropped, doubled or misplaced row or column shows. Rounded mode (standard-normal data): every element is within
gamma(n + 3) S of the reference, a bound taken from the reference alone. The shape tables (tests/_dense_ref.py) walk the
dispatch branches of pvs_launch_linear, pvs_launch_tsgemm_tn and pvs_launch_colreduce; test_dispatch_routes pins one
shape per branch to the branch it was chosen for."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import _dense_ref as R

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def run_linear(x, w, b, g_y, x_grad=True):
    from pointvs_amd import functional as PF
    tx, tw, tb = dev(x).requires_grad_(x_grad), dev(w).requires_grad_(True), dev(b)
    if tb is not None:
        tb.requires_grad_(True)
    y = PF.linear(tx, tw, tb)
    y.backward(dev(g_y))
    got = {'y': host(y), 'g_x': host(tx.grad), 'g_w': host(tw.grad)}
    if tb is not None:
        got['g_b'] = host(tb.grad)
    return got


def check_linear(shape, bias, integer, dtype=F32):
    x, w, b, g_y = R.linear_case(shape, bias, integer, dtype)
    ref = R.linear_ref(x, w, b, g_y, integer=integer)
    got = run_linear(x, w, b, g_y)
    assert set(got) == set(ref)
    for name in ref:
        assert got[name].dtype == dtype
        R.assert_matches(got[name], ref[name], integer, f'linear {shape} bias={bias} {name}')


# ---- PF.linear, fp32 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('shape', R.LINEAR_F32, ids=lambda s: 'x'.join(map(str, s)))
def test_linear_f32_exact(shape, bias):
    check_linear(shape, bias, integer=True)


@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('shape', R.LINEAR_F32_LARGE, ids=lambda s: 'x'.join(map(str, s)))
def test_linear_f32_exact_grid_stride(shape, bias):
    """Row counts past one pass of the grid: 256-row blocks with two tiles per wave, then the 1024-block cap of the
    linear and the 512-block cap of the reductions. S <= 16 N < 2**24 still holds (asserted by the reference)."""
    check_linear(shape, bias, integer=True)


@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('shape', R.LINEAR_F32_ROUNDED, ids=lambda s: 'x'.join(map(str, s)))
def test_linear_f32_rounded(shape, bias):
    check_linear(shape, bias, integer=False)


@pytest.mark.parametrize('shape', R.LINEAR_F32_REFUSED, ids=lambda s: 'x'.join(map(str, s)))
def test_linear_f32_refuses_what_does_not_fit(shape):
    """K_in x C_out weights beyond the 160 KB of LDS (and off the MFMA shapes) are refused on the host with the
    library's error, and the call after it is as right as ever."""
    from pointvs_amd import functional as PF
    x, w, b, g_y = R.linear_case(shape, True, integer=True)
    with pytest.raises(RuntimeError, match='do not fit LDS'):
        PF.linear(dev(x), dev(w), dev(b))
    torch.cuda.synchronize()
    check_linear((64, 33, 100), True, integer=True)


def test_linear_f32_one_dimensional_input():
    """A 1-D x is one row: y comes back 1-D, the gradients as for the [1, K] call."""
    from pointvs_amd import functional as PF
    x, w, b, g_y = R.linear_case((1, 40, 9), True, integer=True)
    ref = R.linear_ref(x, w, b, g_y, integer=True)
    tx, tw, tb = (dev(a).requires_grad_(True) for a in (x[0], w, b))
    y = PF.linear(tx, tw, tb)
    assert y.shape == (9,)
    y.backward(dev(g_y[0]))
    assert tx.grad.shape == (40,)
    R.assert_exact(host(y)[None], ref['y'], 'y')
    R.assert_exact(host(tx.grad)[None], ref['g_x'], 'g_x')
    R.assert_exact(host(tw.grad), ref['g_w'], 'g_w')
    R.assert_exact(host(tb.grad), ref['g_b'], 'g_b')


@pytest.mark.parametrize('shape', [(130, 64, 128), (64, 7, 5)], ids=lambda s: 'x'.join(map(str, s)))
def test_linear_f32_strided_views_equal_contiguous(shape):
    """Transposed views of x and weight give what their contiguous copies give, bit for bit (rounded data)."""
    from pointvs_amd import functional as PF
    x, w, b, g_y = R.linear_case(shape, True, integer=False)
    want = run_linear(x, w, b, g_y)
    xt, wt = dev(x.T), dev(w.T)                   # [K, N] and [K, C] in memory
    vx, vw, tb = xt.t().requires_grad_(True), wt.t().requires_grad_(True), dev(b).requires_grad_(True)
    assert not vx.is_contiguous() and not vw.is_contiguous()
    y = PF.linear(vx, vw, tb)
    y.backward(dev(g_y))
    for name, t in (('y', y), ('g_x', vx.grad), ('g_w', vw.grad), ('g_b', tb.grad)):
        assert np.array_equal(host(t), want[name]), name


def test_linear_f32_input_without_grad_skips_g_x():
    x, w, b, g_y = R.linear_case((129, 64, 32), True, integer=True)
    ref = R.linear_ref(x, w, b, g_y, integer=True)
    got = run_linear(x, w, b, g_y, x_grad=False)
    assert got['g_x'] is None
    for name in ('y', 'g_w', 'g_b'):
        R.assert_exact(got[name], ref[name], name)


def test_linear_f32_backward_is_reproducible_over_a_dirty_workspace():
    """The same backward twice, bit for bit, with a larger unrelated backward in between that reuses the allocator's
    cached workspace block and leaves other partial sums in it."""
    x, w, b, g_y = R.linear_case((1500, 31, 32), True, integer=False)
    first = run_linear(x, w, b, g_y)
    check_linear((4000, 64, 64), True, integer=False)
    second = run_linear(x, w, b, g_y)
    for name in first:
        assert np.array_equal(first[name], second[name]), name


# one shape per dispatch branch -> launches recorded per route (forward, g_x, g_w, g_b of one call with a bias)
ROUTES = {
    (33, 32, 32): {'linear_mfma': 2, 'tsgemm_mfma': 1, 'colreduce4': 1},
    (130, 64, 128): {'linear_chunk64': 1, 'linear_mfma': 3, 'tsgemm_wide': 1, 'colreduce4': 1},
    (37, 64, 320): {'linear_chunk256': 1, 'linear_chunk64': 1, 'linear_mfma': 5, 'linear_generic': 1, 'tsgemm_wide': 1,
                    'colreduce_chunk': 1, 'colreduce4': 2},
    (64, 7, 5): {'linear_generic': 2, 'tsgemm_tn8': 1, 'colreduce': 1},
    (64, 33, 100): {'linear_generic': 2, 'tsgemm_tn32': 1, 'colreduce4': 1},
    (9, 96, 96): {'linear_generic': 2, 'tsgemm_colchunk': 1, 'tsgemm_tn32': 1, 'tsgemm_tn8': 1, 'colreduce4': 1},
    (9, 40, 300): {'linear_chunk256': 1, 'linear_generic': 3, 'tsgemm_colchunk': 1, 'tsgemm_tn32': 2,
                   'colreduce_chunk': 1, 'colreduce4': 2},
    (1023, 12, 32): {'linear_generic': 2, 'tsgemm_tn8': 1, 'colreduce4': 1},
    (1024, 12, 32): {'linear_generic': 2, 'tsgemm_narrow': 1},
    (7, 1024, 2): {'linear_chunk256': 1, 'linear_generic': 5, 'tsgemm_tn8': 1, 'colreduce': 1},
}
ROUTE_NAMES = ('linear_mfma', 'linear_chunk64', 'linear_chunk256', 'linear_generic', 'tsgemm_mfma', 'tsgemm_wide',
               'tsgemm_colchunk', 'tsgemm_narrow', 'tsgemm_tn8', 'tsgemm_tn32', 'colreduce4', 'colreduce',
               'colreduce_chunk')
ROUTE_FIRST_ID = 6          # PVS_PROF_DENSE_FIRST: the route groups follow the six kernel groups, in ROUTE_NAMES order
# the node-level launchers of a layer (csrc/profile.h), after the dense routes; tests/test_gpu_node_side.py reads them
NODE_ROUTE_NAMES = ('node_mlp_fwd', 'node_mlp_bwd', 'node_out_fwd', 'node_out_bwd', 'node_tail', 'node_wgrads')


@pytest.mark.parametrize('shape', list(ROUTES), ids=lambda s: 'x'.join(map(str, s)))
def test_dispatch_routes(shape):
    """The branch of pvs_launch_linear / pvs_launch_tsgemm_tn / pvs_launch_colreduce each representative shape takes,
    read from the library's measurement hook (one group per branch; a chunking branch is recorded once and its inner
    launches under their own branch). A change of a dispatch threshold that moves a shape off the branch it was put in
    the tables for fails here. The hook names the branch, not the template instantiation inside it: <KB, CB> of the MFMA
    kernels follows from (K / 32, C / 32) of the shape alone."""
    from pointvs_amd import _lib
    lib = _lib.lib()
    x, w, b, g_y = R.linear_case(shape, True, integer=True)
    mask = sum(1 << (ROUTE_FIRST_ID + k + 1) for k in range(len(ROUTE_NAMES)))
    lib.pvs_profile_reset()
    lib.pvs_profile_enable(mask)
    try:
        run_linear(x, w, b, g_y)
        torch.cuda.synchronize()
    finally:
        lib.pvs_profile_enable(0)
    seen = {}
    for name in ROUTE_NAMES:
        ms, cnt = C.c_double(0.0), C.c_int64(0)
        assert lib.pvs_profile_read(name.encode(), C.byref(ms), C.byref(cnt)) == 0
        if cnt.value:
            seen[name] = cnt.value
    lib.pvs_profile_reset()
    assert seen == ROUTES[shape]


def test_route_groups_stay_out_of_the_every_group_switch():
    """pvs_profile_enable(1) (what the benchmark's profile legs pass) records the kernel groups only: neither the dense
    routes of a linear nor the dense and node-level routes of a layer's forward and backward - hidden 32 without a gate
    (the folded chain, the fused weight gradients) and hidden 16 with GraphNorm, node attention and a gated residual
    (the separate stages, tsgemm, the column reductions) -, while the layer's edge kernels are recorded."""
    from pointvs_amd import _lib
    from pointvs_amd.egnn_satorras import EGNNLayer
    lib = _lib.lib()
    x, w, b, g_y = R.linear_case((33, 32, 32), True, integer=True)
    gen = torch.Generator().manual_seed(3)
    n = 70
    ei = torch.randint(0, n, (2, 400), generator=gen)
    ei = ei[:, ei[0] != ei[1]].cuda()
    lib.pvs_profile_reset()
    lib.pvs_profile_enable(1)
    try:
        run_linear(x, w, b, g_y)
        for hid, flags in ((32, dict()), (16, dict(graphnorm=True, node_attention=True, gated_residual=True))):
            layer = EGNNLayer(hid, hid, hid, **flags).cuda()
            h = torch.randn(n, hid, generator=gen).cuda().requires_grad_(True)
            pos = torch.randn(n, 3, generator=gen).cuda()
            h_out, x_out, _, m = layer(h, ei, pos)
            (h_out.sum() + x_out.sum() + m.sum()).backward()
        torch.cuda.synchronize()
    finally:
        lib.pvs_profile_enable(0)
    for name in ROUTE_NAMES + NODE_ROUTE_NAMES:
        ms, cnt = C.c_double(0.0), C.c_int64(-1)
        assert lib.pvs_profile_read(name.encode(), C.byref(ms), C.byref(cnt)) == 0 and cnt.value == 0, name
    for name in ('edge_fwd', 'edge_bwd'):
        ms, cnt = C.c_double(0.0), C.c_int64(-1)
        assert lib.pvs_profile_read(name.encode(), C.byref(ms), C.byref(cnt)) == 0 and cnt.value == 2, name
    lib.pvs_profile_reset()


def test_two_operand_generic_linear_in_a_hidden_16_layer_exact():
    """node_mlp.0 of a layer is ONE product over two (input, weight) pairs, y1 = h W1[:, :H]^T + Magg W1[:, H:]^T + b1.
    At hidden size 16 the MFMA linear refuses the shape and the generic kernel takes both pairs (at 32 / 64 the fused
    node MLP does, at 128 two accumulating passes). Through pvs_egnn_layer_fwd with every value an integer: edge_mlp.2
    = 0 * z + b2e with b2e >= 32, where SiLU(v) = v * rcp(1 + exp(-v)) is v itself, so Magg = deg (x) b2e; h, W1 >= 0
    and b1 = 32 keep y1 >= 32, so u = y1; W2, b2 in [-4, 4]. h_out = (y1) W2^T + b2 is then exact in fp32 in any order
    (|sums| < 2**24, asserted): one dropped, doubled or swapped row, column or operand shows. 70 rows: one full pass
    of the kernel's rows plus a ragged remainder; some rows without edges."""
    from pointvs_amd import _lib
    from pointvs_amd.functional import _stream, _ws
    from pointvs_amd.graph import prepare_graph
    lib = _lib.lib()
    rng = np.random.default_rng(16)
    n, H = 70, 16
    ei = rng.integers(0, n - 6, size=(2, 230))                      # rows n-6 .. n-1 have no edges
    ei = ei[:, ei[0] != ei[1]]
    deg = np.bincount(ei[0], minlength=n).astype(F64)
    h = rng.integers(0, 5, size=(n, H)).astype(F32)
    p = dict(edge_w1=rng.standard_normal((H, 2 * H + 1)).astype(F32), edge_b1=rng.standard_normal(H).astype(F32),
             edge_w2=np.zeros((H, H), F32), edge_b2=rng.integers(32, 41, size=H).astype(F32),
             node_w1=rng.integers(0, 5, size=(H, 2 * H)).astype(F32), node_b1=np.full(H, 32, F32),
             node_w2=rng.integers(-4, 5, size=(H, H)).astype(F32), node_b2=rng.integers(-4, 5, size=H).astype(F32))
    magg = deg[:, None] * p['edge_b2'].astype(F64)[None, :]
    y1 = h.astype(F64) @ p['node_w1'][:, :H].astype(F64).T + magg @ p['node_w1'][:, H:].astype(F64).T + p['node_b1']
    want = y1 @ p['node_w2'].astype(F64).T + p['node_b2']
    assert y1.min() >= 32 and np.abs(y1).max() * 4 * H < 2 ** 24 and np.abs(want).max() < 2 ** 24
    pg = prepare_graph(torch.from_numpy(ei).cuda(), None, n, need_backward=False)
    tp = {k: dev(v) for k, v in p.items()}
    pstruct = _lib.PvsLayerParams(*[_lib.ptr(tp.get(name)) for name in _lib.PARAM_FIELDS])
    desc = _lib.PvsLayerDesc(H, 0, 0, _lib.ACT_CODES['sigmoid'])
    th, tx = dev(h), dev(rng.standard_normal((n, 3)).astype(F32) * 3)
    h_out, x_out = torch.empty_like(th), torch.empty_like(tx)
    saved = torch.empty(lib.pvs_egnn_layer_saved_floats(C.byref(desc), n, pg.n_edges), dtype=torch.float32, device='cuda')
    ws_bytes = lib.pvs_egnn_layer_workspace_bytes(C.byref(desc), n, pg.n_edges, 0)
    ws = _ws(ws_bytes, th.device)
    lib.pvs_profile_reset()
    lib.pvs_profile_enable(sum(1 << (ROUTE_FIRST_ID + k + 1) for k in range(len(ROUTE_NAMES))))
    try:
        rc = lib.pvs_egnn_layer_fwd(C.byref(desc), C.byref(pg.c), C.byref(pstruct), _lib.ptr(th), _lib.ptr(tx), None,
                                    _lib.ptr(h_out), _lib.ptr(x_out), None, None, None, _lib.ptr(saved), _lib.ptr(ws),
                                    ws_bytes, _stream(th.device))
        _lib.check(rc, 'pvs_egnn_layer_fwd')
        torch.cuda.synchronize()
    finally:
        lib.pvs_profile_enable(0)
    routes = {}
    for name in ROUTE_NAMES:
        ms, cnt = C.c_double(0.0), C.c_int64(0)
        assert lib.pvs_profile_read(name.encode(), C.byref(ms), C.byref(cnt)) == 0
        if cnt.value:
            routes[name] = cnt.value
    lib.pvs_profile_reset()
    assert routes == {'linear_generic': 4}, routes          # P, Q, node_mlp.0 (two operands), node_mlp.3
    R.assert_exact(host(h_out), R.Ref(want, 2 * H, None), 'h_out of the hidden-16 layer')
    assert np.array_equal(host(x_out), host(tx))


# ---- PF.linear, fp64 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('integer', [True, False], ids=['exact', 'rounded'])
@pytest.mark.parametrize('bias', [True, False], ids=['bias', 'nobias'])
@pytest.mark.parametrize('shape', R.LINEAR_F64, ids=lambda s: 'x'.join(map(str, s)))
def test_linear_f64(shape, bias, integer):
    check_linear(shape, bias, integer, dtype=F64)


def test_linear_f64_one_dimensional_input():
    from pointvs_amd import functional as PF
    x, w, b, g_y = R.linear_case((1, 33, 20), True, integer=True, dtype=F64)
    ref = R.linear_ref(x, w, b, g_y, integer=True)
    tx, tw, tb = (dev(a).requires_grad_(True) for a in (x[0], w, b))
    y = PF.linear(tx, tw, tb)
    assert y.shape == (20,) and y.dtype == torch.float64
    y.backward(dev(g_y[0]))
    R.assert_exact(host(y)[None], ref['y'], 'y')
    R.assert_exact(host(tx.grad)[None], ref['g_x'], 'g_x')
    R.assert_exact(host(tw.grad), ref['g_w'], 'g_w')
    R.assert_exact(host(tb.grad), ref['g_b'], 'g_b')


# ---- PF.mean_pool ---------------------------------------------------------------------------------------------------
def run_mean_pool(h, ptr, g):
    from pointvs_amd import functional as PF
    th = dev(h).requires_grad_(True)
    pooled = PF.mean_pool(th, torch.from_numpy(np.asarray(ptr, dtype=np.int32)).cuda())
    pooled.backward(dev(g))
    return {'pooled': host(pooled), 'g_h': host(th.grad)}


def check_mean_pool(h, ptr, g, integer, what):
    ref = R.mean_pool_ref(h, ptr, g, integer=integer)
    got = run_mean_pool(h, ptr, g)
    for name in ('pooled', 'g_h'):
        assert got[name].dtype == h.dtype
        R.assert_matches(got[name], ref[name], integer, f'mean_pool {what} {name}', mean=True)
    return got, ref


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('width', R.POOL_WIDTHS)
@pytest.mark.parametrize('sizes', R.POOL_GRAPHS, ids=lambda s: 'g' + '_'.join(map(str, s)))
def test_mean_pool(sizes, width, dtype):
    """Empty graphs in front, in a row and at the end; one graph; one row; power-of-two sizes (bit-exact means)."""
    for integer in (True, False):
        h, ptr, g = R.pool_case(sizes, width, integer, dtype)
        got, ref = check_mean_pool(h, ptr, g, integer, f'{sizes} x {width} integer={integer}')
        if integer and all((s & (s - 1)) == 0 for s in sizes):
            R.assert_exact(got['pooled'], ref['pooled'], 'pooled (power-of-two graphs)')
            R.assert_exact(got['g_h'], ref['g_h'], 'g_h (power-of-two graphs)')


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_mean_pool_backward_grid_stride(dtype):
    """3000 rows of 200 channels: more elements than the fp32 backward's 2048 blocks of 256 threads hold at once."""
    case = R.POOL_STRIDE_CASE
    for integer in (True, False):
        h, ptr, g = R.pool_case(case['sizes'], case['width'], integer, dtype)
        assert h.size > 2048 * 256
        check_mean_pool(h, ptr, g, integer, f'stride integer={integer}')


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_mean_pool_rows_outside_every_graph(dtype):
    """graph_ptr = [5, 9, 20] over 25 rows: rows 0-4 and 20-24 feed no mean, so their gradient is ZERO - what autograd of
    the reference pooling gives, in both dtypes."""
    case = R.POOL_OUTSIDE_CASE
    ptr = np.asarray(case['graph_ptr'])
    sizes = np.diff(ptr).tolist()
    for width in (7, 32):
        for integer in (True, False):
            h, p, g = R.pool_case(sizes, width, integer, dtype, lead=int(ptr[0]), tail=case['rows'] - int(ptr[-1]))
            assert h.shape[0] == case['rows'] and p.tolist() == ptr.tolist()
            got, _ = check_mean_pool(h, p, g, integer, f'outside rows x {width} integer={integer}')
            assert not got['g_h'][:ptr[0]].any() and not got['g_h'][ptr[-1]:].any()
            assert got['g_h'][ptr[0]:ptr[-1]].any()


# ---- segment_reduce -------------------------------------------------------------------------------------------------
def run_segment(data, ids, n_seg, mean, g_out, via_module=False):
    from pointvs_amd import functional as PF
    from pointvs_amd.egnn_satorras import unsorted_segment_mean, unsorted_segment_sum
    td = data if torch.is_tensor(data) else dev(data)
    td = td.requires_grad_(True)
    tid = ids if torch.is_tensor(ids) else dev(ids)
    if via_module:
        out = (unsorted_segment_mean if mean else unsorted_segment_sum)(td, tid, n_seg)
    else:
        out = PF.segment_reduce(td, tid, n_seg, mean=mean)
    out.backward(dev(g_out))
    return {'out': host(out), 'g_data': host(td.grad)}


def check_segment(data, ids, n_seg, g_out, integer, what, **kw):
    for mean in (False, True):
        ref = R.segment_ref(data, ids, n_seg, mean, g_out, integer=integer)
        got = run_segment(data, ids, n_seg, mean, g_out, **kw)
        for name in ('out', 'g_data'):
            assert got[name].dtype == data.dtype
            R.assert_matches(got[name], ref[name], integer, f'segment {what} mean={mean} {name}', mean=True)


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('width', R.SEGMENT_WIDTHS)
@pytest.mark.parametrize('variant', list(R.SEGMENT_VARIANTS))
def test_segment_reduce(variant, width, dtype):
    """Unsorted ids with repeats: many empty segments, one segment with every row, one segment in all, no rows at all
    (zeros out, an empty gradient back), and counts that are all powers of two (a bit-exact mean). Sums of integer data
    are always bit-exact; the general means are within 3u of the exact mean."""
    for integer in (True, False):
        data, ids, n_seg, g_out = R.segment_case(variant, width, integer, dtype)
        check_segment(data, ids, n_seg, g_out, integer, f'{variant} x {width} integer={integer}',
                      via_module=(width == 3))
        if variant == 'no_rows':
            got = run_segment(data, ids, n_seg, True, g_out)
            assert got['out'].shape == (n_seg, width) and not got['out'].any() and got['g_data'].shape == (0, width)
        if variant == 'pow2_counts' and integer:
            ref = R.segment_ref(data, ids, n_seg, True, g_out, integer=True)
            got = run_segment(data, ids, n_seg, True, g_out)
            R.assert_exact(got['out'], ref['out'], 'mean over power-of-two counts')
            R.assert_exact(got['g_data'], ref['g_data'], 'mean backward over power-of-two counts')


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
def test_segment_reduce_int32_ids_and_strided_data(dtype):
    data, ids, n_seg, g_out = R.segment_case('sparse', 65, True, dtype)
    ids32 = torch.from_numpy(ids.astype(np.int32)).cuda()
    view = dev(data.T).t()                       # [E, C] over [C, E] memory
    assert not view.is_contiguous()
    for mean in (False, True):
        ref = R.segment_ref(data, ids, n_seg, mean, g_out, integer=True)
        for what, got in (('int32 ids', run_segment(data, ids32, n_seg, mean, g_out)),
                          ('strided data', run_segment(view.detach(), ids, n_seg, mean, g_out))):
            R.assert_mean_exact(got['out'], ref['out'], f'{what} mean={mean} out')
            R.assert_mean_exact(got['g_data'], ref['g_data'], f'{what} mean={mean} g_data')


@pytest.mark.parametrize('dtype', [F32, F64], ids=['f32', 'f64'])
@pytest.mark.parametrize('shape', R.SEGMENT_LOOPS, ids=lambda s: 'x'.join(map(str, s)))
def test_segment_reduce_loops(shape, dtype):
    """20000 segments: the fp32 forward's waves loop over segments behind its 4096-block cap; 30000 x 80 elements: the
    fp32 backward's grid-stride loop behind its 8192-block cap."""
    for integer in (True, False):
        data, ids, n_seg, g_out = R.segment_loop_case(shape, integer, dtype)
        check_segment(data, ids, n_seg, g_out, integer, f'{shape} integer={integer}')
