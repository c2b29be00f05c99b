"""pvs_graph_prepare_runs as two streams over the int64 inputs (graph_prepare.hip: k_scan_rows, k_run_starts on the
caller's rows, k_place_stream): every case compares all nine output arrays - rowptr, row, col, etype, perm, colptr,
cedge, inv_deg, status - for exact equality with pvs_graph_prepare (the radix-sort route) on the same input.

The batches are built on the host in the loader's layout (per graph two row-sorted runs, `generate_edges`), with every
graph boundary and every descent at a chosen edge index. The kernels deal the edges out in a fixed grouping. k_scan_rows:
a workgroup takes GROUP = 2048 consecutive edges, each of its 4 waves 512 of them, and lane l of a wave owns the edges
l, 64 + l, ..., 448 + l of the wave's 512 (8 edges per thread, "slot" j = 0 ... 7). k_place_stream: the same with 4 edges
per thread (1024 per workgroup, 256 per wave, slots j = 0 ... 3), the one-hot words travel in pieces of 128 edges. The
only places where E enters the kernels are the per-edge test e < E and the per-word test w < E * A, so a remainder of E
shows as a last workgroup that is cut off inside a slot, a wave or a 128-edge piece: test_every_remainder walks ALL 2048
remainders of the larger workgroup (which contain every remainder of 1024, of a wave's 512 / 256, of a 128-edge piece
and of a thread's 8 / 4 edges).
"""
import numpy as np
import pytest
import torch

GROUP = 2048                 # edges per workgroup of k_scan_rows: 256 threads x 8 edges (k_place_stream: 1024)
NAMES = ('rowptr', 'row', 'col', 'etype', 'perm', 'colptr', 'cedge', 'inv_deg', 'status')

# (nodes, first edge, descent or None): the graph's edges are [first edge, next graph's first edge); the descent is the
# absolute index of the second run's first edge. Boundaries and descents sit on the first slot of a workgroup (2048:
# j = 0, lane 0 in both kernels), on an inner slot (2048 + 64 * 2 + 17: j = 2, lane 17 of 8 slots and of 4), on the
# last slot of a wave (2 * 2048 + 511: lane 63 of j = 7 / j = 3, the next graph starts with the next wave), on the first
# lane of a last slot (4096 + 448) and on the last lane of an inner slot (4608 + 64 * 4 + 63: j = 4 of 8, j = 0 of 4); the
# descents 13 and 6 are inner lanes of a first slot.
SPEC = (
    (1, 0, None),            # one node: three copies of its self-edge (no descent is possible)
    (2, 3, 6),               # rows 0 1 1 | 0 1
    (3, 8, None),            # no edges
    (5, 8, None),            # an empty second run
    (64, 12, 13),            # the descent at its first possible position: the first run is one edge
    (257, GROUP, GROUP + 64 * 2 + 16),       # ... and at its last: the second run is one edge; nodes without edges
    (64, GROUP + 64 * 2 + 17, 2 * GROUP + 448),      # few distinct pairs: duplicate edges
    (257, 2 * GROUP + 511 + 1, 2 * GROUP + 512 + 64 * 4 + 63),      # takes whatever E leaves
)
E_MIN = 2 * GROUP + 512 + 64 * 4 + 64 + 1      # the smallest E that keeps the last graph's descent
E_CAP = 5 * GROUP                              # the largest E (every batch is this one, cut after E edges)
NO_EDGES_257 = tuple(range(0, 2)) + tuple(range(100, 121)) + (255, 256)      # start, middle and end of the graph


def build_batch(n_edges, n_attr, seed=0):
    """-> dict(ei int64 [2, E], ea int64 one-hot [E, A] or None, node_ptr, edge_ptr (int lists), N). Deterministic, and
    the batch for E - 1 is the batch for E without its last edge."""
    assert E_MIN <= n_edges <= E_CAP
    rng = np.random.default_rng(seed)
    rows, cols, node_ptr, edge_ptr = [], [], [0], [0]
    for k, (n, first, descent) in enumerate(SPEC):
        assert first == edge_ptr[-1]
        end = SPEC[k + 1][1] if k + 1 < len(SPEC) else E_CAP
        m = end - first
        base = node_ptr[-1]
        allowed = np.setdiff1d(np.arange(n), NO_EDGES_257) if n == 257 else np.arange(n)
        d = m if descent is None else descent - first
        run_a = np.sort(rng.choice(allowed, size=d))
        run_b = np.sort(rng.choice(allowed, size=m - d))
        if descent is not None:
            run_a[-1], run_b[0] = allowed[-1], allowed[0]        # a descent for sure, and only this one
        r = np.concatenate([run_a, run_b])
        if n == 64 and first > GROUP:        # duplicates: every row has two possible columns
            c = (r + 1 + rng.integers(0, 2, size=m)) % n
        else:
            c = rng.integers(0, n, size=m)
        rows.append(r + base)
        cols.append(c + base)
        node_ptr.append(base + n)
        edge_ptr.append(first + m)
    rows, cols = np.concatenate(rows)[:n_edges], np.concatenate(cols)[:n_edges]
    edge_ptr[-1] = n_edges
    ei = torch.from_numpy(np.vstack([rows, cols]).astype(np.int64))
    ea = None
    if n_attr:
        et = np.random.default_rng(seed + 1).integers(0, n_attr, size=E_CAP)[:n_edges]      # (prefix-stable, as the edges)
        ea = torch.nn.functional.one_hot(torch.from_numpy(et), n_attr)
    return dict(ei=ei, ea=ea, node_ptr=node_ptr, edge_ptr=edge_ptr, N=node_ptr[-1])


def test_host_batches_have_the_loaders_layout():
    """The builder itself (no GPU): per graph two row-sorted runs that meet in exactly the promised descent, rows and
    columns inside the graph's node range, and the batch for a smaller E a prefix of the batch for a larger one."""
    b = build_batch(E_MIN + 700, 3)
    rows, cols = b['ei'][0].numpy(), b['ei'][1].numpy()
    assert b['edge_ptr'][-1] == rows.size == E_MIN + 700 and b['ea'].shape == (rows.size, 3)
    for k, (n, first, descent) in enumerate(SPEC):
        lo, hi = b['edge_ptr'][k], b['edge_ptr'][k + 1]
        assert lo == first and b['node_ptr'][k + 1] - b['node_ptr'][k] == n
        r = rows[lo:hi]
        assert np.all((r >= b['node_ptr'][k]) & (r < b['node_ptr'][k + 1]))
        assert np.all((cols[lo:hi] >= b['node_ptr'][k]) & (cols[lo:hi] < b['node_ptr'][k + 1]))
        drops = np.flatnonzero(np.diff(r) < 0) + 1 + lo
        assert drops.tolist() == ([] if descent is None else [descent])
    small = build_batch(E_MIN, 3)
    assert torch.equal(small['ei'], b['ei'][:, :E_MIN]) and torch.equal(small['ea'], b['ea'][:E_MIN])
    assert np.unique(np.stack([rows, cols])[:, b['edge_ptr'][6]:b['edge_ptr'][7]], axis=1).shape[1] <= 128     # duplicates
    assert not np.isin(rows[GROUP:b['edge_ptr'][6]] - b['node_ptr'][5], NO_EDGES_257).any()


def _tables(b, dev='cuda'):
    node_ptr = torch.tensor(b['node_ptr'], dtype=torch.int32, device=dev)
    edge_ptr = torch.tensor(b['edge_ptr'], dtype=torch.int32, device=dev)
    node_ptr.max_graph_nodes = max(n for n, _, _ in SPEC)
    return node_ptr, edge_ptr


def _offset_by_one_element(t):
    """The same values in storage that starts one int64 past a 16-byte boundary (contiguous, so no copy is made later)."""
    buf = torch.empty(t.numel() + 1, dtype=t.dtype, device=t.device)
    out = buf[1:].view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == 8
    return out


def _both_routes(ei, ea, n, layout):
    from pointvs_amd.graph import prepare_graph
    got = prepare_graph(ei, ea, n, need_backward=True, layout=layout)
    ref = prepare_graph(ei, ea, n, need_backward=True)
    return got, ref


def _assert_same(got, ref, with_etype, what=''):
    for name in NAMES:
        if name == 'etype' and not with_etype:
            assert 'etype' not in got.t and 'etype' not in ref.t
            continue
        assert torch.equal(got.t[name], ref.t[name]), (name, what)
    assert int(ref.t['status'].item()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize('offset', [False, True], ids=['aligned', 'offset_by_one_element'])
@pytest.mark.parametrize('n_edges', [3 * GROUP, 3 * GROUP + 1 - 2], ids=['even', 'odd'])
@pytest.mark.parametrize('n_attr', [0, 1, 3, 9])
def test_streams_equal_the_sort(n_attr, n_edges, offset):
    """All graph shapes of SPEC in one batch, 0 / 1 / 3 classes (and 9: more than the piece route takes, read word by word),
    E even and odd, and the same batch with edge_index / edge_attr one element off a 16-byte boundary."""
    b = build_batch(n_edges, n_attr)
    ei, ea = b['ei'].cuda(), None if b['ea'] is None else b['ea'].cuda()
    assert ei.data_ptr() % 16 == 0 and (ea is None or ea.data_ptr() % 16 == 0)
    if offset:
        ei, ea = _offset_by_one_element(ei), None if ea is None else _offset_by_one_element(ea)
    got, ref = _both_routes(ei, ea, b['N'], _tables(b))
    _assert_same(got, ref, n_attr > 0)
    got.check_status()


@pytest.mark.gpu
def test_every_remainder():
    """E = 2048 k + r for EVERY r of the larger workgroup's 2048 edges (hence every remainder of the other kernel's 1024, of
    a thread's 8 / 4 edges, a wave's 512 / 256 and a 128-edge piece of one-hot words), 3 classes: the batch for E is the largest batch cut after E edges. The nine
    comparisons of a size are folded into one device flag, read once at the end."""
    from pointvs_amd.graph import prepare_graph
    top = build_batch(E_MIN + 177 + GROUP, 3)
    e_top = top['edge_ptr'][-1]
    ei_top, ea_top = top['ei'].cuda(), top['ea'].cuda()
    node_ptr, edge_ptr = _tables(top)
    same = torch.ones(GROUP, dtype=torch.bool, device='cuda')
    for k in range(GROUP):
        e = e_top - k
        ei, ea = ei_top[:, :e].contiguous(), ea_top[:e]
        tables = (node_ptr, edge_ptr.clone())
        tables[1][-1] = e
        tables[0].max_graph_nodes = node_ptr.max_graph_nodes
        got = prepare_graph(ei, ea, top['N'], need_backward=True, layout=tables)
        ref = prepare_graph(ei, ea, top['N'], need_backward=True)
        for name in NAMES:
            same[k] &= (got.t[name] == ref.t[name]).all()
    bad = torch.nonzero(~same).flatten().cpu().numpy()
    assert bad.size == 0, ('E values that differ from the sort', (e_top - bad[:16]).tolist())
    assert sorted({(e_top - k) % GROUP for k in range(GROUP)}) == list(range(GROUP))


def _violate(b, kind):
    """One contract violation at a time, applied to the host batch. -> the status bits pvs_graph_prepare_runs reports
    for it (status bit 1: ids outside [0, N); 2: not one-hot; 4: not the promised layout)."""
    rows, cols = b['ei'][0], b['ei'][1]
    g5_lo, g5_hi = b['edge_ptr'][5], b['edge_ptr'][6]
    if kind == 'two_descents':
        mid = (g5_lo + g5_hi) // 2         # inside the first run of graph 5: a dip below the row in front of it
        rows[mid] = rows[mid - 1] - 1
        assert rows[mid + 1] >= rows[mid] and rows[mid] >= b['node_ptr'][5]
    elif kind == 'row_outside_graph':
        rows[g5_lo + 40] = b['node_ptr'][6] + 3          # a node of the next graph (inside [0, N))
    elif kind == 'col_outside_graph':
        cols[g5_lo + 40] = b['node_ptr'][4] + 3          # a node of the graph before
    elif kind == 'one_hot_two_ones':
        b['ea'][g5_lo + 40] = torch.tensor([1, 0, 1])
        return 2
    elif kind == 'one_hot_holds_a_2':
        b['ea'][g5_lo + 40] = torch.tensor([0, 2, 0])
        return 2
    elif kind == 'edge_ptr_short':
        b['edge_ptr'][-1] -= 5
    else:
        raise AssertionError(kind)
    return 4


@pytest.mark.gpu
@pytest.mark.parametrize('kind', ['two_descents', 'row_outside_graph', 'col_outside_graph', 'one_hot_two_ones',
                                  'one_hot_holds_a_2', 'edge_ptr_short'])
def test_contract_violations(kind):
    """The status bits are those of the two-pass extract / place kernels this replaces (reasoned from their code - every
    violation here sets exactly one bit - and run against that build: the same six values), every output index lies inside its array's range (host copies), and the
    Python layer raises as before."""
    from pointvs_amd.graph import prepare_graph
    b = build_batch(3 * GROUP, 3)
    bits = _violate(b, kind)
    e, n = 3 * GROUP, b['N']
    pg = prepare_graph(b['ei'].cuda(), b['ea'].cuda(), n, need_backward=True, layout=_tables(b))
    torch.cuda.synchronize()
    assert int(pg.t['status'].item()) == bits
    with pytest.raises(ValueError, match='one-hot' if bits == 2 else 'generate_edges'):
        pg.check_status()
    t = {name: pg.t[name].cpu().numpy() for name in NAMES}
    for name in ('rowptr', 'colptr'):
        assert t[name].shape == (n + 1,) and t[name][0] >= 0 and t[name][-1] <= e and np.all(np.diff(t[name]) >= 0), name
    for name in ('row', 'col'):
        assert t[name].min() >= 0 and t[name].max() < n, name
    assert t['perm'].min() >= 0 and t['perm'].max() < e and t['etype'].max() < 3
    used = t['cedge'][:t['colptr'][-1]]
    assert used.size == 0 or (used.min() >= 0 and used.max() < e)
    assert np.all(np.isfinite(t['inv_deg'])) and t['inv_deg'].min() > 0 and t['inv_deg'].max() <= 1
    if bits == 2 or kind == 'col_outside_graph':
        # rows alone decide the positions: the placement is still the sort's, a bijection onto [0, E)
        assert np.array_equal(np.sort(t['perm']), np.arange(e))
        assert np.array_equal(t['row'], np.sort(b['ei'][0].numpy(), kind='stable'))


@pytest.mark.gpu
def test_captured_and_replayed_twice():
    """The call captured in a hipGraph (training capture goes through this entry point) and replayed twice: the same
    arrays both times, with the outputs overwritten in between."""
    from pointvs_amd.graph import prepare_graph
    b = build_batch(3 * GROUP + 38, 3)
    ei, ea = b['ei'].cuda(), b['ea'].cuda()
    layout = _tables(b)
    ref = prepare_graph(ei, ea, b['N'], need_backward=True)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        prepare_graph(ei, ea, b['N'], need_backward=True, layout=layout)         # (first launches outside the capture)
        stream.synchronize()
        hip_graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(hip_graph, stream=stream):
            got = prepare_graph(ei, ea, b['N'], need_backward=True, layout=layout)
        for _ in range(2):
            for name in NAMES:
                got.t[name].fill_(-1 if got.t[name].dtype != torch.uint8 else 255)
            hip_graph.replay()
            stream.synchronize()
            _assert_same(got, ref, True, 'replay')
