"""Masking attribution on the GPU: the leave-out batch builder (pvs_mask_graph_build) against prepare_graph of
host-masked edge lists, and atom_masking / bond_masking / cam / node_attention / edge_attention against the fixtures made
from the real reference (tests/golden/attr_*.npz) and the oracle's fp64 run.

Bound per case (README "Parity"): max|raw - ref64| <= 1e-5 * max|ref64| + 4 * noise32, ref64 = the oracle's fp64 output
of every masked graph, noise32 from the fixture. The returned scores (a difference of two such outputs) are held to
twice that, and their top-k sets (k <= 5) must equal the reference's wherever the reference's own gap between ranks k
and k + 1 exceeds twice the bound; the top-1 of every case qualifies (the maker asserts it).
"""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
import torch

from tests._attribution_ref import (ATTR_CASES, AttrCase, kept_nodes, masked_coo, oracle_outputs, ranked_scores)
from tests._golden import GoldenCase

pytestmark = pytest.mark.gpu
REL64 = 1e-9          # tests/test_gpu_fp64.py: 1e-9 * max|ref| (+ 1e-14 * G for gradients; none here)


def _model(c, dtype=torch.float32):
    from pointvs_amd.egnn_multitask import MultitaskSatorrasEGNN
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    cls = SartorrasEGNN if c.meta['class'] == 'SartorrasEGNN' else MultitaskSatorrasEGNN
    model = cls(Path('/tmp/pvs_test'), 2e-3, 1e-4, None, None, silent=True, **c.meta['kwargs'])
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in c.sd.items()})
    model = model.to('cuda').eval()
    return model.double() if dtype == torch.float64 else model


def _args(c):
    return dict(edge_indices=c.edge_index.cuda(), edge_attrs=c.edge_attr.cuda())


def _raw(c, model, bs=32, drop=None):
    from pointvs_amd import attribution as T
    drop = c.drop_table() if drop is None else drop
    orig, masked = T.masked_outputs(model, c.pos[None], c.x[None], drop, bs, **_args(c))
    return np.concatenate([orig.reshape(1, -1).double().cpu().numpy(), masked.double().cpu().numpy()])


_ORACLE = {}


def _ref64(c):
    if c.name not in _ORACLE:
        _ORACLE[c.name] = oracle_outputs(c)
    return _ORACLE[c.name]


# ---------------------------------------------------------------- the builder

def _check_builder(edge_index, edge_type, n, table):
    """One builder call for the whole table against prepare_graph of every host-masked COO list: arrays equal exactly."""
    from pointvs_amd.attribution import build_mask_batch
    from pointvs_amd.graph import prepare_graph
    ei = torch.as_tensor(edge_index, dtype=torch.long).cuda()
    ea = None if edge_type is None else torch.nn.functional.one_hot(torch.as_tensor(edge_type).long(), 3).cuda()
    parent = prepare_graph(ei, ea, n, need_backward=False)
    parent.check_status()
    mb = build_mask_batch(parent, table)
    mb.check_status()
    t = mb.prepared.t
    gp, ep = mb.graph_ptr.cpu().numpy(), mb.graph_eptr.cpu().numpy()
    rowptr, src = t['rowptr'].cpu().numpy(), mb.src_node.cpu().numpy()
    total_e = int(rowptr[-1])
    assert ep[-1] == total_e and gp[-1] == mb.prepared.n_nodes and gp[0] == 0 and ep[0] == 0
    row, col = t['row'][:total_e].cpu().numpy(), t['col'][:total_e].cpu().numpy()
    etype = None if edge_type is None else t['etype'][:total_e].cpu().numpy()
    inv_deg = t['inv_deg'].cpu().numpy()
    for b, d in enumerate(np.asarray(table).reshape(-1, 2)):
        mei, met, _ = masked_coo(edge_index, edge_type, d)
        keep = kept_nodes(n, d)
        n0, n1, e0, e1 = gp[b], gp[b + 1], ep[b], ep[b + 1]
        assert n1 - n0 == len(keep) and e1 - e0 == mei.shape[1], (b, d)
        assert np.array_equal(src[n0:n1], keep), (b, d)
        if mei.shape[1] == 0:         # nothing left to prepare: every row empty
            assert np.all(rowptr[n0:n1 + 1] == e0) and np.all(inv_deg[n0:n1] == 1.0)
            continue
        mea = None if met is None else torch.nn.functional.one_hot(torch.from_numpy(met).long(), 3).cuda()
        want = prepare_graph(torch.from_numpy(mei).cuda(), mea, len(keep), need_backward=False)
        want.check_status()
        w = want.t
        assert np.array_equal(rowptr[n0:n1 + 1] - e0, w['rowptr'].cpu().numpy()), (b, d)
        assert np.array_equal(col[e0:e1] - n0, w['col'].cpu().numpy()), (b, d)
        assert np.array_equal(row[e0:e1] - n0, w['row'].cpu().numpy()), (b, d)
        assert np.array_equal(inv_deg[n0:n1], w['inv_deg'].cpu().numpy()), (b, d)
        if etype is not None:
            assert np.array_equal(etype[e0:e1], w['etype'].cpu().numpy()), (b, d)


def _graphs():
    out = {}
    for name in ('attr_clidefault_ball120', 'attr_clidefault_ball400', 'attr_clidefault_g1'):
        c = AttrCase(name)
        out[name] = (c.edge_index.numpy(), c.edge_type.numpy(), c.n)
    g = GoldenCase('c0_clidefault_g4dup')             # duplicate inter edges
    out['c0_clidefault_g4dup'] = (g.edge_index.numpy(), g.edge_type.numpy(), int(g.x.shape[0]))
    return out


@pytest.mark.parametrize('name', ['attr_clidefault_ball120', 'attr_clidefault_ball400', 'attr_clidefault_g1',
                                  'c0_clidefault_g4dup'])
def test_builder_equals_prepare_graph_of_masked_lists(name):
    from pointvs_amd.attribution import bond_mask_table
    ei, et, n = _graphs()[name]
    _check_builder(ei, et, n, np.stack([np.arange(n), np.full(n, -1)], axis=1))          # every atom
    _, pairs = bond_mask_table(ei, np.eye(3, dtype=np.int64)[et])
    assert len(pairs) > 0
    _check_builder(ei, et, n, pairs)                                                      # every type-1 pair


def test_builder_degenerate_inputs():
    # node 4 has no edges; node 3 hangs on node 2 alone (masking 2 leaves it with degree 0); (0, 1) is listed twice
    ei = np.array([[0, 1, 0, 1, 1, 2, 2, 3, 0, 2], [1, 0, 1, 0, 2, 1, 3, 2, 2, 0]])
    et = np.array([1, 1, 0, 0, 2, 2, 2, 2, 0, 0])
    table = np.array([[4, -1], [2, -1], [0, 1], [1, 1], [3, 2], [0, -1], [2, 4]])
    _check_builder(ei, et, 5, table)
    _check_builder(ei, None, 5, table)                                   # no edge classes
    _check_builder(ei, et, 5, table[1:2])                                # B = 1
    two = np.array([[0, 1], [1, 0]])
    _check_builder(two, np.array([1, 1]), 2, np.array([[0, -1]]))        # N = 2, B = 1
    _check_builder(two, np.array([1, 1]), 2, np.array([[1, -1], [0, -1]]))
    ei64 = np.array([[i, (i + 1) % 70] for i in range(70)] * 2).T        # rows shorter than a 16-lane group, N > 64
    _check_builder(ei64, np.zeros(140, dtype=np.int64), 70, np.array([[0, 69], [5, -1]]))
    dense = np.array([[i, j] for i in range(80) for j in range(80) if i != j]).T         # 79 edges per row: wave per row
    _check_builder(dense, (dense[0] % 3), 80, np.array([[0, 79], [40, -1], [3, 4]]))


def test_builder_out_of_range_id_raises_through_status():
    from pointvs_amd.attribution import build_mask_batch
    from pointvs_amd.graph import prepare_graph
    ei = torch.tensor([[0, 1, 1, 2], [1, 0, 2, 1]]).cuda()
    parent = prepare_graph(ei, None, 3, need_backward=False)
    for table in ([[3, -1]], [[0, -1], [-2, -1]], [[1, 7]], [[0, -3]]):
        mb = build_mask_batch(parent, np.array(table))
        with pytest.raises(IndexError):
            mb.check_status()
    build_mask_batch(parent, np.array([[2, -1]])).check_status()


def test_builder_is_bitwise_reproducible():
    from pointvs_amd.attribution import build_mask_batch
    from pointvs_amd.graph import prepare_graph
    c = AttrCase('attr_clidefault_ball400')
    parent = prepare_graph(c.edge_index.cuda(), c.edge_attr.cuda(), c.n, need_backward=False)
    runs = []
    for _ in range(2):
        mb = build_mask_batch(parent, c.drop_table())
        mb.check_status()
        e = int(mb.graph_eptr[-1])
        runs.append([mb.prepared.t[k][:e if k in ('row', 'col', 'etype') else None].cpu().numpy()
                     for k in ('rowptr', 'row', 'col', 'etype', 'inv_deg')] + [mb.src_node.cpu().numpy()])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- outputs and scores

@pytest.mark.parametrize('name', ATTR_CASES)
def test_masked_outputs_and_scores_match_reference(name):
    from point_vs.attribution import attribution_fns
    c = AttrCase(name)
    model = _model(c)
    ref64 = _ref64(c)
    bound = c.bound(ref64)
    got = _raw(c, model)
    assert got.shape == ref64.shape
    err = float(np.abs(got - ref64).max())
    print(f'{name}: raw err {err:.3e} bound {bound:.3e} (noise32 {c.noise32:.2e})')
    assert err <= bound, f'{name}: |raw - ref64| = {err:.3e} > {bound:.3e}'
    fn = getattr(attribution_fns, c.fn)
    try:
        attribution_fns.SIGMOID = c.sigmoid
        scores = fn(model, c.pos[None].cuda(), c.x[None].cuda(), **_args(c))
    finally:
        attribution_fns.SIGMOID = False
    assert isinstance(scores, np.ndarray) and scores.shape == c.scores.shape
    # the fp64 scores: the reference's arithmetic on the oracle's outputs
    sig = (lambda a: 1.0 / (1.0 + np.exp(-a))) if c.sigmoid else (lambda a: a)
    pick = 0 if ref64.shape[1] == 1 else 1
    want = np.zeros_like(c.scores)
    want[c.visited if c.fn == 'bond_masking' else slice(None)] = sig(ref64[0, pick]) - sig(ref64[1:, pick])
    s_err = float(np.abs(scores - want).max())
    print(f'{name}: score err {s_err:.3e} bound {2 * bound:.3e}')
    assert s_err <= 2 * bound
    assert float(np.abs(scores - c.scores).max()) <= 2 * bound + 2 * c.noise32      # and the reference's own fp32 scores
    if c.fn == 'bond_masking':
        assert np.all(scores[c.edge_type.numpy() != 1] == 0)
    ref_rank, got_rank = ranked_scores(c, c.scores), ranked_scores(c, scores)
    order_ref, order_got = np.argsort(-ref_rank, kind='stable'), np.argsort(-got_rank, kind='stable')
    compared = 0
    for k in range(1, 6):
        if ref_rank[order_ref[k - 1]] - ref_rank[order_ref[k]] > 2 * bound:
            assert set(order_ref[:k]) == set(order_got[:k]), f'{name}: top-{k} differs'
            compared += 1
            if k == 1:
                assert order_ref[0] == order_got[0]
    print(f'{name}: {compared} of 5 rank cuts compared')
    assert ref_rank[order_ref[0]] - ref_rank[order_ref[1]] > 2 * bound, 'top-1 must qualify'


def test_cam_and_attention_match_reference():
    from point_vs.attribution import attribution_fns as A
    c = AttrCase('attr_testkwargs_g1')
    model = _model(c)
    for name in ('cam', 'node_attention', 'edge_attention'):
        got = np.asarray(getattr(A, name)(model, c.pos[None].cuda(), c.x[None].cuda(), **_args(c)))
        want = c.z[f'extra/{name}']
        assert got.shape == want.shape, name
        assert np.abs(got - want).max() <= 1e-5 * max(1.0, np.abs(want).max()), name


@pytest.mark.parametrize('name', ['attr_clidefault_ball120', 'attr_testkwargs_g1', 'attr_dimout3_ball120'])
def test_chunk_size_does_not_change_the_result(name):
    c = AttrCase(name)
    model = _model(c)
    ref64 = _ref64(c)
    bound = c.bound(ref64)
    runs = {bs: _raw(c, model, bs) for bs in (1, 7, 32)}
    for bs, got in runs.items():
        assert np.abs(got - ref64).max() <= bound, bs
    assert np.abs(runs[1] - runs[32]).max() <= bound and np.abs(runs[7] - runs[32]).max() <= bound
    for bs in (7, 32):
        assert np.array_equal(_raw(c, model, bs), runs[bs]), f'bs={bs} is not bitwise reproducible'


@pytest.mark.parametrize('name', ['attr_clidefault_ball120', 'attr_testkwargs_g1', 'attr_multitask_reg_ball120'])
def test_fp64_model_meets_the_fp64_bound(name):
    c = AttrCase(name)
    model = _model(c, torch.float64)
    ref64 = _ref64(c)
    got = _raw(c, model, 16)
    err, bound = float(np.abs(got - ref64).max()), REL64 * float(np.abs(ref64).max())
    print(f'{name}: fp64 err {err:.3e} bound {bound:.3e}')
    assert err <= bound
    assert float(np.abs(_raw(c, _model(c), 16) - ref64).max()) > bound       # (fp32 cannot meet it: the bound bites)


@pytest.mark.parametrize('name', ['attr_clidefault_g1', 'attr_testkwargs_g1', 'attr_dimout3_ball120'])
def test_batched_equals_loop_over_single_graph_forward(name):
    """The user-visible contract: what a loop of model(graph) over host-masked graphs returns."""
    from pointvs_amd.graph import Data
    c = AttrCase(name)
    model = _model(c)
    bound = c.bound(_ref64(c))
    got = _raw(c, model)
    ei0, et0 = c.edge_index.numpy(), c.edge_type.numpy()
    with torch.no_grad():
        for b, d in enumerate(c.drop_table()):
            mei, met, _ = masked_coo(ei0, et0, d)
            keep = torch.from_numpy(kept_nodes(c.n, d))
            g = Data(x=c.x[keep], pos=c.pos[keep], edge_index=torch.from_numpy(mei),
                     edge_attr=torch.nn.functional.one_hot(torch.from_numpy(met).long(), 3),
                     batch=torch.zeros(len(keep), dtype=torch.long), num_graphs=1).to('cuda')
            one = model(g).reshape(-1).double().cpu().numpy()
            assert np.abs(one - got[1 + b]).max() <= bound, (b, d)


def test_single_output_bond_masking_and_dropout_model():
    """bond_masking of a one-output model returns the scalar score's change (the reference raises there); a model built
    with dropout is scored in eval mode and left in the mode it came in."""
    from pointvs_amd import attribution as T
    c = AttrCase('attr_clidefault_g1')
    model = _model(c)
    visited, drop = T.bond_mask_table(c.edge_index.numpy(), c.edge_attr.numpy())
    ref = oracle_outputs(c, drop=drop)
    bound = c.bound(ref)
    scores = T.bond_masking(model, c.pos[None], c.x[None], bs=13, **_args(c))
    want = np.zeros(c.edge_index.shape[1])
    want[visited] = ref[0, 0] - ref[1:, 0]
    assert np.abs(scores - want).max() <= 2 * bound
    model.dropout_p = 0.5
    model.train()
    again = T.bond_masking(model, c.pos[None], c.x[None], bs=13, **_args(c))
    assert model.training and np.array_equal(again, scores)


def test_graphnorm_model_is_scored_one_copy_per_forward():
    from pointvs_amd.attribution import couples_graphs
    assert couples_graphs(_model(AttrCase('attr_testkwargs_g1')))
    assert not couples_graphs(_model(AttrCase('attr_clidefault_g1')))


def test_launches_grow_with_chunks_not_with_masks():
    from pointvs_amd import _lib
    c = AttrCase('attr_clidefault_ball120')
    model = _model(c)
    lib = _lib.lib()
    table = c.drop_table()
    bs = 16

    def launches(n_masks):
        lib.pvs_profile_enable(1)
        lib.pvs_profile_reset()
        try:
            _raw(c, model, bs, table[:n_masks])
            out = {}
            for key in (b'mask_graph', b'edge_fwd', b'graph_prepare'):
                ms, n = C.c_double(), C.c_int64()
                assert lib.pvs_profile_read(key, C.byref(ms), C.byref(n)) == 0
                out[key] = n.value
        finally:
            lib.pvs_profile_enable(0)
            lib.pvs_profile_reset()
        return out

    launches(bs)                                   # warm-up
    small, large = launches(2 * bs), launches(7 * bs - 3)
    assert small[b'mask_graph'] == 2 and large[b'mask_graph'] == 7             # ceil(masks / bs), not masks
    assert small[b'graph_prepare'] == large[b'graph_prepare'] == 1            # the parent, once
    assert small[b'edge_fwd'] > 0 and small[b'edge_fwd'] % 3 == 0 and large[b'edge_fwd'] % 8 == 0
    assert small[b'edge_fwd'] // 3 == large[b'edge_fwd'] // 8                  # per forward: chunks + the unmasked graph
