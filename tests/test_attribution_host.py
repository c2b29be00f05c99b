"""Attribution, host side (no GPU): the reference's import path and signatures, the yardstick the GPU tests use (a numpy
restatement of the masked-graph construction through the oracle's fp64 forward against the fixtures made from the real
reference), and the host logic of pointvs_amd.attribution (chunking, the masks bond_masking visits, edge counts,
argument validation, score reduction)."""
import inspect

import numpy as np
import pytest
import torch

from tests._attribution_ref import ATTR_CASES, AttrCase, masked_coo, oracle_outputs

REFERENCE_SIGNATURES = {
    'atom_masking': ['model', 'p', 'v', 'm', 'bs', 'edge_indices', 'edge_attrs', 'resis', 'kwargs'],
    'bond_masking': ['model', 'p', 'v', 'm', 'bs', 'edge_indices', 'edge_attrs', 'kwargs'],
    'cam': ['model', 'p', 'v', 'm', 'edge_indices', 'edge_attrs', 'kwargs'],
    'node_attention': ['model', 'p', 'v', 'edge_indices', 'edge_attrs', 'gnn_layer', 'kwargs'],
    'edge_attention': ['model', 'p', 'v', 'edge_indices', 'edge_attrs', 'gnn_layer', 'kwargs'],
}


def test_reference_import_path_and_signatures():
    from point_vs.attribution import attribution_fns
    assert attribution_fns.SIGMOID is False
    for name, params in REFERENCE_SIGNATURES.items():
        fn = getattr(attribution_fns, name)
        assert list(inspect.signature(fn).parameters) == params, name
    sig = inspect.signature(attribution_fns.atom_masking).parameters
    assert sig['bs'].default == 32 and sig['m'].default is None


def test_fixture_set_is_complete():
    assert len(ATTR_CASES) == 7
    fns = {AttrCase(n).fn for n in ATTR_CASES}
    assert fns == {'atom_masking', 'bond_masking'}
    assert any(AttrCase(n).sigmoid for n in ATTR_CASES)
    z = AttrCase('attr_testkwargs_g1').z
    assert {'extra/cam', 'extra/node_attention', 'extra/edge_attention'} <= set(z.files)


@pytest.mark.parametrize('name', ATTR_CASES)
def test_masked_graph_restatement_reproduces_reference_outputs(name):
    """The yardstick: numpy masking + the oracle's fp64 forward gives the reference's own masked outputs, within the
    distance the reference's fp32 run keeps from its fp64 run (noise32; a hair of 1e-9 relative for the fp64 runs'
    own summation order)."""
    c = AttrCase(name)
    if c.n > 200:       # (every 8th mask of the large graph: the oracle is one graph per forward)
        pick = np.arange(0, len(c.visited), 8)
    else:
        pick = np.arange(len(c.visited))
    got = oracle_outputs(c, drop=c.drop_table()[pick])
    rows = np.concatenate([[0], 1 + pick])
    assert got.shape == c.raw64[rows].shape
    scale = float(np.abs(c.raw64).max())
    assert np.abs(got - c.raw64[rows]).max() <= 1e-9 * scale
    assert np.abs(got - c.raw32[rows]).max() <= c.noise32 + 1e-9 * scale
    assert c.noise32 > 0 and c.bound() < 1e-5


@pytest.mark.parametrize('name', ATTR_CASES)
def test_fixture_scores_follow_from_raw_outputs(name):
    from pointvs_amd import attribution as T
    c = AttrCase(name)
    raw = c.z['raw32']
    if c.fn == 'atom_masking':
        orig, masked = torch.from_numpy(raw[0]), torch.from_numpy(raw[1:])
        if c.sigmoid:
            orig, masked = torch.sigmoid(orig), torch.sigmoid(masked)
        got = T._atom_scores(orig.numpy(), masked.numpy(), c.sigmoid)
        assert np.abs(got - c.scores).max() <= 1e-7
    else:
        got = np.zeros(c.edge_index.shape[1])
        got[c.visited] = T._bond_scores(raw[0], raw[1:])
        assert np.abs(got - c.scores).max() <= 1e-7
        assert np.all(c.scores[c.edge_type.numpy() != 1] == 0)


def test_chunk_size():
    from pointvs_amd.attribution import MAX_CHUNK_EDGES, chunk_size
    assert chunk_size(32, 5, 100, 1000) == 5                 # bs larger than the mask count
    assert chunk_size(1, 500, 100, 1000) == 1
    assert chunk_size(32, 500, 100, 1000) == 32
    assert chunk_size(32, 2000, 2000, 320_000) == MAX_CHUNK_EDGES // 320_000 == 31      # the edge cap
    assert chunk_size(32, 2000, 2000, 2 * MAX_CHUNK_EDGES) == 1                          # never below one graph
    assert chunk_size(10 ** 6, 10 ** 6, 3000, 1, max_edges=2 ** 40) == (2 ** 31 - 2) // 3000     # int32 node ids
    assert chunk_size(10 ** 6, 10 ** 6, 1, 3000, max_edges=2 ** 40) == (2 ** 31 - 1) // 3000     # int32 edge ids
    assert chunk_size(32, 0, 10, 10) == 1
    with pytest.raises(ValueError):
        chunk_size(0, 5, 10, 10)


def test_bond_mask_table_and_edge_counts():
    from pointvs_amd.attribution import bond_mask_table, masked_edge_counts
    c = AttrCase('attr_dimout3_ball120')
    ei, ea = c.edge_index.numpy(), c.edge_attr.numpy()
    visited, drop = bond_mask_table(ei, ea)
    assert np.array_equal(visited, np.nonzero(c.edge_type.numpy() == 1)[0])
    assert np.array_equal(visited, c.visited)
    assert np.array_equal(drop, c.drop_table())
    assert np.all(drop[:, 0] < drop[:, 1])
    atoms = np.stack([np.arange(c.n), np.full(c.n, -1)], axis=1)
    for table in (drop, atoms, np.array([[3, 3], [5, 2]])):
        want = [masked_coo(ei, None, d)[0].shape[1] for d in table]
        assert np.array_equal(masked_edge_counts(ei, table, c.n), want)
    # duplicate edges, a self loop, an isolated atom
    ei = np.array([[0, 1, 1, 2, 0, 2, 2, 1, 0], [1, 0, 2, 1, 2, 0, 2, 2, 1]])
    table = np.array([[0, -1], [1, -1], [2, -1], [3, -1], [0, 1], [1, 2], [0, 2], [2, 3], [2, 2]])
    want = [masked_coo(ei, None, d)[0].shape[1] for d in table]
    assert np.array_equal(masked_edge_counts(ei, table, 4), want)
    visited, drop = bond_mask_table(np.array([[1, 2], [1, 0]]), np.array([[0, 1, 0], [0, 1, 0]]))
    assert drop.tolist() == [[1, -1], [0, 2]]


def test_score_reduction_branches():
    from pointvs_amd import attribution as T
    masked = np.array([[1.0, 2.0, 6.0], [0.0, 0.0, 0.0]], dtype=np.float32)
    got = T._atom_scores(np.array([[3.0, 3.0, 6.0]], dtype=np.float32), masked, False)      # [1, 3]: the mean of three
    assert np.allclose(got, [1.0, 4.0])
    with pytest.raises(TypeError):                   # a 1-D three-vector: the reference's float() raises
        T._atom_scores(np.array([3.0, 3.0, 6.0], dtype=np.float32), masked, False)
    assert np.allclose(T._atom_scores(np.array([0.5], dtype=np.float32), masked[:, :1], False), [-0.5, 0.5])
    assert np.allclose(T._bond_scores(np.array([3.0, 4.0, 6.0]), masked), [2.0, 4.0])       # output 1 of several
    assert np.allclose(T._bond_scores(np.array([3.0]), masked[:, :1]), [2.0, 3.0])          # the single output


def test_argument_validation_without_a_device():
    from pointvs_amd import attribution as T
    p, v = torch.zeros(1, 4, 3), torch.zeros(1, 4, 12)
    with pytest.raises(TypeError):
        T.atom_masking(torch.nn.Linear(1, 1), p, v, edge_indices=torch.zeros(2, 3, dtype=torch.long))
    with pytest.raises(ValueError):
        T.bond_masking(None, p, v, edge_indices=torch.zeros(2, 3, dtype=torch.long))
    with pytest.raises(ValueError):
        T.bond_masking(None, p, v, edge_indices=torch.zeros(2, 3, dtype=torch.long),
                       edge_attrs=torch.zeros(4, 3, dtype=torch.long))
    with pytest.raises(ValueError):
        T.build_mask_batch(None, np.zeros((0, 2)))
    for code, exc in ((1, IndexError), (4, RuntimeError), (8, RuntimeError), (16, RuntimeError)):
        with pytest.raises(exc):
            T.raise_for_status(code)
    T.raise_for_status(0)


def test_switch_follows_the_alias_module():
    from point_vs.attribution import attribution_fns
    from pointvs_amd import attribution as T
    try:
        attribution_fns.SIGMOID = True
        with pytest.raises(ValueError):
            attribution_fns.bond_masking(None, None, None)
        assert T.SIGMOID is True
    finally:
        attribution_fns.SIGMOID = False
        T.SIGMOID = False
