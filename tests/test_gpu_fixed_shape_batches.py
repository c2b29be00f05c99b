"""GPU checks of the capacity batch builders (pvs_complex_batch_build_cap, pvs_radius_graph_build_cap): every output
array against the existing path - `build_batch`, then `prepare_graph` on its edge list, which
test_gpu_parquet_dataset.py pins to the reference loader's golden files - with no tolerance; padding rows; canaries
behind the edge count; exact-fit and one-short capacities; stale state; the status bits; repeatability."""
import numpy as np
import pytest

from tests._fixed_shape_cases import (DEV, LATTICE_NODE_COUNTS, OUTPUTS, assert_edge_canaries, assert_equals_eager,
                                      assert_padding, build_cap, canary_buffers, eager_reference, exact_capacities,
                                      generous_capacities, lattice_root, same_bytes, write_root)
from tests.test_gpu_parquet_dataset import setting

pytestmark = pytest.mark.gpu

GOLDEN_SETTINGS = ('cli_default', 'ref_test_smina', 'atomic_noh', 'noncompact')


def index_groups(n):
    """Singles, pairs, all, reversed."""
    return ([[i] for i in range(n)] + [list(range(k, min(k + 2, n))) for k in range(0, n, 2)] + [list(range(n))]
            + [list(range(n))[::-1]])


@pytest.mark.parametrize('name', GOLDEN_SETTINGS)
def test_golden_roots_equal_the_eager_batch(name):
    z, ds = setting(name)
    for indices in index_groups(len(z['order'])):
        cap = generous_capacities(ds, indices)
        assert_equals_eager(build_cap(ds, indices, cap), eager_reference(ds, indices), cap)


@pytest.fixture(scope='module')
def lattice(tmp_path_factory):
    return lattice_root(tmp_path_factory.mktemp('fixed_shape_lattice'))


def test_hand_made_roots_at_the_block_and_chunk_edges(lattice):
    """Kept node counts 1, 2, 63, 64, 65, 128, 129, 200 (the 64-row blocks and 64-column chunks of the mask kernels),
    each alone (a batch of one), all together, mixed with the hand cases (an empty crop, hydrogens dropped on one side,
    a receptor of 300 with two survivors), and out of order."""
    ds, at, n_lattice = lattice
    hand = list(range(n_lattice, len(ds)))
    for n in LATTICE_NODE_COUNTS:
        ref = eager_reference(ds, [at[n]])
        assert ref['n'] == n                                       # the case is what it says
    groups = [[at[n]] for n in LATTICE_NODE_COUNTS] + [[at[n] for n in LATTICE_NODE_COUNTS], hand,
                                                        [at[200], hand[0], at[1], hand[2], at[64], hand[3], at[65]],
                                                        [at[129], at[129], at[2], at[63], at[128]], [hand[2]]]
    for indices in groups:
        cap = generous_capacities(ds, indices)
        assert_equals_eager(build_cap(ds, indices, cap), eager_reference(ds, indices), cap)
    counts = eager_reference(ds, hand)['batch_obj'].graph_node_counts
    assert counts[0] == 3 and counts[2] == 5 and counts[3] == 2   # empty crop; 2 of 300; hydrogens dropped


def mixed(lattice):
    ds, at, n_lattice = lattice
    return ds, [at[65], n_lattice + 2, at[200], at[1], at[128], n_lattice + 3]


def test_exact_fit_capacities_raise_no_bit(lattice):
    _, golden = setting('cli_default')
    for ds, indices in (mixed(lattice), (golden, [0, 1, 2, 3, 4, 5]), (golden, [4])):
        cap = exact_capacities(ds, indices)
        ref = eager_reference(ds, indices)
        assert (cap.node_cap, cap.graph_node_cap, cap.edge_cap) == (ref['n'], ref['max_graph'], ref['e'])
        assert_equals_eager(build_cap(ds, indices, cap), ref, cap)


@pytest.mark.parametrize('short', ('node_cap', 'graph_node_cap', 'edge_cap'))
def test_one_short_of_a_capacity_sets_its_own_bit(lattice, short):
    from pointvs_amd import _lib
    bit = dict(node_cap=_lib.CAP_NODE_OVERFLOW, graph_node_cap=_lib.CAP_GRAPH_OVERFLOW,
               edge_cap=_lib.CAP_EDGE_OVERFLOW)[short]
    _, golden = setting('cli_default')
    for ds, indices in (mixed(lattice), (golden, [0, 1, 2, 3, 4, 5])):
        exact, ref = exact_capacities(ds, indices), eager_reference(ds, indices)
        cap = exact._replace(**{short: getattr(exact, short) - 1})
        out = build_cap(ds, indices, cap)
        assert int(out['status'][0]) == bit, (short, int(out['status'][0]))
        assert_edge_canaries(out, 0)                               # nothing written to row / col / etype
        assert int(out['n_edges_fwd'][0]) == 0                     # ... so a forward is handed no edge
        assert np.array_equal(out['node_ptr'], ref['ptr'].astype(np.int32))      # the true offsets either way
        if short == 'edge_cap':                                    # nodes fit: true counts, true E
            assert np.array_equal(out['rowptr'][:ref['n'] + 1], ref['rowptr'])
            assert int(out['rowptr'][cap.node_cap]) == ref['e']
            assert same_bytes(out['inv_deg'][:ref['n']], ref['inv_deg'])
            for key in ('x', 'pos', 'bp'):
                assert same_bytes(out[key][:ref['n']], ref[key]), key
        else:
            assert not out['rowptr'].any() and (out['inv_deg'] == 1.0).all()
        if short == 'node_cap':                                    # the sample that ends behind node_cap is left out whole
            kept = int(ref['ptr'][-2])
            for key in ('x', 'pos', 'bp'):
                assert same_bytes(out[key][:kept], ref[key][:kept]), key
            assert_padding(out, kept)


def test_a_small_batch_after_a_large_one_leaves_no_stale_rows(lattice):
    ds, at, n_lattice = lattice
    large, small = [at[200], at[129], at[128], at[65]], [at[2], n_lattice + 2, at[1], at[63]]
    cap = generous_capacities(ds, large)
    fresh = build_cap(ds, small, cap)
    buffers = canary_buffers(ds, len(large), cap)
    assert int(build_cap(ds, large, cap, buffers)['status'][0]) == 0
    reused = build_cap(ds, small, cap, buffers)
    e = eager_reference(ds, small)['e']
    for key in OUTPUTS:
        upto = e if key in ('row', 'col', 'etype') else None       # (behind E: the large batch's entries, never read)
        assert same_bytes(reused[key][:upto], fresh[key][:upto]), key
    assert_equals_eager(fresh, eager_reference(ds, small), cap)


def test_status_bits_of_an_empty_sample_and_of_a_class_outside_the_encoding(tmp_path):
    from pointvs_amd import _lib
    from pointvs_amd.captured_scoring import Capacities
    from pointvs_amd.parquet_data import PygPointCloudDataset
    lig = [(0.0, 0.0, 0.0, 6, 1)]
    only_h = [(0.0, 0.0, 0.0, 1, 11), (0.0, 0.0, 1.0, 1, 11)]
    root, types = write_root(tmp_path, [(lig, [(1.0, 0.0, 0.0, 34, 1)]), (only_h, [(30.0, 0.0, 0.0, 6, 1)])])
    cap = Capacities(64, 64, 1024, 16)
    noh = PygPointCloudDataset(root, radius=3, edge_radius=4, types_fname=types, use_atomic_numbers=True,
                               polar_hydrogens=False, compact=True)
    with pytest.raises(ValueError, match='no atom left'):          # the eager path raises for it
        noh.build_batch([0, 1], device=DEV)
    out = build_cap(noh, [0, 1], cap)
    assert int(out['status'][0]) == _lib.CAP_EMPTY_SAMPLE
    assert out['node_ptr'].tolist() == [0, 2, 2]                   # the other sample is built all the same
    assert int(out['rowptr'][cap.node_cap]) == 4                   # one contact: inter and intra, both directions
    noncompact = PygPointCloudDataset(root, radius=3, edge_radius=4, types_fname=types, use_atomic_numbers=True,
                                      polar_hydrogens=True, compact=False)
    assert int(build_cap(noncompact, [0], cap)['status'][0]) == 4  # the loader's 'outside the feature encoding' bit


def test_two_calls_give_identical_bytes(lattice):
    ds, indices = mixed(lattice)
    cap = generous_capacities(ds, indices)
    first, second = build_cap(ds, indices, cap), build_cap(ds, indices, cap)
    for key in OUTPUTS:
        assert same_bytes(first[key], second[key]), key
