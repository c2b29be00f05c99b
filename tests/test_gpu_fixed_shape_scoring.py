"""GPU checks of data-root scoring through the fixed-shape step (pointvs_amd/captured_scoring.py): the eager fixed-shape
step against `model(batch)` on `build_batch`'s batch, one captured step replayed on other batch compositions,
`val(capture=True)` end to end with and without forced fallbacks, the refusals and the command line."""
import ctypes as C
import json
from pathlib import Path

import pytest
import torch

from tests._fixed_shape_cases import DEV, eager_reference, exact_capacities, generous_capacities, lattice_root
from tests._golden import needs_caching_allocator
from tests.test_gpu_parquet_dataset import DATAROOT, load_cli, setting

pytestmark = pytest.mark.gpu

FLAG_SETS = {
    'default': dict(k=32),                                                                   # build_net's: GraphNorm on
    'attention': dict(k=32, edge_attention=True, node_attention=True, tanh=True, residual=True, graphnorm=False,
                      normalize=False),
    'k64_graphnorm': dict(k=64, normalize=True, graphnorm=True),
}
BOUND = 1e-5          # max|delta| <= BOUND * max|ref|: what the screening paths are held to (test_gpu_library_screen.py)


def make_model(feature_dim, seed=0, **kwargs):
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    torch.manual_seed(seed)
    kwargs = {'k': 32, 'num_layers': 3, 'dim_output': 1, 'model_task': 'classification', **kwargs}
    return SartorrasEGNN(Path('/tmp/pvs_fixed_shape'), 2e-3, 1e-4, silent=True, dim_input=feature_dim,
                         **kwargs).cuda().eval()


@pytest.fixture(scope='module')
def lattice(tmp_path_factory):
    return lattice_root(tmp_path_factory.mktemp('fixed_shape_scoring'))


def cases(lattice):
    _, golden = setting('cli_default')
    ds, at, n_lattice = lattice
    return (('cli_default', golden, [0, 1, 2, 3, 4, 5]),
            ('hand-made', ds, [at[65], n_lattice + 2, at[200], at[1], at[128], n_lattice + 3]))


@pytest.mark.parametrize('flags', sorted(FLAG_SETS))
def test_eager_fixed_shape_step_equals_the_model_forward(lattice, flags):
    from pointvs_amd.captured_scoring import FixedShapeScorer
    for name, ds, indices in cases(lattice):
        model = make_model(ds.feature_dim, **FLAG_SETS[flags])
        with torch.no_grad():
            ref = model(eager_reference(ds, indices)['batch_obj']).reshape(-1)
        scorer = FixedShapeScorer(model, ds, len(indices), generous_capacities(ds, indices), device=DEV)
        got = scorer(indices).reshape(-1)
        scorer.check()
        delta, scale = (got - ref).abs().max().item(), ref.abs().max().item()
        print(f'{flags} / {name}: max|delta| = {delta:.3g}, max|ref| = {scale:.3g}, ratio {delta / scale:.3g}')
        assert torch.isfinite(got).all() and delta <= BOUND * scale, (flags, name, delta, scale)


def scores_at(model, ds, indices, cap):
    from pointvs_amd.captured_scoring import FixedShapeScorer
    scorer = FixedShapeScorer(model, ds, len(indices), cap, device=DEV)
    out = scorer(indices).clone()
    scorer.check()
    return out


def test_graphnorm_statistics_ignore_the_padding_rows(lattice):
    """A GraphNorm model with generous node padding and with exact-fit node capacities, at one edge capacity: the same
    bits. The statistics, the dense layers, pooling and head never see a padding row."""
    for name, ds, indices in cases(lattice):
        model = make_model(ds.feature_dim, **FLAG_SETS['default'])
        exact, generous = exact_capacities(ds, indices), generous_capacities(ds, indices)
        for edge_cap in (exact.edge_cap, generous.edge_cap):
            padded = scores_at(model, ds, indices, generous._replace(edge_cap=edge_cap))
            tight = scores_at(model, ds, indices, exact._replace(edge_cap=edge_cap))
            assert torch.equal(padded, tight), (name, edge_cap, (padded - tight).abs().max().item())


def test_generous_and_exact_fit_capacities_give_the_same_bits(lattice):
    """A GraphNorm model with generous padding and with exact-fit capacities (every capacity, the edge room too): the
    same bits. The statistics ignore the padding rows, and the MFMA edge forward plans its chunks from the device-side
    edge count (pvs_edge_replan, csrc/edge_dispatch.h), not from the room of the edge arrays - planned from the room,
    the chunk ends, and with them the order of a row's fp32 partial sums, moved with edge_cap (7.45e-08 at a largest
    score of 0.255 on the six cli_default complexes)."""
    for name, ds, indices in cases(lattice):
        model = make_model(ds.feature_dim, **FLAG_SETS['default'])
        padded = scores_at(model, ds, indices, generous_capacities(ds, indices))
        tight = scores_at(model, ds, indices, exact_capacities(ds, indices))
        print(f'{name}: max|delta| = {(padded - tight).abs().max().item():.3g}, max|score| = {tight.abs().max().item():.3g}')
        assert torch.equal(padded, tight), (name, (padded - tight).abs().max().item())


@needs_caching_allocator
@pytest.mark.parametrize('flags', ('default', 'attention'))
def test_one_captured_step_serves_other_batch_compositions(flags):
    """Permutations, and subsets that fill the batch with repeats: every replay equals the eager fixed-shape step on
    the same load, bit for bit. The eager step is a second scorer's, of the same capacities: a scorer is eager or
    captured, never both."""
    from pointvs_amd.captured_scoring import FixedShapeScorer
    _, ds = setting('cli_default')
    model = make_model(ds.feature_dim, **FLAG_SETS[flags])
    every = [0, 1, 2, 3, 4, 5]
    cap = generous_capacities(ds, every)
    scorer = FixedShapeScorer(model, ds, 6, cap, device=DEV).capture([5, 4, 3, 2, 1, 0])
    twin = FixedShapeScorer(model, ds, 6, cap, device=DEV)
    for indices in (every, [3, 0, 5, 1, 4, 2], [1, 1, 1, 2, 2, 2], [0, 3, 0, 3, 0, 3], [1, 2, 1, 2, 1, 1]):
        replayed = scorer.replay(indices).clone()
        eager = twin(indices).clone()
        scorer.check()
        twin.check()
        assert torch.equal(replayed, eager), (indices, (replayed - eager).abs().max().item())
    repeats = scorer.replay([1, 1, 1, 2, 2, 2]).clone()           # the load reaches the step: equal samples score alike
    scorer.check()                                                 # (up to fp32 summation order: they sit at other rows)
    assert torch.allclose(repeats[0], repeats[1], rtol=1e-4) and torch.allclose(repeats[3], repeats[5], rtol=1e-4)
    assert not torch.allclose(repeats[0], repeats[3], rtol=1e-3)
    with pytest.raises(RuntimeError, match='replay'):             # a captured scorer runs no eager step,
        scorer(every)
    with pytest.raises(RuntimeError, match='fresh scorer'):       # is not captured twice,
        scorer.capture(every)
    with pytest.raises(RuntimeError, match='fresh scorer'):       # and a scorer that has run eager steps is not captured
        twin.capture(every)


@pytest.mark.parametrize('flags', ('attention', 'k128'))
def test_an_edge_overflow_after_a_good_batch_stays_inside_the_edge_room(flags):
    """edge_cap fits the first batch and not the second, every other capacity fits both: the second build keeps the true
    counts in rowptr beside the first batch's row / col / etype, sets the edge bit alone and hands the forward no edge
    (n_edges_fwd = 0). A layer run on that graph with edge attention writes nothing behind the edge room of its
    attention output (a guard of canaries as long as the overflow and more); the whole step runs, reports the bit, and
    the good batch afterwards scores what it scored before, bit for bit. k128: the width with a per-edge message
    scratch."""
    from pointvs_amd import _lib
    from pointvs_amd import functional as PF
    from pointvs_amd.captured_scoring import FixedShapeScorer, batch_input_atoms
    _, ds = setting('cli_default')
    kwargs =FLAG_SETS['attention'] if flags == 'attention' else dict(FLAG_SETS['attention'], k=128)
    model = make_model(ds.feature_dim, **kwargs)
    good, big = [1, 0], [4, 5]
    e_good, e_big = eager_reference(ds, good)['e'], eager_reference(ds, big)['e']
    assert e_good < e_big
    cap = generous_capacities(ds, big)._replace(edge_cap=e_good, atoms_in_cap=batch_input_atoms(ds, [good, big]))
    scorer = FixedShapeScorer(model, ds, 2, cap, device=DEV)
    first = scorer(good).clone()
    scorer.check()
    scorer.load(big)
    scorer.build()
    t = scorer.t
    assert int(t['status'].item()) == _lib.CAP_EDGE_OVERFLOW
    assert int(t['rowptr'][cap.node_cap].item()) == e_big and int(t['n_edges_fwd'].item()) == 0
    # one layer through the C ABI, its attention output a view of a guarded buffer
    layer, kind = scorer.egnn[0], PF._K32
    params, pstruct = layer._params_cached()
    desc = _lib.PvsLayerDesc(*layer._desc())
    n, e = cap.node_cap, cap.edge_cap
    h = scorer.embed.embed(t['x'], t['pos']).contiguous()
    guarded = torch.full((e_big + 4096,), -77.0, device=DEV)
    h_out, x_out = torch.empty_like(h), torch.empty_like(t['pos'])
    node_att = torch.empty(n, device=DEV)
    saved = torch.empty(kind.layer_saved(C.byref(desc), n, e), device=DEV)
    ws_bytes = kind.layer_ws(C.byref(desc), n, e, 0)
    ws = torch.full((ws_bytes + (e_big + 4096) * 4 * layer.hidden_nf,), 0x4D, dtype=torch.uint8, device=DEV)
    kind.check(kind.layer_fwd(C.byref(desc), C.byref(scorer.pg.c), C.byref(pstruct), _lib.ptr(h), _lib.ptr(t['pos']), None,
                              _lib.ptr(h_out), _lib.ptr(x_out), None, _lib.ptr(guarded), _lib.ptr(node_att),
                              _lib.ptr(saved), _lib.ptr(ws), ws_bytes, _lib.stream(torch.device(DEV))), 'layer_fwd')
    torch.cuda.synchronize()
    assert (guarded[e:] == -77.0).all() and (ws[ws_bytes:] == 0x4D).all()
    scorer()                                                       # the whole step on the overflowing batch
    assert scorer.take_status() == _lib.CAP_EDGE_OVERFLOW
    again = scorer(good).clone()
    scorer.check()
    assert torch.equal(again, first)


def val_loader():
    from pointvs_amd.parquet_data import get_data_loader
    z, _ = setting('cli_default')
    meta = json.loads(str(z['settings']))
    return get_data_loader(DATAROOT, types_fname=DATAROOT / meta['types'], mode='val', batch_size=2, rot=False,
                           device=DEV, **meta['kwargs'])


def rows(path):
    return [ln.split() for ln in Path(path).read_text().splitlines()]


def val_both_ways(tmp_path, **capture_options):
    """(model, rows of val()'s file, rows of val(capture=True)'s file) on chembl6.types, batch 2, one probe batch."""
    loader = val_loader()
    model = make_model(loader.dataset.feature_dim)
    model.val(loader, predictions_file=tmp_path / 'eager.txt')
    model.val(loader, predictions_file=tmp_path / 'captured.txt', capture=True,
              capture_options=dict(probe_batches=1, **capture_options))
    return model, rows(tmp_path / 'pose_eager.txt'), rows(tmp_path / 'pose_captured.txt')


def assert_same_predictions(eager, captured):
    """The same lines in the same order: labels and names identical, every score within one unit of the last printed
    digit."""
    wanted = [ln.split() for ln in (DATAROOT / 'chembl6.types').read_text().splitlines()]
    assert len(eager) == len(captured) == len(wanted) == 6
    for a, b, w in zip(eager, captured, wanted):
        assert (a[0], a[1], a[3], a[4]) == (b[0], b[1], b[3], b[4]) and (b[3], b[4]) == (w[3], w[4])
        assert abs(float(a[2]) - float(b[2])) <= 0.001 + 1e-9, (a, b)


@needs_caching_allocator
def test_val_with_capture_writes_the_same_file(tmp_path):
    _, eager, captured = val_both_ways(tmp_path)
    assert_same_predictions(eager, captured)


@needs_caching_allocator
def test_val_with_capture_replays_two_batches_without_fallback(tmp_path):
    """chembl6.types, batch 2, probe_batches=1, the default headroom: two replays and no fallback. The last batch
    (complexes 4, 5: the file's two largest, 11,962 edges) is larger than 1.5 x the probe batch's 7,106 edges; it fits
    because the plan counts a batch as no less than batch_size copies of the largest complex seen (2 x 3,832 edges x
    1.5 = 11,496, rounded up to 12,288)."""
    model, _, _ = val_both_ways(tmp_path)
    print(model.last_val_stats)
    assert model.last_val_stats['fallback'] == 0 and model.last_val_stats['replayed'] == 2
    assert model.last_val_stats == dict(eager=1, replayed=2, fallback=0)


@needs_caching_allocator
def test_val_falls_back_where_the_capacities_are_too_small(tmp_path):
    """Capacities that fit only the smallest complex: both replayed batches overflow, are rebuilt by the eager route and
    land in file order; the file is the eager file."""
    from pointvs_amd.captured_scoring import Capacities, batch_input_atoms
    loader = val_loader()
    ds = loader.dataset
    model = make_model(ds.feature_dim)
    model.save_path = tmp_path
    smallest = eager_reference(ds, [1])                            # 296 nodes, 3,274 edges
    assert smallest['n'] == min(eager_reference(ds, [i])['n'] for i in range(6))
    cap = Capacities(smallest['n'], smallest['n'], smallest['e'], batch_input_atoms(ds, [[0, 1], [2, 3], [4, 5]]))
    model.val(loader, predictions_file=tmp_path / 'eager.txt')
    model.val(loader, predictions_file=tmp_path / 'forced.txt', capture=True,
              capture_options=dict(probe_batches=1, capacities=cap))
    assert model.last_val_stats == dict(eager=1, replayed=0, fallback=2)
    assert (tmp_path / 'pose_forced.txt').read_text() == (tmp_path / 'pose_eager.txt').read_text()


def test_refusals_name_their_reason():
    from pointvs_amd.captured_scoring import FixedShapeScorer
    _, ds = setting('cli_default')
    _, turned = setting('cli_default', rot=True)
    cap = generous_capacities(ds, [0, 1])
    with pytest.raises(NotImplementedError, match='fp64'):
        FixedShapeScorer(make_model(ds.feature_dim).double(), ds, 2, cap, device=DEV)
    with pytest.raises(NotImplementedError, match='edge_residual'):
        FixedShapeScorer(make_model(ds.feature_dim, edge_residual=True), ds, 2, cap, device=DEV)
    with pytest.raises(NotImplementedError, match='rot=True'):
        FixedShapeScorer(make_model(ds.feature_dim), turned, 2, cap, device=DEV)


@needs_caching_allocator
def test_capture_val_through_the_command_line(tmp_path):
    run = tmp_path / 'run'
    model = load_cli().main(['egnn', str(run), '--test_data_root_pose', str(DATAROOT), '--test_types_pose',
                             str(DATAROOT / 'chembl6.types'), '--layers', '2', '-b', '1', '--radius', '6',
                             '--capture_val'])
    # six batches of one: four probes, then two captured steps (the last two complexes are the file's largest, so either
    # may overflow the probes' capacities and be rebuilt eagerly - the file is the same)
    stats = model.last_val_stats
    assert stats['eager'] == 4 and stats['replayed'] + stats['fallback'] == 2
    lines = (run / 'pose_predictions.txt').read_text().splitlines()
    wanted = [ln.split() for ln in (DATAROOT / 'chembl6.types').read_text().splitlines()]
    assert len(lines) == len(wanted)
    for line, row in zip(lines, wanted):
        label, _, score, rec, lig = line.split()
        assert (float(label), rec, lig) == (float(row[0]), row[3], row[4]) and 0.0 <= float(score) <= 1.0
