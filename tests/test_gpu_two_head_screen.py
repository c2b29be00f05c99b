"""Screening a two-headed model (MultitaskSatorrasEGNN) through ReceptorScreen, LibraryScreen and ScreeningSweep with
`tasks`: pose logit and affinity from one trunk pass, against the model's plain forward under set_task(...) on the same
complexes built from oracle edge lists (rel 1e-5 per head, the bound of the screening paths). Receptor of 130 atoms, as
in test_gpu_library_screen.py (three contact-mask words, the last one partial)."""
import tempfile

import numpy as np
import pytest
import torch

from tests._golden import needs_caching_allocator

pytestmark = pytest.mark.gpu

N_REC = 130
SIZES = (1, 64, 0, 7, 33, 20)
KW = dict(dim_input=12, k=32, dim_output=1, num_layers=2, residual=False, edge_residual=False,
          edge_attention=False, normalize=False, tanh=False, dropout=0.0, graphnorm=False, update_coords=True,
          permutation_invariance=False, node_attention=False, gated_residual=False, rezero=False,
          softmax_attention=False, model_task='classification', final_softplus=False)
# (k, layers, affinity outputs, final_softplus)
SHAPES = [dict(k=32, num_layers=2, dim_output=1, final_softplus=False),
          dict(k=64, num_layers=3, dim_output=3, final_softplus=True)]


def _model(seed=0, **flags):
    from pointvs_amd.egnn_multitask import MultitaskSatorrasEGNN
    torch.manual_seed(seed)
    return MultitaskSatorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **dict(KW, **flags)).eval()


def _set(seed, n_lig=64):
    """(ligand [n_lig,3], receptor [130,3], ligand feats, receptor feats): the 130 receptor atoms of a
    screening_set nearest its centre."""
    from pointvs_amd.synthetic import screening_set
    lig, rec, feats = screening_set(seed=seed, n_nodes=n_lig + 400, n_lig=n_lig)
    near = torch.argsort((rec - lig.mean(0)).norm(dim=1))[:N_REC].sort().values
    return lig, rec[near].contiguous(), feats[:n_lig].contiguous(), feats[n_lig:][near].contiguous()


def _slots(lig, lig_feats, sizes, seed):
    """One pose per slot: slot k holds the first sizes[k] ligand atoms (features rolled by k) in a random pose."""
    from pointvs_amd.synthetic import random_poses
    slots = []
    for k, n in enumerate(sizes):
        pose = random_poses(lig[:n], 1, seed=seed + k, max_shift=3.0)[0].contiguous() if n else lig[:0]
        slots.append((lig_feats[:n].roll(k, 0).contiguous(), pose))
    return slots


def _plain(model, slots, rec, rec_feats, radius):
    """[B, 1 + A]: the model's plain forward under set_task('classification'), then under set_task('regression'), on
    the slots' complexes with the oracle's edge lists; the model's task is put back."""
    from oracle.generate_edges_oracle import generate_edges as oracle_edges
    from pointvs_amd.graph import Batch, Data
    items = []
    for feats, pose in slots:
        pos, x = torch.cat([pose, rec], 0), torch.cat([feats, rec_feats], 0)
        _, (rows, cols), attrs = oracle_edges(pos.numpy(), x[:, -1].numpy(), radius, radius, prune=False)
        items.append(Data(x=x, pos=pos, edge_index=torch.from_numpy(np.vstack([rows, cols])).long(),
                          edge_attr=torch.nn.functional.one_hot(torch.from_numpy(attrs).long(), 3),
                          y=torch.tensor(0), lig_fname='l', rec_fname='r'))
    task, out = model.model_task, []
    try:
        for name in ('classification', 'regression'):
            model.set_task(name)
            with torch.no_grad():
                out.append(model(Batch.from_data_list(items).to('cuda')).reshape(len(slots), -1))
    finally:
        model.set_task(task)
    return torch.cat(out, 1)


def _live(model, slots, rec, rec_feats, radius):
    """The model with an affinity head that is alive on these complexes: random weights leave a ReLU head dead (every
    output 0, a column that would test nothing) about every other time - then the head's Linear changes sign. Decided
    on the plain forward, before any screen is made."""
    for _ in range(2):
        if bool((_plain(model, slots, rec, rec_feats, radius)[:, 1:] > 0).any()):
            return model
        with torch.no_grad():
            model.feats_linear_layers_affinity[0].weight.neg_()
            model.feats_linear_layers_affinity[0].bias.neg_()
    raise AssertionError('the affinity head is dead either way round')


def _assert_close(fast, slow, what):
    """max|fast - slow| / max|slow| < 1e-5 per head (column 0: pose; the columns behind it: affinity)."""
    assert fast.shape == slow.shape, (fast.shape, slow.shape)
    for name, cols in (('pose', slice(0, 1)), ('affinity', slice(1, None))):
        err = float((fast[:, cols] - slow[:, cols]).abs().max() / slow[:, cols].abs().max().clamp_min(1e-30))
        print(f'{what} {name}: max|fast-slow|/max|slow| = {err:.3e}')
        assert err < 1e-5, (what, name, err)


@pytest.mark.parametrize('shape', SHAPES, ids=['k32-A1-relu', 'k64-A3-softplus'])
def test_library_screen_both_heads_match_the_plain_forwards(shape):
    from pointvs_amd.screening import LibraryScreen
    lig, rec, lig_feats, rec_feats = _set(7001)
    model = _live(_model(1, **shape), _slots(lig, lig_feats, SIZES, seed=40), rec, rec_feats, 7.0)
    screens = {tasks: LibraryScreen(model, rec.cuda(), rec_feats, len(SIZES), 64, 7.0, tasks=tasks)
               for tasks in ('both', 'pose', 'affinity', None)}
    assert screens[None].tasks == 'pose' and all(s.reuse for s in screens.values())
    for k, sizes in enumerate((SIZES, (20, 0, 64, 33, 1, 7))):
        slots = _slots(lig, lig_feats, sizes, seed=40 + 10 * k)
        both = screens['both'](slots).clone()
        assert both.shape == (len(sizes), 1 + shape['dim_output'])
        _assert_close(both, _plain(model, slots, rec, rec_feats, 7.0), f'{shape} batch {k}')
        assert torch.equal(screens['pose'](slots), both[:, :1])
        assert torch.equal(screens[None](slots), both[:, :1])
        assert torch.equal(screens['affinity'](slots), both[:, 1:])
    for screen in screens.values():
        screen.check()
    assert model.model_task == 'classification'
    model.set_task('regression')
    assert LibraryScreen(model, rec.cuda(), rec_feats, 2, 8, 7.0).tasks == 'affinity'
    assert screens[None].tasks == 'pose'                # (resolved when the screen was made)
    with pytest.raises(ValueError, match="one of 'pose', 'affinity', 'both' or None"):
        LibraryScreen(model, rec.cuda(), rec_feats, 2, 8, 7.0, tasks='regression')


@pytest.mark.parametrize('case', ['edge_residual', 'one-slot'])
def test_library_screen_plain_route_and_one_slot(case):
    """The route without the first-layer reuse (edge_residual: LibraryScreen._plain_forward, the model's trunk and then
    the same head code) and a batch of ONE slot at the padded shape (33 atoms in a 64-atom slot: the pooling ends at
    node_ptr[1], not at the last row)."""
    from pointvs_amd.screening import LibraryScreen
    lig, rec, lig_feats, rec_feats = _set(7004)
    sizes, flags = ((33,), dict()) if case == 'one-slot' else (SIZES, dict(edge_residual=True))
    slots = _slots(lig, lig_feats, sizes, seed=55)
    model = _live(_model(4, **SHAPES[1], **flags), slots, rec, rec_feats, 7.0)
    screens = {tasks: LibraryScreen(model, rec.cuda(), rec_feats, len(sizes), 64, 7.0, tasks=tasks)
               for tasks in ('both', 'pose', 'affinity')}
    assert screens['both'].reuse == (case == 'one-slot')
    both = screens['both'](slots).clone()
    assert both.shape == (len(sizes), 4)
    _assert_close(both, _plain(model, slots, rec, rec_feats, 7.0), case)
    assert torch.equal(screens['pose'](slots), both[:, :1])
    assert torch.equal(screens['affinity'](slots), both[:, 1:])
    for screen in screens.values():
        screen.check()
    assert model.model_task == 'classification'


@pytest.mark.parametrize('batch_size', [3, 1])
@pytest.mark.parametrize('shape', SHAPES, ids=['k32-A1-relu', 'k64-A3-softplus'])
def test_receptor_screen_both_heads_match_the_plain_forwards(shape, batch_size):
    from pointvs_amd.screening import ReceptorScreen
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(7002)
    n_lig = 12
    feats = torch.cat([lig_feats[:n_lig], rec_feats], 0)
    poses = random_poses(lig[:n_lig], batch_size, seed=11, max_shift=3.0)
    slots = [(lig_feats[:n_lig], pose.contiguous()) for pose in poses]
    for flags in (dict(), dict(edge_residual=True)):              # (edge_residual: the route without the reuse)
        model = _live(_model(2, **shape, **flags), slots, rec, rec_feats, 7.0)
        screens = {tasks: ReceptorScreen(model, rec.cuda(), feats, n_lig, batch_size, 7.0, tasks=tasks)
                   for tasks in ('both', 'pose', 'affinity')}
        assert screens['both'].reuse == (not flags)
        both = screens['both'](poses.cuda()).clone()
        assert both.shape == (batch_size, 1 + shape['dim_output'])
        _assert_close(both, _plain(model, slots, rec, rec_feats, 7.0), f'{shape} {flags} B={batch_size}')
        assert torch.equal(screens['pose'](poses.cuda()), both[:, :1])
        assert torch.equal(screens['affinity'](poses.cuda()), both[:, 1:])
        for screen in screens.values():
            screen.check()
        assert model.model_task == 'classification'


@needs_caching_allocator
def test_captured_steps_replay_bit_for_bit():
    """ONE captured 'both' step of LibraryScreen over four compositions, and a captured ReceptorScreen: every replay
    == the eager screen on the same batch."""
    from pointvs_amd.screening import LibraryScreen, ReceptorScreen
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(7003)
    model = _model(3, **SHAPES[1], residual=True, edge_attention=True, tanh=True)
    comps = [(7, 20, 3), (5, 17, 1), (12, 9), (20, 20, 20)]           # B = 3, L_cap = 60
    batches = [_slots(lig, lig_feats, sizes, seed=70 + 10 * k) for k, sizes in enumerate(comps)]
    eager = LibraryScreen(model, rec.cuda(), rec_feats, 3, 20, 7.0, tasks='both')
    want = [eager(slots).clone() for slots in batches]               # (first batch first: the same probe)
    eager.check()
    graph = LibraryScreen(model, rec.cuda(), rec_feats, 3, 20, 7.0, tasks='both').capture(batches[0])
    for k in (2, 3, 1, 0):
        got = graph.replay(batches[k]).clone()
        assert got.shape == (3, 4) and torch.equal(got, want[k]), k
    graph.check()
    feats = torch.cat([lig_feats[:12], rec_feats], 0)
    poses = [random_poses(lig[:12], 3, seed=s, max_shift=3.0).cuda() for s in (5, 6)]
    for tasks in ('both', 'affinity'):
        eager = ReceptorScreen(model, rec.cuda(), feats, 12, 3, 7.0, tasks=tasks)
        want = [eager(p).clone() for p in poses]
        eager.check()
        graph = ReceptorScreen(model, rec.cuda(), feats, 12, 3, 7.0, tasks=tasks).capture(poses[0])
        for k in (1, 0):
            assert torch.equal(graph.replay(poses[k]), want[k]), (tasks, k)
        graph.check()


def _library(lig, lig_feats):
    from pointvs_amd.synthetic import random_poses
    ligs = [('ligA', lig_feats[:12], lig[:12], 7), ('ligB', lig_feats[:9].roll(1, 0), lig[:9] * 0.9, 5),
            ('ligC', lig_feats, lig, 3), ('ligD', lig_feats[:12].roll(3, 0), lig[:12].flip(0), 4),
            ('ligE', lig_feats[5:6], lig[5:6], 2)]
    return [(name, f, random_poses(pos, n, seed=20 + k, max_shift=3.0).cuda()) for k, (name, f, pos, n) in enumerate(ligs)]


@needs_caching_allocator
@pytest.mark.parametrize('shape', SHAPES, ids=['k32-A1-relu', 'k64-A3-softplus'])
def test_run_library_both_heads_end_to_end(tmp_path, shape):
    """Five ligands (12, 9, 70, 12, 1 atoms; 7, 5, 3, 4, 2 poses), batch of 4, max_lig_atoms 64 (the 70-atom ligand takes
    its size bucket): scores, the two predictions files and the hits file, with the sigmoid on the pose column and
    without it."""
    from pointvs_amd.predictions import format_hit_lines
    from pointvs_amd.radius_graph import PoseBatcher
    from pointvs_amd.screening import ScreeningSweep
    lig, rec, lig_feats, rec_feats = _set(7005, n_lig=70)
    n_aff = shape['dim_output']
    work = _library(lig, lig_feats)
    model = _live(_model(2, **dict(shape, num_layers=3)), [(work[0][1], work[0][2][0].cpu())], rec, rec_feats, 6.0)
    # the one-complex plain forwards, raw, once: {name: [P, 1 + A]}
    slow = {}
    for name, f, poses in work:
        plain = PoseBatcher(rec.cuda(), torch.cat([f, rec_feats], 0), f.shape[0], 1, edge_radius=6.0)
        rows = []
        for k in range(poses.shape[0]):
            heads = []
            for task in ('classification', 'regression'):
                model.set_task(task)
                with torch.no_grad():
                    heads.append(model(plain.load(poses[k:k + 1])).reshape(-1))
            rows.append(torch.cat(heads))
        slow[name] = torch.stack(rows)
    model.set_task('classification')
    sweep = ScreeningSweep(model, rec.cuda(), rec_feats, edge_radius=6.0, batch_size=4, tasks='both')
    raw = None
    for sigmoid in (False, None):
        out = tmp_path / f'sigmoid_{sigmoid}'
        got = sweep.run_library(work, predictions_file=out / 'library.txt', sigmoid=sigmoid, hits_file=out / 'hits.txt')
        assert sorted(sweep.buckets) == [70] and list(got) == [name for name, _, _ in work]
        assert not (out / 'library.txt').exists()
        pose_lines = (out / 'pose_library.txt').read_text().splitlines()
        aff_lines = (out / 'affinity_library.txt').read_text().splitlines()
        hit_lines = (out / 'hits.txt').read_text().splitlines()
        assert len(pose_lines) == len(aff_lines) == 21 and len(hit_lines) == 5
        if sigmoid is False:
            raw = {name: scores.clone() for name, scores in got.items()}
        at = 0
        for i, (name, f, poses) in enumerate(work):
            want = slow[name].clone()
            if sigmoid is None:
                want[:, 0] = torch.sigmoid(want[:, 0])
                assert torch.equal(got[name][:, 1:], raw[name][:, 1:])          # the sigmoid: the pose column only
            _assert_close(got[name], want, f'{name} sigmoid={sigmoid}')
            for k in range(poses.shape[0]):
                row = got[name][k].tolist()
                assert pose_lines[at] == f'{row[0]:.3f} | receptor {name}_pose{k}'
                assert aff_lines[at] == ' '.join(f'{v:.3f}' for v in row[1:]) + f' | receptor {name}_pose{k}'
                at += 1
            # the best pose: argmax of the RAW pose logits on the host, the lowest index on ties
            best, row = sweep.hits[name]
            assert best == int(np.argmax(raw[name][:, 0].cpu().numpy()))
            assert torch.equal(row[1:], got[name][best, 1:].cpu())
            assert abs(float(row[0]) - float(got[name][best, 0])) <= (0.0 if sigmoid is False else 1e-6)
            assert hit_lines[i] == format_hit_lines([best], [row.numpy()], 'receptor', [name])[0]
            assert hit_lines[i].endswith(f' | receptor {name}_pose{best}') and len(hit_lines[i].split(' | ')[0].split()) == 1 + n_aff
    assert model.model_task == 'classification'


@needs_caching_allocator
def test_single_head_sweep_is_unchanged_and_refuses_tasks(tmp_path):
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.screening import ScreeningSweep
    lig, rec, lig_feats, rec_feats = _set(7006, n_lig=70)
    torch.manual_seed(4)
    kw = {k: v for k, v in KW.items() if k != 'final_softplus'}
    model = SartorrasEGNN(tempfile.mkdtemp(), 2e-3, 1e-4, silent=True, **dict(kw, num_layers=3)).eval()
    work = _library(lig, lig_feats)
    plain = ScreeningSweep(model, rec.cuda(), rec_feats, edge_radius=6.0, batch_size=4)
    keyword = ScreeningSweep(model, rec.cuda(), rec_feats, edge_radius=6.0, batch_size=4, tasks=None)
    assert plain.tasks is None and keyword.tasks is None
    a = plain.run_library(work, predictions_file=tmp_path / 'a.txt')
    b = keyword.run_library(work, predictions_file=tmp_path / 'b.txt', hits_file=tmp_path / 'hits.txt')
    assert list(a) == list(b) and all(torch.equal(a[name], b[name]) for name in a)
    assert (tmp_path / 'a.txt').read_text() == (tmp_path / 'b.txt').read_text()
    assert len((tmp_path / 'a.txt').read_text().splitlines()) == 21
    lines = (tmp_path / 'hits.txt').read_text().splitlines()
    for i, (name, _, _) in enumerate(work):           # (sigmoid is monotonic: here the argmax of the scores themselves)
        best = int(np.argmax(b[name][:, 0].cpu().numpy()))
        assert keyword.hits[name][0] == best
        assert lines[i] == f'{float(b[name][best, 0]):.3f} | receptor {name}_pose{best}'
    for tasks in ('both', 'pose'):
        with pytest.raises(ValueError, match='has one head'):
            ScreeningSweep(model, rec.cuda(), rec_feats, edge_radius=6.0, batch_size=4, tasks=tasks)


@needs_caching_allocator
def test_three_captured_sweeps_alternating_keep_their_status_words():
    """Three captured LibraryScreen steps of one model ('both', 'pose', 'affinity') replayed in turn over a 512-ligand
    library at the cfg5 receptor: with the builders' status word cleared by a 4-byte memset node, the second round
    read the word as 0x2c2c2c2c (a valid lig_ptr reported as no table). The word is now stored by the builder's first
    kernel: no sweep raises, and every round gives the first round's scores bit for bit."""
    from pointvs_amd.screening import ScreeningSweep
    from pointvs_amd.synthetic import CONFIGS, random_poses, screening_set
    lig30, rec, feats = screening_set()
    rec_feats, rec = feats[lig30.shape[0]:].cuda(), rec.cuda()
    lig, _, feats64 = screening_set(seed=5064, n_lig=64)
    model = _model(0, **{k: v for k, v in CONFIGS['cfg2']['model'].items() if k in KW})
    sizes = torch.randint(8, 65, (512,), generator=torch.Generator().manual_seed(20260405)).tolist()
    work = [(f'lig{k}', feats64[:n].roll(k, 0).contiguous(),
             random_poses(lig[:n], 9, seed=100 + k, max_shift=6.0, device='cuda')) for k, n in enumerate(sizes)]
    sweeps = {tasks: ScreeningSweep(model, rec, rec_feats, 10.0, 128, tasks=tasks) for tasks in ('both', 'pose', 'affinity')}
    first = {}
    for rnd in range(3):
        for tasks, sweep in sweeps.items():
            got = torch.cat(list(sweep.run_library(work, sigmoid=False).values()), 0)
            assert sweep.library._captured
            assert torch.equal(got, first.setdefault(tasks, got)), (rnd, tasks)
    assert torch.equal(first['both'][:, :1], first['pose']) and torch.equal(first['both'][:, 1:], first['affinity'])
