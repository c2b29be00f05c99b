"""GPU checks of the parquet data-root loader (pointvs_amd/parquet_data.py, csrc/complex_build.hip): batches built on
the device equal, array for array, what the reference's loader returned for the same samples (tests/golden/dataroot_*.npz);
crop edge cases on hand-made pools against numpy in fp64; rot=True; augmented actives; and two end-to-end runs."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden'
DATAROOT = GOLDEN / 'dataroot'
SETTINGS = ('ref_test', 'ref_test_smina', 'cli_default', 'r6_smina', 'noncompact', 'atomic_noh', 'rmsd', 'aug2',
            'regression')
DEV = 'cuda:0'

_CACHE = {}


def setting(name, **extra):
    """(golden arrays, dataset) of a golden setting; built once per argument set and shared."""
    from pointvs_amd.parquet_data import PygPointCloudDataset
    key = (name, tuple(sorted(extra.items())))
    if key not in _CACHE:
        z = np.load(GOLDEN / f'dataroot_{name}.npz')
        meta = json.loads(str(z['settings']))
        ds = PygPointCloudDataset(DATAROOT, types_fname=DATAROOT / meta['types'],
                                  **{'rot': False, **meta['kwargs'], **extra})
        _CACHE[key] = ({k: z[k] for k in z.files}, ds)
    return _CACHE[key]


def golden_batch(z, indices):
    """The golden samples `indices` collated as the loader collates them (numpy)."""
    npt, ept = z['node_ptr'], z['edge_ptr']
    x = np.concatenate([z['x'][npt[i]:npt[i + 1]] for i in indices]).astype(np.float32)
    pos = np.concatenate([z['pos'][npt[i]:npt[i + 1]] for i in indices])
    sizes = [int(npt[i + 1] - npt[i]) for i in indices]
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    ei = np.concatenate([z['edge_index'][:, ept[i]:ept[i + 1]].astype(np.int64) + offsets[k]
                         for k, i in enumerate(indices)], axis=1)
    et = np.concatenate([z['edge_type'][ept[i]:ept[i + 1]] for i in indices]).astype(np.int64)
    batch = np.repeat(np.arange(len(indices)), sizes)
    return dict(x=x, pos=pos, edge_index=ei, edge_attr=np.eye(3, dtype=np.int64)[et], batch=batch,
                y=np.stack([z['y'][i] for i in indices]), ptr=offsets,
                edge_counts=[int(ept[i + 1] - ept[i]) for i in indices])


def assert_batch_equals(b, g):
    assert b.x.dtype == torch.float32 and b.pos.dtype == torch.float32
    assert b.edge_index.dtype == torch.int64 and b.edge_attr.dtype == torch.int64 and b.batch.dtype == torch.int64
    assert tuple(b.x.shape) == g['x'].shape, (tuple(b.x.shape), g['x'].shape)       # the node count
    assert np.array_equal(b.x.cpu().numpy(), g['x'])
    assert np.array_equal(b.pos.cpu().numpy(), g['pos'])            # golden pos is the reference's p.float()
    assert np.array_equal(b.edge_index.cpu().numpy(), g['edge_index'])
    assert np.array_equal(b.edge_attr.cpu().numpy(), g['edge_attr'])
    assert np.array_equal(b.batch.cpu().numpy(), g['batch'])
    assert np.array_equal(b.y.cpu().numpy(), g['y'].astype(b.y.cpu().numpy().dtype))
    assert np.array_equal(b.ptr.numpy(), g['ptr']) and b.num_graphs == len(g['ptr']) - 1
    assert b.graph_node_counts == np.diff(g['ptr']).tolist() and b.graph_edge_counts == g['edge_counts']
    assert b.edge_layout == 'generate_edges'


@pytest.mark.parametrize('name', SETTINGS)
def test_batches_equal_the_reference_loader(name):
    """Every sample of every setting, in batches of 1, of 2 (the test resources and the chembl complexes pair up on one
    receptor each) and of all samples; the smallest is the 82-node / 642-edge complex of the reference's own test.
    Integer and comparison results: no tolerance."""
    z, ds = setting(name)
    n = len(z['order'])
    groups = [[i] for i in range(n)] + [list(range(k, min(k + 2, n))) for k in range(0, n, 2)] + [list(range(n))]
    groups.append(list(range(n))[::-1])      # and out of file order
    for indices in groups:
        b = ds.build_batch(indices, device=DEV)
        assert_batch_equals(b, golden_batch(z, indices))
        assert [str(f) for f in b.lig_fname] == [str(z['ligand_fnames'][i]) for i in indices]
        assert [str(f) for f in b.rec_fname] == [str(z['receptor_fnames'][i]) for i in indices]
    if name == 'ref_test_smina':
        assert tuple(b.x.shape) == (164, 12) and b.graph_edge_counts == [642, 642]


# ---- hand-made pools ------------------------------------------------------------------------------------------------

def write_root(tmp_path, complexes):
    """complexes: list of (ligand atoms, receptor atoms), each a list of (x, y, z, atomic_number, smina type).
    Writes one parquet per structure and a types file; returns (root, types file)."""
    import pandas as pd
    lines = []
    for k, (lig, rec) in enumerate(complexes):
        for kind, atoms, bp in (('lig', lig, 0), ('rec', rec, 1)):
            a = np.array(atoms, dtype=np.float64).reshape(-1, 5)
            pd.DataFrame({'x': a[:, 0], 'y': a[:, 1], 'z': a[:, 2], 'atomic_number': a[:, 3].astype(np.int64),
                          'types': a[:, 4].astype(np.int64), 'bp': bp}).to_parquet(tmp_path / f'{kind}_{k}.parquet')
        lines.append(f'{k % 2} -1 -1.0 rec_{k}.parquet lig_{k}.parquet')
    (tmp_path / 'hand.types').write_text('\n'.join(lines) + '\n')
    return tmp_path, tmp_path / 'hand.types'


def numpy_complex(ds, item, lig_matrix=None):
    """The reference's parquets_to_inputs for one sample in numpy fp64, from the dataset's host pool:
    (xyz [n,3] fp64, features [n,F] fp32, bp [n])."""
    from pointvs_amd.parquet_data import apply_matrix
    lig = ds.ligand_coordinates(item)
    if lig_matrix is not None:
        lig = apply_matrix(lig, lig_matrix)
    rec = ds.receptor_coordinates(item)
    lo, hi = ds.lig_pool['ptr'][ds.lig_ids[item]:ds.lig_ids[item] + 2]
    lig_z, lig_t = ds.lig_pool['z'][lo:hi], ds.lig_pool['types'][lo:hi]
    lo, hi = ds.rec_pool['ptr'][ds.rec_ids[item]:ds.rec_ids[item] + 2]
    rec_z, rec_t = ds.rec_pool['z'][lo:hi], ds.rec_pool['types'][lo:hi]
    d = lig[:, None, :] - rec[None, :, :]                       # cdist(ligand, receptor): fp64, sums in index order
    dist = np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])
    near = (dist < ds.radius).any(axis=0)
    xyz = np.concatenate([lig, rec[near]])
    z = np.concatenate([lig_z, rec_z[near]])
    t = np.concatenate([lig_t, rec_t[near]])
    bp = np.concatenate([np.zeros(len(lig), np.int64), np.ones(int(near.sum()), np.int64)])
    if not ds.polar_hydrogens:
        keep = z > 1
        xyz, z, t, bp = xyz[keep], z[keep], t[keep], bp[keep]
    if ds.use_atomic_numbers:
        t = np.array([ds.atomic_number_to_index[int(v)] for v in z], dtype=np.int64)
    cls = t.astype(np.int64) + bp * ds.n_features
    feats = np.zeros((len(cls), ds.feature_dim), dtype=np.float32)
    if ds.compact:
        feats[np.arange(len(cls)), cls % ds.n_features] = 1
        feats[:, -1] = cls // ds.n_features
    else:
        feats[np.arange(len(cls)), cls] = 1
    return xyz, feats, bp


def assert_matches_numpy(ds, b, indices, lig_matrices=None, rotations=None):
    """Node tables against numpy_complex, edges against the generate_edges oracle on the fp32 coordinates."""
    from oracle.generate_edges_oracle import generate_edges
    from pointvs_amd.parquet_data import apply_matrix
    edge_radius = ds.edge_radius if ds.edge_radius > 0 else 4
    intra = 2.0 if ds.estimate_bonds else edge_radius
    x, pos, bp = b.x.cpu().numpy(), b.pos.cpu().numpy(), b.bp.cpu().numpy()
    ei, ea = b.edge_index.cpu().numpy(), b.edge_attr.cpu().numpy()
    n0 = e0 = 0
    for k, item in enumerate(indices):
        xyz, feats, bp_ref = numpy_complex(ds, item, None if lig_matrices is None else lig_matrices[k])
        n1 = n0 + len(xyz)
        assert b.graph_node_counts[k] == len(xyz), (item, b.graph_node_counts[k], len(xyz))
        shown = xyz if rotations is None else apply_matrix(xyz, rotations[k])
        assert np.array_equal(pos[n0:n1], shown.astype(np.float32)), item
        assert np.array_equal(x[n0:n1], feats) and np.array_equal(bp[n0:n1], bp_ref), item
        _, (rows, cols), attrs = generate_edges(xyz.astype(np.float32), bp_ref, edge_radius, intra, prune=False)
        e1 = e0 + len(rows)
        assert b.graph_edge_counts[k] == len(rows), item
        assert np.array_equal(ei[:, e0:e1], np.stack([rows, cols]) + n0), item
        assert np.array_equal(ea[e0:e1], np.eye(3, dtype=np.int64)[attrs]), item
        n0, e0 = n1, e1
    assert n0 == len(x) and e0 == ei.shape[1]


def hand_made_complexes(r):
    up, down = np.nextafter(r, np.inf), np.nextafter(r, 0.0)
    C, N, O, H = (6, 1), (7, 5), (8, 7), (1, 11)          # (atomic number, a smina type)
    at = (lambda x, y, z, kind: (x, y, z) + kind)
    lig3 = [at(0.0, 0.0, 0.0, C), at(1.5, 0.0, 0.0, N), at(0.0, 1.25, 0.0, O)]
    far = [at(20.0 + k, 20.0, 20.0, C) for k in range(4)]
    # exactly r / one ulp inside / one ulp outside of the single ligand atom at the origin, along the axes; 1.8, 2.4 is
    # the oblique 3-4-5 direction (1.8^2 + 2.4^2 rounds as numpy decides: the expectation is computed, not assumed)
    shell = [at(r, 0.0, 0.0, C), at(0.0, down, 0.0, N), at(0.0, 0.0, up, O), at(-r, 0.0, 0.0, C), at(0.0, -down, 0.0, N),
             at(1.8, 2.4, 0.0, O), at(np.nextafter(1.8, 0.0), 2.4, 0.0, C), at(1.8, 0.0, np.nextafter(2.4, 3.0), N)]
    big = [at(30.0 + 0.5 * k, -15.0, 8.0, C) for k in range(300)]
    big[270] = at(1.0, 1.0, 1.0, N)
    big[299] = at(-1.0, 0.5, 2.0, O)
    lig_h = [at(0.0, 0.0, 0.0, C), at(0.0, 0.0, 1.0, H), at(9.0, 0.0, 0.0, H)]
    rec_h = [at(0.0, 0.0, 2.5, H), at(1.0, 0.0, 2.0, H), at(10.5, 0.0, 0.0, C), at(11.0, 0.5, 0.0, H), at(20.0, 0.0, 0.0, C)]
    return [(lig3, far), ([at(0.0, 0.0, 0.0, C)], shell), (lig3, big), (lig_h, rec_h),
            ([at(0.25, 0.0, 0.0, O)], far[:3] + [at(1.0, 1.0, 0.0, N)])]


def test_crop_edge_cases_on_hand_made_pools(tmp_path):
    """3-8 atoms per structure (one receptor of 300), expected results from numpy in fp64: an empty crop, a one-atom
    ligand, distances of exactly the radius and one ulp to either side of it (axis-aligned and oblique), survivors only
    in the workgroup's second pass over a receptor, hydrogens dropped on one side, a contact through a hydrogen only."""
    from pointvs_amd.parquet_data import PygPointCloudDataset
    r = 3.0
    up, down = np.nextafter(r, np.inf), np.nextafter(r, 0.0)
    root, types = write_root(tmp_path, hand_made_complexes(r))
    for kwargs in (dict(use_atomic_numbers=True, polar_hydrogens=False, compact=True),
                   dict(use_atomic_numbers=True, polar_hydrogens=True, compact=False),
                   dict(use_atomic_numbers=False, polar_hydrogens=False, compact=True)):
        ds = PygPointCloudDataset(root, radius=r, edge_radius=4, estimate_bonds=False, types_fname=types, **kwargs)
        for indices in ([0, 1, 2, 3, 4], [1], [2], [3, 0]):
            b = ds.build_batch(indices, device=DEV)
            assert_matches_numpy(ds, b, indices)
        b = ds.build_batch([0, 1, 2, 3, 4], device=DEV)
        counts = b.graph_node_counts
        assert counts[0] == 3                                   # nothing inside the radius: the ligand alone
        assert counts[2] == 3 + 2                               # atoms 270 and 299 of the 300
        if kwargs['polar_hydrogens']:
            assert counts[3] == 3 + 4                           # rec_h[:2] by the carbon, [2:4] by the far hydrogen
        else:
            assert counts[3] == 1 + 1                           # both ligand H and 3 receptor H dropped; the carbon at
            #                                                     10.5 stays though only a ligand HYDROGEN touches it
    # the shell, stated outright: of the axis-aligned atoms only the one-ulp-inside pair is kept
    xyz, _, _ = numpy_complex(ds, 1)
    kept = {tuple(v) for v in xyz[1:].tolist()}
    assert (0.0, down, 0.0) in kept and (0.0, -down, 0.0) in kept
    assert not {(r, 0.0, 0.0), (-r, 0.0, 0.0), (0.0, 0.0, up)} & kept


def test_rot_moves_pos_only_and_is_reproducible():
    """rot=True: x and the edge list are bit-equal to rot=False (the edges come from the unrotated coordinates), pos is
    the rotated fp64 coordinate rounded to fp32. The device evaluates x @ R with one rounding per operation; the host
    reference is the reference's own ((x - mean) @ R) + mean @ R in numpy fp64. Their distance after rounding both to
    fp32, measured on the CPU over these six complexes (2,820 coordinates up to 69.2 A) with these rotations: 0 - the
    two fp64 values differ by a few 1e-14 and round to the same fp32 everywhere; the test measures it again and allows
    the device that plus 2 fp32 ulp of the largest coordinate. The tables are orthogonal with determinant +1 to 1e-12; the same (seed, epoch, index) gives
    the same batch bit for bit, another epoch another rotation."""
    from pointvs_amd.parquet_data import apply_matrix, rotate_about_mean
    z, plain = setting('aug2')
    _, ds = setting('aug2', rot=True, seed=11)
    indices = [0, 1, 2, 3, 4, 5]
    fixed = plain.build_batch(indices, device=DEV)
    a = ds.build_batch(indices, epoch=4, device=DEV)
    again = ds.build_batch(indices, epoch=4, device=DEV)
    other = ds.build_batch(indices, epoch=5, device=DEV)
    for key in ('x', 'edge_index', 'edge_attr', 'batch', 'y'):
        assert torch.equal(getattr(a, key), getattr(fixed, key)), key
    for key in ('x', 'pos', 'edge_index', 'edge_attr', 'batch', 'y'):
        assert torch.equal(getattr(a, key), getattr(again, key)), key
    assert not torch.equal(a.pos, other.pos) and not torch.equal(a.pos, fixed.pos)
    _, _, rots = ds.host_draws(indices, epoch=4)
    for m in rots:
        assert np.abs(m @ m.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(m) - 1.0) < 1e-12
    assert_matches_numpy(ds, a, indices, rotations=rots)      # bit-equal to the per-operation host evaluation
    pos = a.pos.cpu().numpy()
    measured, worst, n0 = 0.0, 0.0, 0
    for k, item in enumerate(indices):
        xyz, _, _ = numpy_complex(ds, item)
        want = rotate_about_mean(xyz, rots[k])
        emulated = apply_matrix(xyz, rots[k]).astype(np.float32)
        measured = max(measured, float(np.abs(emulated.astype(np.float64) - want.astype(np.float32)).max()))
        got = pos[n0:n0 + len(xyz)]
        ulp = float(np.spacing(np.float32(np.abs(want).max())))
        worst = max(worst, float(np.abs(got.astype(np.float64) - want.astype(np.float32)).max()))
        assert np.abs(got.astype(np.float64) - want.astype(np.float32)).max() <= measured + 2 * ulp
        n0 += len(xyz)
    print(f'rot: host-emulated distance {measured:.3g}, device distance {worst:.3g}')


def test_augmented_actives_are_turned_and_cropped_anew():
    from pointvs_amd.parquet_data import angle_3d, apply_matrix
    z, ds = setting('aug2', seed=5)
    n = len(z['order'])
    indices = list(range(n, len(ds))) + [0]
    assert all(ds.is_augmented(i) for i in indices[:-1]) and (np.asarray(ds.labels)[indices[:-1]] == 0).all()
    b = ds.build_batch(indices, epoch=1, device=DEV)
    _, mats, _ = ds.host_draws(indices, epoch=1)
    assert np.array_equal(mats[-1], np.eye(3))
    assert (b.y.cpu().numpy() == [0] * 6 + [int(z['labels'][0])]).all()
    assert_matches_numpy(ds, b, indices, lig_matrices=mats)          # the crop of the TURNED ligand, exactly
    changed = 0
    for k, item in enumerate(indices[:-1]):
        lig = ds.ligand_coordinates(item)
        turned = apply_matrix(lig, mats[k])
        d0 = np.linalg.norm(lig[:, None] - lig[None], axis=-1)
        d1 = np.linalg.norm(turned[:, None] - turned[None], axis=-1)
        assert np.abs(d0 - d1).max() < 1e-12                          # rigid, to fp64 rounding (coordinates < 64 A)
        assert angle_3d(lig[0], turned[0]) >= np.pi * 30 / 180
        plain_nodes = int(z['node_ptr'][ds.lig_ids[item] + 1] - z['node_ptr'][ds.lig_ids[item]])
        changed += b.graph_node_counts[k] != plain_nodes
    assert changed >= 4       # turned out of its pocket, a ligand meets other receptor atoms
    assert_batch_equals(ds.build_batch([0], epoch=1, device=DEV), golden_batch(z, [0]))


def test_device_status_raises(tmp_path):
    """A receptor element outside the atomic-number table has class 2 * n_features under the non-compact encoding: the
    reference's one_hot raises, and so does the batch builder (from its device status word)."""
    from pointvs_amd.parquet_data import PygPointCloudDataset
    lig = [(0.0, 0.0, 0.0, 6, 1)]
    root, types = write_root(tmp_path, [(lig, [(1.0, 0.0, 0.0, 34, 1)])])
    ds = PygPointCloudDataset(root, radius=3, edge_radius=4, types_fname=types, use_atomic_numbers=True,
                              polar_hydrogens=True, compact=False)
    with pytest.raises(ValueError, match='outside the feature encoding'):
        ds.build_batch([0], device=DEV)
    compact = PygPointCloudDataset(root, radius=3, edge_radius=4, types_fname=types, use_atomic_numbers=True,
                                   polar_hydrogens=True, compact=True)
    x = compact.build_batch([0], device=DEV).x.cpu().numpy()          # compact: class 0 with 2 in the last column
    assert x[1].tolist() == [1.0] + [0.0] * 11 + [2.0]


# ---- end to end -----------------------------------------------------------------------------------------------------

def load_cli():
    spec = importlib.util.spec_from_file_location('pvs_entry', ROOT / 'point_vs.py')
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_point_vs_trains_and_scores_from_the_data_root(tmp_path):
    run = tmp_path / 'run'
    model = load_cli().main(['egnn', str(run), '--train_data_root_pose', str(DATAROOT), '--train_types_pose',
                             str(DATAROOT / 'chembl6.types'), '--test_data_root_pose', str(DATAROOT),
                             '--test_types_pose', str(DATAROOT / 'chembl6.types'), '-ep', '1', '--layers', '2', '-b', '4',
                             '--radius', '6', '--augmented_actives', '1'])
    assert model.p_epoch == 1 and (run / 'checkpoints' / 'pose_ckpt_epoch_1.pt').exists()
    lines = (run / 'pose_predictions.txt').read_text().splitlines()
    wanted = [ln.split() for ln in (DATAROOT / 'chembl6.types').read_text().splitlines()]
    assert len(lines) == len(wanted)
    for line, row in zip(lines, wanted):
        label, _, score, rec, lig = line.split()
        assert (float(label), rec, lig) == (float(row[0]), row[3], row[4]) and 0.0 <= float(score) <= 1.0


def test_logits_equal_the_existing_batch_path_on_the_golden_arrays():
    """One model, one batch: the loader's device-built batch against the golden arrays of the same samples collated by
    Batch.from_data_list (what an `.npz` dump of the reference loader goes through). Bit for bit."""
    from pointvs_amd.graph import Batch, Data
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.parquet_data import get_data_loader
    z, _ = setting('cli_default')
    meta = json.loads(str(z['settings']))
    kwargs = {k: v for k, v in meta['kwargs'].items()}
    loader = get_data_loader(DATAROOT, types_fname=DATAROOT / meta['types'], mode='val', batch_size=6, rot=False,
                             device=DEV, **kwargs)
    (batch,) = list(loader)
    npt, ept = z['node_ptr'], z['edge_ptr']
    items = [Data(x=torch.from_numpy(z['x'][npt[i]:npt[i + 1]].astype(np.float32)),
                  pos=torch.from_numpy(z['pos'][npt[i]:npt[i + 1]]),
                  edge_index=torch.from_numpy(z['edge_index'][:, ept[i]:ept[i + 1]].astype(np.int64)),
                  edge_attr=torch.nn.functional.one_hot(torch.from_numpy(z['edge_type'][ept[i]:ept[i + 1]].astype(np.int64)), 3),
                  y=torch.tensor(int(z['y'][i])), lig_fname=str(z['ligand_fnames'][i]),
                  rec_fname=str(z['receptor_fnames'][i]), edge_layout='generate_edges') for i in range(6)]
    ref = Batch.from_data_list(items).to(DEV)
    torch.manual_seed(0)
    model = SartorrasEGNN(Path('/tmp/pvs_parquet_logits'), 2e-3, 1e-4, silent=True, k=32, num_layers=3,
                          dim_input=int(z['feature_dim']), dim_output=1, residual=True, edge_attention=True,
                          model_task='classification').cuda().eval()
    with torch.no_grad():
        y_new = model.unpack_input_data_and_predict(batch)[0]
        y_ref = model.unpack_input_data_and_predict(ref)[0]
    assert y_new.shape[0] == 6 and torch.isfinite(y_new).all()
    assert torch.equal(y_new, y_ref), (y_new - y_ref).abs().max().item()
