"""CPU-side checks of the parquet data-root dataset (pointvs_amd/parquet_data.py): what the constructor derives from a
types file equals what the reference's PygPointCloudDataset derived (tests/golden/dataroot_*.npz, written by
tests/golden/make_golden_dataroot.py), the options the path does not build raise by name, the reference's import paths
resolve, and the new C entries are declared, bound and exported."""
import ctypes
import json
import re
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / 'tests' / 'golden'
DATAROOT = GOLDEN / 'dataroot'
SETTINGS = ('ref_test', 'ref_test_smina', 'cli_default', 'r6_smina', 'noncompact', 'atomic_noh', 'rmsd', 'aug2',
            'regression')


def load_setting(name):
    z = np.load(GOLDEN / f'dataroot_{name}.npz')
    meta = json.loads(str(z['settings']))
    return z, meta['types'], meta['kwargs']


def make_dataset(name, **extra):
    from pointvs_amd.parquet_data import PygPointCloudDataset
    z, types, kwargs = load_setting(name)
    return z, PygPointCloudDataset(DATAROOT, types_fname=DATAROOT / types, **{'rot': False, **kwargs, **extra})


@pytest.mark.parametrize('name', SETTINGS)
def test_lists_labels_and_sizes_equal_the_reference(name):
    z, ds = make_dataset(name)
    assert [str(f) for f in ds.ligand_fnames] == z['ligand_fnames'].tolist()
    assert [str(f) for f in ds.receptor_fnames] == z['receptor_fnames'].tolist()
    assert len(ds) == int(z['length'])
    assert ds.feature_dim == int(z['feature_dim']) and ds.n_features == int(z['n_features'])
    if name == 'regression':
        for key in ('pki', 'pkd', 'ic50'):
            assert np.array_equal(np.array(getattr(ds, key), dtype=np.float64), z[key])
        y = np.array([ds.label(i) for i in range(len(ds))], dtype=np.float32)
        assert np.array_equal(y, z['y'])
        assert ds.sample_weights is None
        return
    assert np.array_equal(np.asarray(ds.labels).astype(np.int64), z['labels'])
    assert ds.pre_aug_ds_len == int(z['pre_aug_ds_len'])
    n_plain = len(z['order'])
    assert np.array_equal(np.array([ds.label(i) for i in range(n_plain)]), z['y'])
    if z['sample_weights'].size:
        assert np.array_equal(ds.sample_weights.numpy(), z['sample_weights'])     # 1 / class count: exact
        assert ds.sampler is not None
    else:
        assert ds.sample_weights is None and ds.sampler is None


def test_augmented_actives_sit_at_the_end_with_label_zero():
    z, ds = make_dataset('aug2')
    n = len(z['order'])
    assert len(ds) == n + 2 * 3 and ds.pre_aug_ds_len == n
    actives = [f for f, lab in zip(ds.ligand_fnames[:n], ds.labels[:n]) if lab == 1]
    assert ds.ligand_fnames[n:] == [f for f in actives for _ in range(2)]
    assert (np.asarray(ds.labels[n:]) == 0).all()
    assert [ds.is_augmented(i) for i in range(len(ds))] == [False] * n + [True] * 6


def test_pool_holds_every_unique_file_once():
    _, ds = make_dataset('cli_default')
    assert ds.rec_files == ['receptors/10498.parquet', 'receptors/11534.parquet', 'receptors/10378.parquet']
    assert ds.rec_ids.tolist() == [0, 0, 1, 1, 2, 2] and ds.lig_ids.tolist() == list(range(6))
    assert ds.rec_pool['xyz'].dtype == np.float64 and ds.rec_pool['xyz'].shape == (ds.rec_pool['ptr'][-1], 3)
    assert len(ds.rec_pool['ptr']) == 4 and len(ds.lig_pool['ptr']) == 7
    _, aug = make_dataset('aug2')
    assert len(aug.lig_files) == 6 and len(aug) == 12       # the augmented copies share their ligand's pool entry
    import pandas as pd
    df = pd.read_parquet(DATAROOT / 'receptors/11534.parquet')
    lo, hi = ds.rec_pool['ptr'][1:3]
    assert np.array_equal(ds.rec_pool['xyz'][lo:hi], df[['x', 'y', 'z']].to_numpy())
    assert np.array_equal(ds.rec_pool['z'][lo:hi], df['atomic_number'].to_numpy())
    assert np.array_equal(ds.rec_pool['types'][lo:hi], df['types'].to_numpy())


@pytest.mark.parametrize('kwargs, flag', [
    (dict(prune=True), 'prune'),
    (dict(p_remove_entity=0.5), 'p_remove_entity'),
    (dict(include_strain_info=True), 'include_strain_info'),
    (dict(bp=0), 'bp'),
    (dict(use_atomic_numbers=False, polar_hydrogens=True), 'hydrogens'),
])
def test_unsupported_options_raise_by_name(kwargs, flag):
    with pytest.raises(NotImplementedError, match=flag):
        make_dataset('r6_smina', **kwargs)


def test_synthpharm_raises_by_name():
    from pointvs_amd.parquet_data import SynthPharmDataset
    with pytest.raises(NotImplementedError, match='synthpharm'):
        SynthPharmDataset(DATAROOT, types_fname=DATAROOT / 'chembl6.types')


def load_cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location('pvs_entry', ROOT / 'point_vs.py')
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_refuses_unbuilt_flags_on_a_parquet_root(tmp_path):
    cli = load_cli()
    assert cli.is_parquet_root(DATAROOT) and not cli.is_parquet_root(tmp_path)
    base = ['egnn', str(tmp_path), '--train_data_root_pose', str(DATAROOT), '--train_types_pose',
            str(DATAROOT / 'chembl6.types')]
    for extra, flag in ((['--prune'], 'prune'), (['--p_remove_entity', '0.5'], 'p_remove_entity'),
                        (['--synthpharm'], 'synthpharm'), (['--hydrogens'], 'hydrogens')):
        args = cli.parse_args(base + extra)
        with pytest.raises(NotImplementedError, match=flag):
            cli.make_loader(args, args.train_data_root_pose, args.train_types_pose, 'train', 'classification', 0, 1, 1)


def test_loader_samplers_follow_make_loader():
    from pointvs_amd.data_loaders import RankWeightedSampler
    from pointvs_amd.parquet_data import get_data_loader
    _, types, kwargs = load_setting('aug2')
    kwargs['augmented_actives'] = kwargs.pop('augmented_active_count')
    kwargs['min_aug_angle'] = kwargs.pop('augmented_active_min_angle')
    train = get_data_loader(DATAROOT, types_fname=DATAROOT / types, mode='train', batch_size=4, rot=False, rank=1,
                            world=2, seed=7, **kwargs)
    assert isinstance(train.sampler, RankWeightedSampler) and train.sampler.rank == 1 and train.sampler.world == 2
    assert np.array_equal(train.sampler.weights.numpy(), train.dataset.sample_weights.numpy())
    assert len(train.dataset) == 12 and len(train) == 2
    val = get_data_loader(DATAROOT, types_fname=DATAROOT / types, mode='val', batch_size=4, rot=False, rank=1, world=2,
                          **kwargs)
    assert val.sampler == list(range(6, 12)) and len(val) == 2


def test_host_draws_are_a_function_of_seed_epoch_and_index():
    from pointvs_amd.parquet_data import angle_3d, rotate_about_mean
    _, ds = make_dataset('aug2', rot=True, p_noise=0.5, seed=3)
    a = ds.host_draws([0, 7, 11], epoch=2)
    b = ds.host_draws([11, 0, 7], epoch=2)
    assert np.array_equal(a[2][0], b[2][1]) and np.array_equal(a[1][1], b[1][2]) and a[0][0] == b[0][1]
    c = ds.host_draws([0, 7, 11], epoch=3)
    assert not np.array_equal(a[2], c[2]) and not np.array_equal(a[1][1], c[1][1])
    for mats in (a[1], a[2]):
        for m in mats:
            assert np.abs(m @ m.T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(m) - 1.0) < 1e-12
    assert np.array_equal(a[1][0], np.eye(3))        # sample 0 is no augmented active
    for b_idx, item in ((1, 7), (2, 11)):
        xyz = ds.ligand_coordinates(item)
        turned = rotate_about_mean(xyz, a[1][b_idx])
        assert angle_3d(xyz[0], turned[0]) >= np.pi * 30 / 180
    flips = sum(ds.host_draws([i], epoch=e)[0][0] != ds.label(i) for i in range(6) for e in range(40))
    assert 80 < flips < 160          # p_noise = 0.5 over 240 draws


def test_reference_import_paths_resolve():
    from point_vs.preprocessing.data_loaders import (PygPointCloudDataset, SynthPharmDataset,  # noqa: F401
                                                     classifiaction_types_to_lists, get_data_loader,
                                                     regression_types_to_lists)
    from pointvs_amd import parquet_data
    assert PygPointCloudDataset is parquet_data.PygPointCloudDataset
    assert get_data_loader is parquet_data.get_data_loader
    labels, rmsds, recs, ligs = classifiaction_types_to_lists(DATAROOT / 'test.types')
    assert (labels, rmsds, recs, ligs) == ([1, 1], [-1.0, -1.0], ['rec_0.parquet'] * 2, ['lig_0.parquet'] * 2)


def test_complex_entries_are_declared_bound_and_exported():
    from pointvs_amd import _lib
    header = (ROOT / 'include' / 'pvs_egnn.h').read_text()
    declared = set(re.findall(r'\b(pvs_[a-z0-9_]+)\s*\(', header))
    new = {'pvs_complex_batch_workspace_bytes', 'pvs_complex_batch_count', 'pvs_complex_batch_fill',
           'pvs_complex_edges'}
    assert new <= declared
    assert len(declared) == len(_lib.EXPORTED_SYMBOLS) and declared == set(_lib.EXPORTED_SYMBOLS)
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    assert sum(hasattr(handle, name) for name in declared) == len(declared)
    assert _lib.MIN_VERSION >= 105 and _lib.lib().pvs_version() >= 105
    fields = [f for f, _ in _lib.PvsComplexPool._fields_]
    struct = re.search(r'typedef struct \{([^}]*)\} PvsComplexPool;', header).group(1)
    assert fields == re.findall(r'[*\s,](\w+)(?=[,;])', struct)
