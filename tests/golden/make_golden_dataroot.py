"""Golden vectors for the parquet data-root loader: runs the REFERENCE PygPointCloudDataset
(/root/reference/point_vs/preprocessing/data_loaders.py) over tests/golden/dataroot for a handful of settings and
stores, per setting, what its constructor derives (lists, labels, weights, sizes) and what its __getitem__ returns for
every sample that is not an augmented active (those are random in the reference). One `dataroot_<setting>.npz` each.
Usage (build container only, where /root/reference exists): python tests/golden/make_golden_dataroot.py

The data root holds the reference's own data files: test/resources/{rec,lig,rec_0,lig_0}.parquet with test.types, and
six complexes of data/small_chembl_test (one active and one decoy for each of three receptors: the set has one active
per receptor) with their types lines in chembl6.types. rmsd6.types and regression6.types are hand-made listings of the
same six complexes (the set's own RMSD column is -1 throughout and it has no affinity labels); regression6.types
also names one file that does not exist."""
import json
import sys
from pathlib import Path

import numpy as np

OUT = Path(__file__).resolve().parent
ROOT = OUT / 'dataroot'
sys.path.insert(0, str(OUT / '_refstubs'))   # import-only stand-ins for pymol/rdkit/... (see README there)
sys.path.insert(0, '/root/reference')
if not hasattr(np, 'product'):
    np.product = np.prod
from point_vs.preprocessing.data_loaders import PygPointCloudDataset   # noqa: E402

ATOMIC_H = dict(use_atomic_numbers=True, polar_hydrogens=True, compact=True)
SETTINGS = {   # name -> (types file, constructor kwargs)
    'ref_test': ('test.types', dict(radius=4, edge_radius=4, estimate_bonds=True, **ATOMIC_H)),
    'ref_test_smina': ('test.types', dict(radius=4, edge_radius=4, estimate_bonds=True, use_atomic_numbers=False,
                                          polar_hydrogens=False, compact=True)),   # the reference's own test fixture
    'cli_default': ('chembl6.types', dict(radius=10, edge_radius=4, estimate_bonds=False, use_atomic_numbers=False,
                                          polar_hydrogens=False, compact=False)),
    'r6_smina': ('chembl6.types', dict(radius=6, edge_radius=4, estimate_bonds=False, use_atomic_numbers=False,
                                       polar_hydrogens=False, compact=True)),
    'noncompact': ('chembl6.types', dict(radius=6, edge_radius=4, estimate_bonds=True, use_atomic_numbers=True,
                                         polar_hydrogens=True, compact=False)),
    'atomic_noh': ('chembl6.types', dict(radius=6, edge_radius=3, estimate_bonds=False, use_atomic_numbers=True,
                                         polar_hydrogens=False, compact=True)),
    'rmsd': ('rmsd6.types', dict(radius=6, edge_radius=4, estimate_bonds=False, max_active_rms_distance=2,
                                 min_inactive_rms_distance=2, augmented_active_count=1, **ATOMIC_H)),
    'aug2': ('chembl6.types', dict(radius=6, edge_radius=4, estimate_bonds=False, augmented_active_count=2,
                                   augmented_active_min_angle=30, **ATOMIC_H)),
    'regression': ('regression6.types', dict(radius=6, edge_radius=4, estimate_bonds=False, model_task='regression',
                                             **ATOMIC_H)),
}

for name, (types, kwargs) in SETTINGS.items():
    ds = PygPointCloudDataset(ROOT, types_fname=ROOT / types, rot=False, **kwargs)
    n_plain = len(ds) if ds.model_task.endswith('regression') else len(ds.dEs)    # (dEs: one per confirmed entry)
    xs, ps, eis, ets, ys, node_ptr, edge_ptr = [], [], [], [], [], [0], [0]
    for i in range(n_plain):
        d = ds[i]
        assert str(d.lig_fname) == str(ds.ligand_fnames[i]) and str(d.rec_fname) == str(ds.receptor_fnames[i])
        xs.append(d.x.numpy().astype(np.uint8))
        assert (xs[-1] == d.x.numpy()).all()
        ps.append(d.pos.numpy())
        assert ps[-1].dtype == np.float32
        eis.append(d.edge_index.numpy().astype(np.int32))
        et = d.edge_attr.numpy().argmax(1).astype(np.int8)
        assert (np.eye(3, dtype=np.int64)[et] == d.edge_attr.numpy()).all()
        ets.append(et)
        ys.append(np.asarray(d.y.numpy()))
        node_ptr.append(node_ptr[-1] + len(xs[-1]))
        edge_ptr.append(edge_ptr[-1] + len(et))
    rec = dict(
        settings=json.dumps(dict(types=types, kwargs=kwargs)), x=np.concatenate(xs), pos=np.concatenate(ps),
        edge_index=np.concatenate(eis, axis=1), edge_type=np.concatenate(ets), y=np.stack(ys),
        node_ptr=np.array(node_ptr), edge_ptr=np.array(edge_ptr), order=np.arange(n_plain),
        ligand_fnames=np.array([str(f) for f in ds.ligand_fnames]),
        receptor_fnames=np.array([str(f) for f in ds.receptor_fnames]),
        feature_dim=ds.feature_dim, n_features=ds.n_features, length=len(ds))
    if ds.model_task.endswith('regression'):
        rec.update(pki=np.array(ds.pki, dtype=np.float64), pkd=np.array(ds.pkd, dtype=np.float64),
                   ic50=np.array(ds.ic50, dtype=np.float64))
    else:
        rec.update(labels=np.asarray(ds.labels).astype(np.int64), pre_aug_ds_len=ds.pre_aug_ds_len,
                   sample_weights=(ds.sample_weights.numpy() if getattr(ds, 'sampler', None) is not None
                                   else np.zeros(0)))
    np.savez_compressed(OUT / f'dataroot_{name}.npz', **rec)
    print(name, 'len', len(ds), 'recorded', n_plain, 'nodes', np.diff(node_ptr).tolist(), 'edges',
          np.diff(edge_ptr).tolist(), 'feature_dim', ds.feature_dim)
