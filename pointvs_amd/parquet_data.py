"""PointVS data roots (`receptors/*.parquet`, `ligands/**/*.parquet`, a types file) as training / scoring batches whose
complexes are built on the GPU.

The reference builds every sample on the host (/root/reference/point_vs/preprocessing/data_loaders.py:259-391: two
`pandas.read_parquet`, a `cdist` crop, a second `cdist` for the edges - milliseconds per graph) while the model step
here takes tens of microseconds per graph. So the files are read ONCE: every unique receptor and ligand file goes into a
device-resident pool (fp64 coordinates as stored, smina types, atomic numbers, one offset table each), and a batch is
made from `(receptor id, ligand id)` pairs by `pvs_complex_batch_count / _fill` (csrc/complex_build.hip: ligand
transform, crop, hydrogen filter, features, node tables), the existing `pvs_radius_graph_count / _fill` on the cropped,
unrotated coordinates and `pvs_complex_edges` (the loader's edge-list order). Two small device-to-host copies per batch
(node counts, edge counts); none per graph.

What is drawn at random is drawn on the host from `numpy.random.default_rng((seed, epoch, sample index))`: the rotation
of `rot=True`, the turn of an augmented active, the label flip of `p_noise`. The reference uses numpy's global state,
so its draws are not reproduced bit for bit; the constructions are (Arvo's rotation, the rejection loop on the angle).

`PygPointCloudDataset` takes the reference's constructor arguments; options this path does not build raise
NotImplementedError naming the flag instead of being ignored.
"""
import ctypes as C
from collections import defaultdict
from pathlib import Path

import numpy as np
import torch

from . import _lib
from .data_loaders import RankWeightedSampler, class_balance_weights
from .graph import Batch
from .nowait import LateQueue

MAX_LIGAND_ATOMS = 1024     # csrc/complex_build.hip keeps a sample's ligand in LDS; the screening paths accept the
                            # same number (screening.MAX_SCREEN_LIGAND_ATOMS)


def classification_types_to_lists(types_fname):
    """Types file -> (labels, rmsds, receptor paths, ligand paths), the reading of data_loaders.py:560-635: a line of two
    fields is `receptor ligand` (no label); otherwise the label is the first field where it is an integer, the first
    field that is no number is the receptor, the field before it its RMSD, the next such field the ligand; fields that
    start with '#' are skipped; lines without both paths are dropped."""
    labels, rmsds, recs, ligs = [], [], [], []
    for line in Path(types_fname).expanduser().read_text().splitlines():
        chunks = line.strip().split()
        if not chunks:
            continue
        label = rmsd = rec = lig = None
        if len(chunks) == 2:
            rec, lig = chunks
        else:
            try:
                label = int(chunks[0])
            except ValueError:
                label = None
            for idx, chunk in enumerate(chunks):
                if chunk.startswith('#'):
                    continue
                try:
                    float(chunk)
                except ValueError:
                    if rec is None:
                        rec, rmsd = chunk, float(chunks[idx - 1])
                    else:
                        lig = chunk
        if rec is not None and lig is not None:
            labels.append(label)
            rmsds.append(rmsd)
            recs.append(rec)
            ligs.append(lig)
    return labels, rmsds, recs, ligs


def regression_types_to_lists(data_root, types_fname):
    """Types file -> (pki, pkd, ic50, receptor paths, ligand paths), data_loaders.py:523-557: five columns
    `pki pkd ic50 receptor ligand`, or two (`receptor ligand`, targets None); rows whose files are missing are dropped."""
    rows = [ln.split() for ln in Path(types_fname).expanduser().read_text().splitlines() if ln.strip()]
    pki, pkd, ic50, recs, ligs = [], [], [], [], []
    for row in rows:
        rec, lig = row[-2], row[-1]
        if not (Path(data_root, rec).is_file() and Path(data_root, lig).is_file()):
            continue
        targets = [float(v) for v in row[:3]] if len(row) >= 5 else [None, None, None]
        for dst, val in zip((pki, pkd, ic50), targets):
            dst.append(val)
        recs.append(rec)
        ligs.append(lig)
    return pki, pkd, ic50, recs, ligs


def atomic_number_classes(polar_hydrogens):
    """(class of every recognised atomic number, n_features), data_loaders.py:194-216: C N O F P S Cl on their own, the
    groups (Br I), (Li Na K), (Be Mg Ca), (Fe Cu Zn) sharing one class each, H last when hydrogens are kept; every other
    element falls into the overflow class `n_features`."""
    classes = {num: idx for idx, num in enumerate((6, 7, 8, 9, 15, 16, 17))}
    for group in ((35, 53), (3, 11, 19), (4, 12, 20), (26, 29, 30)):
        nxt = max(classes.values()) + 1
        classes.update({elem: nxt for elem in group})
    if polar_hydrogens:
        classes[1] = max(classes.values()) + 1
    return classes, max(classes.values()) + 1


def arvo_matrix(rng):
    """M of uniform_random_rotation (preprocessing.py:20-50, "Fast Random Rotation Matrices", Arvo 1992): a rotation
    about z, then a Householder reflection through a random direction, negated: M = -(H @ R)."""
    x2 = 2 * np.pi * rng.random()
    x3 = rng.random()
    x1 = rng.random()
    R = np.eye(3)
    R[0, 0] = R[1, 1] = np.cos(2 * np.pi * x1)
    R[0, 1] = -np.sin(2 * np.pi * x1)
    R[1, 0] = np.sin(2 * np.pi * x1)
    v = np.array([np.cos(x2) * np.sqrt(x3), np.sin(x2) * np.sqrt(x3), np.sqrt(1 - x3)])
    H = np.eye(3) - (2 * np.outer(v, v))
    return -(H @ R)


def rotate_about_mean(x, M):
    """The reference's way of applying M (preprocessing.py:51-53): ((x - mean) @ M) + mean @ M. Equal to x @ M up to
    fp64 rounding; the device evaluates x @ M (apply_matrix)."""
    x = np.asarray(x, dtype=np.float64).reshape((-1, 3))
    mean = np.mean(x, axis=0)
    return ((x - mean) @ M) + mean @ M


def apply_matrix(x, M):
    """x @ M exactly as the device kernel rounds it: (x0 * M0j + x1 * M1j) + x2 * M2j, one rounding per operation."""
    x = np.asarray(x, dtype=np.float64).reshape((-1, 3))
    return (x[:, 0:1] * M[0:1, :] + x[:, 1:2] * M[1:2, :]) + x[:, 2:3] * M[2:3, :]


def angle_3d(v1, v2):
    """preprocessing.py:56-65."""
    denom = max(1e-7, np.linalg.norm(v1) * np.linalg.norm(v2))
    return np.arccos(np.clip(np.dot(v1, v2) / denom, -1.0, 1.0))


def augmentation_matrix(lig_xyz, min_angle_deg, rng):
    """The turn of an augmented active (preprocessing.py:277-288): rotations are drawn until the position vector of the
    ligand's first atom has turned by at least the minimum angle."""
    first = np.asarray(lig_xyz[0], dtype=np.float64)
    min_rad = np.pi * min_angle_deg / 180
    while True:
        M = arvo_matrix(rng)
        if angle_3d(first, rotate_about_mean(lig_xyz, M)[0]) >= min_rad:
            return M


class PygPointCloudDataset:
    """The reference's PygPointCloudDataset (data_loaders.py:33-391) over a resident pool: same constructor arguments,
    same lists (`ligand_fnames`, `receptor_fnames`, `labels`, `pre_aug_ds_len`, `sample_weights`, `feature_dim`); a batch
    is built by `build_batch(indices, epoch)` on the device instead of sample by sample in `__getitem__`
    (`ds[i]` returns the one-sample batch).

    `pre_aug_ds_len` is, as in the reference, the number of usable lines of the types file BEFORE the RMSD filter, so
    with RMSD labelling that drops lines the first augmented entries are not turned - kept as it is there."""

    def __init__(self, base_path, radius=12, polar_hydrogens=True, use_atomic_numbers=False, compact=True, rot=False,
                 augmented_active_count=0, augmented_active_min_angle=90, max_active_rms_distance=None,
                 min_inactive_rms_distance=None, max_inactive_rms_distance=None, fname_suffix='parquet',
                 model_task='classification', types_fname=None, edge_radius=None, estimate_bonds=False, prune=False,
                 bp=None, p_remove_entity=0, extended_atom_types=False, p_noise=-1, include_strain_info=False,
                 seed=0, device=None, **kwargs):
        if prune:
            raise NotImplementedError('--prune (prune=True) is not built on the data-root path: the batch builder keeps '
                                      'every cropped receptor atom')
        if p_remove_entity and p_remove_entity > 0:
            raise NotImplementedError('--p_remove_entity > 0 is not built on the data-root path')
        if include_strain_info:
            raise NotImplementedError('--include_strain_info is not built on the data-root path')
        if bp is not None:
            raise NotImplementedError('bp (ligand-only / receptor-only graphs) is not built on the data-root path')
        if not use_atomic_numbers and polar_hydrogens:
            raise NotImplementedError('--hydrogens (polar_hydrogens=True) with smina types: the reference raises too '
                                      '("Hydrogens temporarily disabled"); use --use_atomic_numbers')
        if types_fname is None:
            raise ValueError('a types file is required (the reference reads its sample list from it)')
        assert not ((max_active_rms_distance is None) != (min_inactive_rms_distance is None))
        self.base_path = Path(base_path).expanduser()
        if not self.base_path.exists():
            raise FileNotFoundError(f'Dataset {self.base_path} does not exist.')
        self.radius, self.edge_radius, self.estimate_bonds = radius, edge_radius, estimate_bonds
        self.polar_hydrogens, self.use_atomic_numbers, self.compact = polar_hydrogens, use_atomic_numbers, compact
        self.rot, self.model_task, self.p_noise, self.fname_suffix = bool(rot), model_task, p_noise, fname_suffix
        self.prune, self.bp, self.p_remove_entity, self.include_strain_info = False, None, 0, False
        self.augmented_active_min_angle = augmented_active_min_angle
        self.use_types = True
        self.seed, self.epoch = int(seed), 0
        self.device = device

        labels = []
        self.sampler, self.sample_weights = None, None
        if model_task.endswith('regression'):
            self.pki, self.pkd, self.ic50, self.receptor_fnames, self.ligand_fnames = regression_types_to_lists(
                self.base_path, types_fname)
            self.pre_aug_ds_len = len(self.ligand_fnames)
        else:
            label_by_rmsd = max_active_rms_distance is not None or max_inactive_rms_distance is not None
            if label_by_rmsd:
                max_active = np.inf if max_active_rms_distance is None else max_active_rms_distance
                max_inactive = np.inf if max_inactive_rms_distance is None else max_inactive_rms_distance
                min_inactive = 0 if min_inactive_rms_distance is None else min_inactive_rms_distance
            file_labels, rmsds, recs, ligs = classification_types_to_lists(types_fname)
            labels = [] if label_by_rmsd else list(file_labels)
            kept_recs, kept_ligs, aug_recs, aug_ligs = [], [], [], []
            for k, (rec, lig) in enumerate(zip(recs, ligs)):
                if label_by_rmsd:        # pose selection by RMSD from the crystal pose (:136-154)
                    rmsd = rmsds[k]
                    if rmsd < 0:
                        continue
                    if rmsd < max_active:
                        labels.append(1)
                        aug_recs += [rec] * augmented_active_count
                        aug_ligs += [lig] * augmented_active_count
                    elif rmsd >= max_inactive:
                        continue
                    elif rmsd >= min_inactive:
                        labels.append(0)
                    else:
                        continue
                elif labels[k]:
                    aug_recs += [rec] * augmented_active_count
                    aug_ligs += [lig] * augmented_active_count
                kept_recs.append(rec)
                kept_ligs.append(lig)
            self.pre_aug_ds_len = len(ligs)
            self.n_confirmed = len(kept_ligs)
            self.receptor_fnames = kept_recs + aug_recs     # augmented actives at the end, labelled 0 (:163-172)
            self.ligand_fnames = kept_ligs + aug_ligs
            labels = np.array(labels + [0] * len(aug_ligs))
            if len(labels) and labels[0] is not None:
                self.sample_weights = class_balance_weights(labels)
                self.sampler = self.sample_weights     # (not None exactly when the reference builds a sampler)
        self.labels = labels

        if use_atomic_numbers:
            classes, self.n_features = atomic_number_classes(polar_hydrogens)
            self.atomic_number_to_index = defaultdict(lambda: self.n_features)
            self.atomic_number_to_index.update(classes)
        else:
            self.n_features = 11 + 8 * bool(extended_atom_types)
        self.feature_dim = self.n_features + 1 if compact else self.n_features * 2
        self._read_pool()

    # ---- host pool -------------------------------------------------------------------------------------------------
    def _read_pool(self):
        """Every unique file once (pandas.read_parquet), concatenated per kind with an offset table."""
        import pandas as pd

        def gather(names):
            ids, order = {}, []
            for name in names:
                if name not in ids:
                    ids[name] = len(order)
                    order.append(name)
            xyz, types, z, ptr = [], [], [], [0]
            for name in order:
                path = self.base_path / name
                if not path.is_file():
                    raise FileNotFoundError(f'{path} does not exist')
                df = pd.read_parquet(path)
                xyz.append(np.stack([df['x'].to_numpy(), df['y'].to_numpy(), df['z'].to_numpy()], axis=1).astype(np.float64))
                types.append(df['types'].to_numpy().astype(np.int32))
                z.append(df['atomic_number'].to_numpy().astype(np.int32))
                ptr.append(ptr[-1] + len(df))
            cat = (lambda parts, shape, dt: np.concatenate(parts) if parts else np.zeros(shape, dt))
            return (np.array([ids[n] for n in names], dtype=np.int32), order,
                    dict(xyz=cat(xyz, (0, 3), np.float64), types=cat(types, (0,), np.int32), z=cat(z, (0,), np.int32),
                         ptr=np.array(ptr, dtype=np.int32)))

        self.rec_ids, self.rec_files, self.rec_pool = gather([str(f) for f in self.receptor_fnames])
        self.lig_ids, self.lig_files, self.lig_pool = gather([str(f) for f in self.ligand_fnames])
        sizes = np.diff(self.lig_pool['ptr'])
        if len(sizes) and sizes.max() > MAX_LIGAND_ATOMS:
            raise ValueError(f'{self.lig_files[int(sizes.argmax())]} has {int(sizes.max())} atoms; the batch builder '
                             f'takes ligands of up to {MAX_LIGAND_ATOMS}')
        self._dev_pool = None

    def _pool_on(self, device):
        """The pool in device memory (uploaded at first use) and its C struct."""
        if self._dev_pool is not None and self._dev_pool[0] == device:
            return self._dev_pool[1], self._dev_pool[2]
        t = {}
        for kind, pool in (('rec', self.rec_pool), ('lig', self.lig_pool)):
            for key, arr in pool.items():
                t[f'{kind}_{key}'] = torch.from_numpy(np.ascontiguousarray(arr)).to(device)
        lut = np.full(128, self.n_features, dtype=np.int32)
        if self.use_atomic_numbers:
            for num, idx in self.atomic_number_to_index.items():
                lut[num] = idx
        t['class_of_z'] = torch.from_numpy(lut).to(device)
        c = _lib.PvsComplexPool()
        for field, key in (('rec_xyz', 'rec_xyz'), ('lig_xyz', 'lig_xyz'), ('rec_types', 'rec_types'),
                           ('lig_types', 'lig_types'), ('rec_z', 'rec_z'), ('lig_z', 'lig_z'), ('rec_ptr', 'rec_ptr'),
                           ('lig_ptr', 'lig_ptr')):
            setattr(c, field, _lib.ptr(t[key]))
        c.n_rec, c.n_lig = len(self.rec_files), len(self.lig_files)
        self._dev_pool = (device, t, c)
        return t, c

    # ---- the reference's surface -----------------------------------------------------------------------------------
    def __len__(self):
        return len(self.ligand_fnames)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def label(self, item):
        """Clean label of a sample (classification: 0 / 1; regression: the largest of pki, pkd, ic50, :235-242)."""
        if self.model_task == 'classification':
            return 0 if self.labels[item] is None else int(self.labels[item])      # (a types file without labels)
        targets = tuple(np.nan if v is None else v for v in (self.pki[item], self.pkd[item], self.ic50[item]))
        return targets if self.model_task == 'multi_regression' else max(targets)

    def is_augmented(self, item):
        return (not self.model_task.endswith('regression') and item >= self.pre_aug_ds_len
                and bool(self.augmented_active_min_angle))

    def _rng(self, item, epoch, stream):
        return np.random.default_rng((self.seed, int(epoch), int(item), stream))

    def ligand_coordinates(self, item):
        lo, hi = self.lig_pool['ptr'][self.lig_ids[item]:self.lig_ids[item] + 2]
        return self.lig_pool['xyz'][lo:hi]

    def receptor_coordinates(self, item):
        lo, hi = self.rec_pool['ptr'][self.rec_ids[item]:self.rec_ids[item] + 2]
        return self.rec_pool['xyz'][lo:hi]

    def host_draws(self, indices, epoch=None):
        """(labels, ligand transforms [B,3,3] or None, rotations [B,3,3] or None) of a batch: everything random about it,
        a function of (seed, epoch, sample index) alone."""
        epoch = self.epoch if epoch is None else epoch
        labels, lig_xform, rots = [], None, None
        for b, item in enumerate(indices):
            label = self.label(item)
            if self.model_task == 'classification' and self._rng(item, epoch, 2).random() < self.p_noise:
                label = 1 - label
            labels.append(label)
            if self.is_augmented(item):
                if lig_xform is None:
                    lig_xform = np.tile(np.eye(3), (len(indices), 1, 1))
                lig_xform[b] = augmentation_matrix(self.ligand_coordinates(item), self.augmented_active_min_angle,
                                                   self._rng(item, epoch, 0))
        if self.rot:
            rots = np.stack([arvo_matrix(self._rng(item, epoch, 1)) for item in indices])
        return labels, lig_xform, rots

    # ---- device ----------------------------------------------------------------------------------------------------
    def build_batch(self, indices, epoch=None, device=None):
        """Samples `indices` -> one `pointvs_amd.graph.Batch` on the device (x, pos, edge_index, edge_attr, batch, y,
        lig_fname, rec_fname, ptr, edge_layout = 'generate_edges')."""
        from .global_objects import DEVICE
        device = torch.device(device or self.device or DEVICE)
        if device.type != 'cuda':
            raise RuntimeError('complex batches are built by HIP kernels on a GPU; there is no CPU path')
        indices = [int(i) for i in indices]
        lib = _lib.lib()
        pool_t, pool_c = self._pool_on(device)
        stream = _lib.stream(device)
        n_b = len(indices)
        labels, lig_xform, rots = self.host_draws(indices, epoch)

        rec_id, lig_id = self.rec_ids[indices], self.lig_ids[indices]
        n_in = (np.diff(self.rec_pool['ptr'])[rec_id] + np.diff(self.lig_pool['ptr'])[lig_id]).astype(np.int64)
        flag_off = np.concatenate([[0], np.cumsum(n_in)])
        n_atoms_in = int(flag_off[-1])
        pairs = torch.from_numpy(np.stack([rec_id, lig_id, flag_off[:-1].astype(np.int32)], axis=1).astype(np.int32)
                                 ).contiguous().to(device)
        mats = [m for m in (lig_xform, rots) if m is not None]
        mats_dev = torch.from_numpy(np.ascontiguousarray(np.stack(mats))).to(device) if mats else None
        xform_dev = mats_dev[0] if lig_xform is not None else None
        rot_dev = mats_dev[-1] if rots is not None else None

        i32 = dict(dtype=torch.int32, device=device)
        counts_status = torch.empty(2 * n_b + 1, **i32)        # counts [B,2], then the status word: one copy back
        counts_ptr = counts_status.data_ptr()
        status_ptr = counts_ptr + 8 * n_b
        ws_bytes = lib.pvs_complex_batch_workspace_bytes(n_b, n_atoms_in)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
        keep_h = 1 if self.polar_hydrogens else 0
        _lib.check(lib.pvs_complex_batch_count(
            C.byref(pool_c), _lib.ptr(pairs), _lib.ptr(xform_dev), n_b, n_atoms_in, float(self.radius), keep_h,
            counts_ptr, status_ptr, _lib.ptr(ws), ws_bytes, stream), 'pvs_complex_batch_count')
        host = counts_status.cpu().numpy()       # host copy 1 of 2: the batch's node counts
        _check_late_status()
        _raise_for_status(int(host[-1]))
        node_counts = host[:-1].reshape(n_b, 2).sum(axis=1)
        if (node_counts == 0).any():
            raise ValueError(f'sample {indices[int(np.argmin(node_counts))]} has no atom left after the hydrogen filter')
        graph_ptr_host = np.concatenate([[0], np.cumsum(node_counts)]).astype(np.int32)
        n = int(graph_ptr_host[-1])
        graph_ptr = torch.from_numpy(graph_ptr_host).to(device)

        x = torch.empty((n, self.feature_dim), dtype=torch.float32, device=device)
        pos = torch.empty((n, 3), dtype=torch.float32, device=device)
        pos_graph = torch.empty((n, 3), dtype=torch.float32, device=device) if rot_dev is not None else None
        bp = torch.empty(n, dtype=torch.uint8, device=device)
        batch_vec = torch.empty(n, dtype=torch.int64, device=device)
        _lib.check(lib.pvs_complex_batch_fill(
            C.byref(pool_c), _lib.ptr(pairs), _lib.ptr(xform_dev), _lib.ptr(rot_dev), n_b, n_atoms_in, n,
            1 if self.use_atomic_numbers else 0, self.n_features, 1 if self.compact else 0,
            _lib.ptr(pool_t['class_of_z']), counts_ptr, _lib.ptr(graph_ptr), _lib.ptr(x), _lib.ptr(pos),
            _lib.ptr(pos_graph), _lib.ptr(bp), _lib.ptr(batch_vec), status_ptr, _lib.ptr(ws), ws_bytes, stream),
            'pvs_complex_batch_fill')

        # the edge list, from the unrotated coordinates (data_loaders.py:359-370; edge_radius 0 means 4)
        edge_radius = self.edge_radius if self.edge_radius and self.edge_radius > 0 else 4
        if self.edge_radius is not None and self.edge_radius < 0:
            raise NotImplementedError('edge_radius < 0 (no edge list) is not built on the data-root path')
        intra_radius = 2.0 if self.estimate_bonds else edge_radius
        coords = pos if pos_graph is None else pos_graph
        max_nodes = int(node_counts.max())
        rowptr, inter_ptr, intra_ptr = (torch.empty(n + 1, **i32) for _ in range(3))
        st_bytes = lib.pvs_radius_graph_state_bytes(n, n_b, max_nodes)
        state = torch.empty(st_bytes, dtype=torch.uint8, device=device)
        _lib.check(lib.pvs_radius_graph_count(
            _lib.ptr(coords), _lib.ptr(bp), _lib.ptr(graph_ptr), n_b, n, max_nodes, float(edge_radius),
            float(intra_radius), 0, _lib.ptr(rowptr), _lib.ptr(inter_ptr), _lib.ptr(intra_ptr), _lib.ptr(state), st_bytes,
            stream), 'pvs_radius_graph_count')
        # host copy 2 of 2: where every graph's edges start (rowptr at the node offsets; the last entry is E), with the
        # status word of the fill
        host = torch.cat([rowptr.index_select(0, graph_ptr.long()), counts_status[-1:]]).cpu().numpy()
        _raise_for_status(int(host[-1]))
        edge_ptr_host = host[:-1]
        n_edges = int(edge_ptr_host[-1])
        e_alloc = max(n_edges, 1)
        row, col, perm = (torch.empty(e_alloc, **i32) for _ in range(3))
        etype = torch.empty(e_alloc, dtype=torch.uint8, device=device)
        inv_deg = torch.empty(n, dtype=torch.float32, device=device)
        ws2_bytes = lib.pvs_radius_graph_workspace_bytes(n, n_b, n_edges)
        ws2 = torch.empty(ws2_bytes, dtype=torch.uint8, device=device)
        _lib.check(lib.pvs_radius_graph_fill(
            _lib.ptr(bp), _lib.ptr(graph_ptr), n_b, n, max_nodes, n_edges, _lib.ptr(rowptr), _lib.ptr(inter_ptr),
            _lib.ptr(intra_ptr), _lib.ptr(row), _lib.ptr(col), _lib.ptr(etype), _lib.ptr(perm), None, None,
            _lib.ptr(inv_deg), _lib.ptr(state), st_bytes, _lib.ptr(ws2), ws2_bytes, stream), 'pvs_radius_graph_fill')
        edge_index = torch.empty((2, n_edges), dtype=torch.int64, device=device)
        edge_attr = torch.empty((n_edges, 3), dtype=torch.int64, device=device)
        _lib.check(lib.pvs_complex_edges(
            n, n_edges, n_b, _lib.ptr(graph_ptr), _lib.ptr(rowptr), _lib.ptr(inter_ptr), _lib.ptr(intra_ptr),
            _lib.ptr(row), _lib.ptr(col), _lib.ptr(etype), _lib.ptr(perm), _lib.ptr(edge_index), _lib.ptr(edge_attr),
            status_ptr, stream), 'pvs_complex_edges')
        _LATE.put(counts_status[-1:], keep=counts_status)

        y = torch.tensor(np.asarray(labels, dtype=np.float64).reshape(-1))
        y = (y.long() if self.model_task == 'classification' else y.float()).to(device)
        return Batch(
            x=x, pos=pos, edge_index=edge_index, edge_attr=edge_attr, batch=batch_vec, y=y,
            lig_fname=[Path(self.ligand_fnames[i]) for i in indices],
            rec_fname=[Path(self.receptor_fnames[i]) for i in indices],
            edge_layout='generate_edges', ptr=torch.from_numpy(graph_ptr_host.astype(np.int64)), num_graphs=n_b,
            graph_node_counts=[int(v) for v in node_counts], graph_edge_counts=[int(v) for v in np.diff(edge_ptr_host)],
            bp=bp)

    def __getitem__(self, item):
        return self.build_batch([item])


_STATUS_TEXT = (
    (1, 'a (receptor, ligand) pair outside the pool'),
    (2, f'a ligand of more than {MAX_LIGAND_ATOMS} atoms'),
    (4, 'an atom type outside the feature encoding (the reference\'s one_hot raises on it: a negative type, or under '
        'the non-compact encoding a class of 2 * n_features or more, e.g. a receptor element outside the atomic-number '
        'table)'),
    (8, 'node offsets that do not match the counted atoms'),
    (16, 'radius-graph tables that do not describe the batch'),
)


def _raise_for_status(code):
    if code:
        raise ValueError('complex batch: ' + '; '.join(text for bit, text in _STATUS_TEXT if code & bit))


_LATE = LateQueue()      # status words of pvs_complex_edges, copied back without waiting and read at the next batch


def _check_late_status(wait=False):
    """Raises for the words that have landed; wait=True: for every word still in flight, oldest first."""
    while wait and len(_LATE):
        _raise_for_status(_LATE.take()[0])
    for code, _ in _LATE.landed():
        _raise_for_status(code)


class ComplexLoader:
    """Iterable over device-built batches: `batch_size` samples in sampler (or index) order, drop_last=False like the
    reference's loader (data_loaders.py:517-520). `.dataset` and `.sampler` as the training loop expects them."""

    def __init__(self, dataset, batch_size=32, sampler=None, device=None):
        self.dataset, self.batch_size, self.sampler, self.device = dataset, int(batch_size), sampler, device

    def __len__(self):
        n = len(self.sampler) if self.sampler is not None else len(self.dataset)
        return -(-n // self.batch_size)

    def __iter__(self):
        order = list(self.sampler) if self.sampler is not None else list(range(len(self.dataset)))
        epoch = getattr(self.sampler, 'epoch', self.dataset.epoch)
        for k in range(0, len(order), self.batch_size):
            yield self.dataset.build_batch(order[k:k + self.batch_size], epoch=epoch, device=self.device)
        _check_late_status(wait=True)


class SynthPharmDataset:
    def __init__(self, *args, **kwargs):
        raise NotImplementedError('--synthpharm (SynthPharmDataset) is not built on the data-root path')


def get_data_loader(data_root, dataset_class=PygPointCloudDataset, receptors=None, batch_size=32, compact=True,
                    use_atomic_numbers=False, radius=6, rot=True, augmented_actives=0, min_aug_angle=30,
                    polar_hydrogens=True, mode='train', model_task='classification', max_active_rms_distance=None,
                    fname_suffix='parquet', min_inactive_rms_distance=None, types_fname=None, edge_radius=None,
                    prune=False, estimate_bonds=False, bp=None, p_noise=-1, rank=0, world=1, seed=0, device=None,
                    **kwargs):
    """The reference's get_data_loader (data_loaders.py:481-520). Train mode draws with the class-balancing
    RankWeightedSampler (index order where the reference builds no sampler); val mode iterates the rank's contiguous
    share in order."""
    from .distributed import shard_range
    ds = dataset_class(
        data_root, compact=compact, receptors=receptors, augmented_active_count=augmented_actives,
        augmented_active_min_angle=min_aug_angle, polar_hydrogens=polar_hydrogens,
        max_active_rms_distance=max_active_rms_distance, min_inactive_rms_distance=min_inactive_rms_distance,
        use_atomic_numbers=use_atomic_numbers, fname_suffix=fname_suffix, types_fname=types_fname,
        edge_radius=edge_radius, estimate_bonds=estimate_bonds, prune=prune, bp=bp, radius=radius, rot=rot,
        model_task=model_task, p_noise=p_noise, seed=seed, device=device, **kwargs)
    if mode == 'train':
        weights = ds.sample_weights if ds.model_task == 'classification' else None
        sampler = RankWeightedSampler(weights, len(ds), rank, world, seed=seed)
    else:
        lo, hi = shard_range(len(ds), rank, world)
        sampler = list(range(lo, hi))
    return ComplexLoader(ds, batch_size, sampler=sampler, device=device)
