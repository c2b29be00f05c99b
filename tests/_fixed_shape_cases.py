"""Shared pieces of the fixed-shape batch tests (test_gpu_fixed_shape_batches.py, test_gpu_fixed_shape_scoring.py):
hand-made data roots whose kept node counts sit on the row-block / column-chunk edges of the radius-graph kernels, a
harness that runs the two capacity builders into canary-filled buffers, and the eager reference (`build_batch`, then
`prepare_graph` on its edge list), built once per (dataset, indices) and never modified."""
import ctypes as C

import numpy as np
import torch

from tests.test_gpu_parquet_dataset import hand_made_complexes, write_root      # noqa: F401  (same files, same writer)

DEV = 'cuda:0'
INT_CANARY, BYTE_CANARY = -77, 0x4D
GUARD = 64                                         # canary entries behind edge_cap
LATTICE_NODE_COUNTS = (1, 2, 63, 64, 65, 128, 129, 200)
C_ATOM, N_ATOM, O_ATOM, H_ATOM = (6, 1), (7, 5), (8, 7), (1, 11)      # (atomic number, a smina type)


def lattice_complex(n_nodes, crop_radius=3.0):
    """A one-atom ligand at the origin and n_nodes - 1 receptor atoms on a 0.5 A lattice, all closer than 2.9 A (inside
    the crop radius of 3), nearest first; one far atom closes the file, so that a receptor is never empty. Every kept
    node count is therefore exactly n_nodes."""
    assert crop_radius >= 3.0
    grid = np.arange(-6, 7) * 0.5
    pts = np.array([(x, y, z) for x in grid for y in grid for z in grid if (x, y, z) != (0.0, 0.0, 0.0)])
    dist = np.sqrt((pts ** 2).sum(axis=1))
    pts = pts[np.argsort(dist, kind='stable')]
    pts = pts[np.sort(dist, kind='stable') < 2.9][:n_nodes - 1]
    assert len(pts) == n_nodes - 1
    kinds = (C_ATOM, N_ATOM, O_ATOM)
    rec = [tuple(p) + kinds[k % 3] for k, p in enumerate(pts.tolist())] + [(40.0, 40.0, 40.0) + C_ATOM]
    return [(0.0, 0.0, 0.0) + C_ATOM], rec


def lattice_root(tmp_path):
    """(dataset, {kept node count: sample index}): the lattice complexes, then the existing hand-made cases (an empty
    crop, hydrogens dropped on one side, a receptor of 300 with two survivors, ...) behind them."""
    from pointvs_amd.parquet_data import PygPointCloudDataset
    complexes = [lattice_complex(n) for n in LATTICE_NODE_COUNTS] + hand_made_complexes(3.0)
    root, types = write_root(tmp_path, complexes)
    ds = PygPointCloudDataset(root, radius=3.0, edge_radius=4, estimate_bonds=False, types_fname=types,
                              use_atomic_numbers=True, polar_hydrogens=False, compact=True)
    return ds, {n: k for k, n in enumerate(LATTICE_NODE_COUNTS)}, len(LATTICE_NODE_COUNTS)


_EAGER = {}


def eager_reference(ds, indices):
    """The existing path on `indices`: build_batch, then the PreparedGraph of its edge list. Host copies, made once."""
    from pointvs_amd.graph import prepare_graph, runs_layout
    key = (id(ds), tuple(indices))
    if key not in _EAGER:
        b = ds.build_batch(list(indices), device=DEV)
        n = int(b.x.shape[0])
        pg = prepare_graph(b.edge_index, b.edge_attr, n, need_backward=False, layout=runs_layout(b, DEV))
        pg.check_status()
        e = pg.n_edges
        ref = dict(x=b.x, pos=b.pos, bp=b.bp, batch=b.batch, ptr=b.ptr, rowptr=pg.t['rowptr'], row=pg.t['row'][:e],
                   col=pg.t['col'][:e], etype=pg.t['etype'][:e], inv_deg=pg.t['inv_deg'])
        ref = {k: v.cpu().numpy().copy() for k, v in ref.items()}
        ref.update(n=n, e=e, max_graph=max(b.graph_node_counts), batch_obj=b, _keep=ds)
        _EAGER[key] = ref
    return _EAGER[key]


def exact_capacities(ds, indices):
    from pointvs_amd.captured_scoring import Capacities, batch_input_atoms
    ref = eager_reference(ds, indices)
    return Capacities(ref['n'], ref['max_graph'], max(ref['e'], 1), batch_input_atoms(ds, [indices]))


def generous_capacities(ds, indices):
    from pointvs_amd.captured_scoring import Capacities
    cap = exact_capacities(ds, indices)
    return Capacities(cap.node_cap + 131, cap.graph_node_cap + 70, cap.edge_cap + 1000, cap.atoms_in_cap + 17)


def canary_buffers(ds, n_samples, cap):
    """Every output of the two builders, pre-filled: ints -77, bytes 0x4D, floats NaN."""
    from pointvs_amd import _lib
    lib = _lib.lib()
    i32 = (lambda *shape: torch.full(shape, INT_CANARY, dtype=torch.int32, device=DEV))
    u8 = (lambda *shape: torch.full(shape, BYTE_CANARY, dtype=torch.uint8, device=DEV))
    f32 = (lambda *shape: torch.full(shape, float('nan'), dtype=torch.float32, device=DEV))
    room = cap.edge_cap + GUARD
    return dict(
        counts=i32(n_samples, 2), node_ptr=i32(n_samples + 1), x=f32(cap.node_cap, ds.feature_dim),
        pos=f32(cap.node_cap, 3), bp=u8(cap.node_cap), node_graph=i32(cap.node_cap), rowptr=i32(cap.node_cap + 1),
        row=i32(room), col=i32(room), etype=u8(room), inv_deg=f32(cap.node_cap), n_edges_fwd=i32(1), status=i32(1),
        workspace=u8(lib.pvs_complex_batch_workspace_bytes(n_samples, cap.atoms_in_cap)),
        state=u8(lib.pvs_radius_graph_state_bytes(cap.node_cap, n_samples, cap.graph_node_cap)))


OUTPUTS = ('counts', 'node_ptr', 'x', 'pos', 'bp', 'node_graph', 'rowptr', 'row', 'col', 'etype', 'inv_deg',
           'n_edges_fwd', 'status')


def build_cap(ds, indices, cap, buffers=None):
    """The two capacity builders on `indices` into `buffers` (default: fresh canary buffers). Returns host copies of
    every output, and the device buffers under 'device'."""
    from pointvs_amd import _lib
    lib = _lib.lib()
    indices = [int(i) for i in indices]
    n_b = len(indices)
    t = buffers if buffers is not None else canary_buffers(ds, n_b, cap)
    pool_t, pool_c = ds._pool_on(torch.device(DEV))
    rec_id, lig_id = ds.rec_ids[indices], ds.lig_ids[indices]
    n_in = np.diff(ds.rec_pool['ptr'])[rec_id] + np.diff(ds.lig_pool['ptr'])[lig_id]
    flag_off = np.concatenate([[0], np.cumsum(n_in)])
    assert flag_off[-1] <= cap.atoms_in_cap
    pairs = torch.from_numpy(np.stack([rec_id, lig_id, flag_off[:-1]], axis=1).astype(np.int32)).contiguous().to(DEV)
    stream = _lib.stream(torch.device(DEV))
    edge_radius = ds.edge_radius if ds.edge_radius and ds.edge_radius > 0 else 4
    intra = 2.0 if ds.estimate_bonds else edge_radius
    _lib.check(lib.pvs_complex_batch_build_cap(
        C.byref(pool_c), _lib.ptr(pairs), None, None, n_b, cap.atoms_in_cap, cap.node_cap, float(ds.radius),
        1 if ds.polar_hydrogens else 0, 1 if ds.use_atomic_numbers else 0, ds.n_features, 1 if ds.compact else 0,
        _lib.ptr(pool_t['class_of_z']), _lib.ptr(t['counts']), _lib.ptr(t['node_ptr']), _lib.ptr(t['x']),
        _lib.ptr(t['pos']), None, _lib.ptr(t['bp']), _lib.ptr(t['node_graph']), _lib.ptr(t['status']),
        _lib.ptr(t['workspace']), t['workspace'].numel(), stream), 'pvs_complex_batch_build_cap')
    _lib.check(lib.pvs_radius_graph_build_cap(
        _lib.ptr(t['pos']), _lib.ptr(t['bp']), _lib.ptr(t['node_ptr']), n_b, cap.node_cap, cap.graph_node_cap,
        float(edge_radius), float(intra), 0, cap.edge_cap, _lib.ptr(t['rowptr']), _lib.ptr(t['row']), _lib.ptr(t['col']),
        _lib.ptr(t['etype']), _lib.ptr(t['inv_deg']), _lib.ptr(t['n_edges_fwd']), _lib.ptr(t['status']), 0,
        _lib.ptr(t['state']), t['state'].numel(), stream), 'pvs_radius_graph_build_cap')
    torch.cuda.synchronize()
    out = {k: t[k].cpu().numpy().copy() for k in OUTPUTS}
    out['device'] = t
    return out


def same_bytes(a, b):
    """Bit equality of two arrays (NaN canaries included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_equals_eager(out, ref, cap):
    """Every array of a capacity build against the eager reference, no tolerance; padding rows; canaries behind E."""
    n, e = ref['n'], ref['e']
    assert int(out['status'][0]) == 0, int(out['status'][0])
    assert np.array_equal(out['node_ptr'], ref['ptr'].astype(np.int32))
    for key in ('x', 'pos', 'bp'):
        assert same_bytes(out[key][:n], ref[key]), key
    assert np.array_equal(out['node_graph'][:n].astype(np.int64), ref['batch'])
    assert np.array_equal(out['rowptr'][:n + 1], ref['rowptr'])
    for key in ('row', 'col', 'etype'):
        assert np.array_equal(out[key][:e], ref[key]), key
    assert same_bytes(out['inv_deg'][:n], ref['inv_deg'])
    assert (out['rowptr'][n:] == e).all() and len(out['rowptr']) == cap.node_cap + 1
    assert int(out['n_edges_fwd'][0]) == e                          # every entry written: the forward may use them all
    assert_padding(out, n)
    assert_edge_canaries(out, e)


def assert_padding(out, n):
    assert not out['x'][n:].any() and not out['pos'][n:].any() and not out['bp'][n:].any()
    assert (out['node_graph'][n:] == -1).all() and (out['inv_deg'][n:] == 1.0).all()


def assert_edge_canaries(out, e):
    assert (out['row'][e:] == INT_CANARY).all() and (out['col'][e:] == INT_CANARY).all()
    assert (out['etype'][e:] == BYTE_CANARY).all()
