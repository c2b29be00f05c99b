"""Test helper: the yardsticks of the maps on a cropped pose batch. (1) Numpy restatements of the two cropped reductions
(pvs_contact_attention_cropped, pvs_slot_node_values_cropped) as plain loops over the layout that PVS_SLOTS_CROPPED
writes - slot p owns the rows node_ptr[p] .. node_ptr[p + 1], its ligand atoms first, then the receptor atoms whose bit is
set in keep[p, :], in receptor order - with the slot verdict of csrc/contact_attention.h (pvs_cropped_slot) restated.
(2) The oracle maps of a set of hits on their cropped complexes: tests/_contact_ref.oracle_hotspots and
tests/_cam_ref.oracle_cam on each hit's cropped complex (tests/_crop_ref.cropped_complex), the receptor values scattered
back to [n_rec] with NaN for the atoms the hit does not keep."""
import numpy as np

from tests._cam_ref import node_value, single_thread
from tests._contact_ref import row_max
from tests._crop_ref import cropped_complex, words_mask

MAX_SLOT_LIGAND = 1024


def _words(keep_row):
    return np.asarray(keep_row).astype(np.uint64).reshape(-1)


def slot_ok(node_ptr, lig_ptr, keep_row, p, n_rec, n_nodes):
    """The slots the cropped operators accept: 0 <= a0 <= a1, at most 1024 ligand atoms, rows inside [0, n_nodes], as
    many rows as ligand atoms + set mask bits, no mask bit at or beyond n_rec."""
    a0, a1, r0, r1 = int(lig_ptr[p]), int(lig_ptr[p + 1]), int(node_ptr[p]), int(node_ptr[p + 1])
    words = _words(keep_row)
    bits = (((words[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)) != 0).reshape(-1)
    return (0 <= a0 <= a1 and a1 - a0 <= MAX_SLOT_LIGAND and 0 <= r0 and r1 <= n_nodes
            and r1 - r0 == (a1 - a0) + int(bits.sum()) and not bits[n_rec:].any())


def _accumulate(slot_rec, rec_sum, rec_count, rec_max):
    n_slots, n_rec = slot_rec.shape
    for j in range(n_rec):
        for p in range(n_slots):                 # slot order: what the float64 sum is rounded in
            v = slot_rec[p, j]
            if not np.isnan(v):
                rec_sum[j] = rec_sum[j] + np.float64(v)
                rec_count[j] += 1
                if np.isnan(rec_max[j]) or v > rec_max[j] or (v == rec_max[j] and np.signbit(rec_max[j])):
                    rec_max[j] = v


def _reduce(row_value, n_nodes, node_ptr, lig_ptr, keep, n_rec, rec_sum, rec_count, rec_max, lig_out, need_ligand):
    """Both operators: row_value(r) is the value of node row r. need_ligand: a slot without ligand atoms gives NaN."""
    n_slots = len(node_ptr) - 1
    keep = np.asarray(keep).reshape(n_slots, -1)
    lig_out = np.array(lig_out, dtype=np.float32)
    rec_sum, rec_count = np.array(rec_sum, dtype=np.float64), np.array(rec_count, dtype=np.int32)
    rec_max = np.array(rec_max, dtype=np.float32)
    slot_rec = np.full((n_slots, n_rec), np.nan, dtype=np.float32)
    for p in range(n_slots):
        if not slot_ok(node_ptr, lig_ptr, keep[p], p, n_rec, n_nodes):
            continue
        a0, n_lig, node0 = int(lig_ptr[p]), int(lig_ptr[p + 1] - lig_ptr[p]), int(node_ptr[p])
        for i in range(n_lig):
            lig_out[a0 + i] = row_value(node0 + i)
        if need_ligand and n_lig == 0:
            continue
        rank = 0
        for j in np.flatnonzero(words_mask(keep[p], n_rec)):
            slot_rec[p, j] = row_value(node0 + n_lig + rank)
            rank += 1
    _accumulate(slot_rec, rec_sum, rec_count, rec_max)
    return lig_out, slot_rec, rec_sum, rec_count, rec_max


def contact_attention_cropped(rowptr, etype, att, node_ptr, lig_ptr, keep, n_rec, rec_sum, rec_count, rec_max, lig_att):
    """(lig_att, slot_rec_att [n_slots, n_rec], rec_sum, rec_count, rec_max) after one call: copies of the arrays given,
    updated. Edge ranges are clamped to the arrays, as in the kernel."""
    n_edges = len(etype)

    def value(r):
        return row_max(att, etype, max(int(rowptr[r]), 0), min(int(rowptr[r + 1]), n_edges))
    return _reduce(value, len(rowptr) - 1, node_ptr, lig_ptr, keep, n_rec, rec_sum, rec_count, rec_max, lig_att, False)


def slot_node_values_cropped(y, col, n_mean, node_ptr, lig_ptr, keep, n_rec, rec_sum, rec_count, rec_max, lig_val):
    y = np.asarray(y, dtype=np.float32)
    return _reduce(lambda r: node_value(y, r, col, n_mean), y.shape[0], node_ptr, lig_ptr, keep, n_rec, rec_sum,
                   rec_count, rec_max, lig_val, True)


# ---- the maps of a set of hits on their cropped complexes, from the CPU oracle ----

def _gather(per_hit, ligand, n_rec):
    per_hit = np.stack(per_hit) if per_hit else np.zeros((0, n_rec))
    has = ~np.isnan(per_hit)
    count = has.sum(0).astype(np.int32)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.where(count > 0, np.where(has, per_hit, 0.0).sum(0) / count, np.nan)
    top = np.where(count > 0, np.where(has, per_hit, -np.inf).max(0, initial=-np.inf), np.nan)
    return dict(ligand=ligand, per_hit=per_hit, mean=mean, count=count, max=top)


def _cropped_items(items, rec, rec_feats, crop_radius):
    """Per hit: (name, feats, pose, kept receptor indices, rec[kept], rec_feats[kept])."""
    import torch
    for name, feats, pose in items:
        kept = cropped_complex(feats.numpy(), pose.numpy(), rec_feats.numpy(), rec.numpy(), crop_radius)[2]
        idx = torch.from_numpy(kept).long()
        yield name, feats, pose, kept, rec[idx], rec_feats[idx]


def kept_counts(items, rec, rec_feats, crop_radius):
    return [len(kept) for _, _, _, kept, _, _ in _cropped_items(items, rec, rec_feats, crop_radius)]


def oracle_cropped_hotspots(sd, cfg, items, rec, rec_feats, radius, crop_radius, layers, dtype):
    """{layer: dict(ligand, per_hit [hits, n_rec], mean, count, max)} in float64: per hit _contact_ref.oracle_hotspots
    on its cropped complex, its receptor values scattered to [n_rec], NaN elsewhere. A hit that keeps nothing: an
    all-NaN row and NaN ligand values."""
    from tests._contact_ref import oracle_hotspots
    n_rec = int(rec.shape[0])
    rows = {layer: ([], {}) for layer in layers}
    for name, feats, pose, kept, rec_k, feats_k in _cropped_items(items, rec, rec_feats, crop_radius):
        if len(kept) == 0:
            for layer in layers:
                rows[layer][0].append(np.full(n_rec, np.nan))
                rows[layer][1][name] = np.full(int(pose.shape[0]), np.nan)
            continue
        one = oracle_hotspots(sd, cfg, [(name, feats, pose)], rec_k, feats_k, radius, layers, dtype)
        for layer in layers:
            full = np.full(n_rec, np.nan)
            full[kept] = one[layer]['per_hit'][0]
            rows[layer][0].append(full)
            rows[layer][1][name] = one[layer]['ligand'][name]
    return {layer: _gather(per_hit, ligand, n_rec) for layer, (per_hit, ligand) in rows.items()}


def oracle_cropped_cam(sd, cfg, items, rec, rec_feats, radius, crop_radius, dtype, **kw):
    """The same for _cam_ref.oracle_cam (kw: column, n_mean, tasks). A hit that keeps nothing still has ligand values:
    the oracle runs on its ligand atoms alone."""
    from tests._cam_ref import oracle_cam
    n_rec = int(rec.shape[0])
    per_hit, ligand = [], {}
    for name, feats, pose, kept, rec_k, feats_k in _cropped_items(items, rec, rec_feats, crop_radius):
        one = oracle_cam(sd, cfg, [(name, feats, pose)], rec_k, feats_k, radius, dtype, **kw)
        full = np.full(n_rec, np.nan)
        full[kept] = one['per_hit'][0]
        per_hit.append(full)
        ligand[name] = one['ligand'][name]
    return _gather(per_hit, ligand, n_rec)


def bound_of(a, b):
    """(max|value64|, noise32, the project's parity bound 1e-5 * max|value64| + 4 * noise32) of the fp64 map a and the
    single-thread fp32 map b; their NaN patterns and counts agree."""
    pairs = [(a[k], b[k]) for k in ('per_hit', 'mean', 'max')] + [(a['ligand'][n], b['ligand'][n]) for n in a['ligand']]
    assert np.array_equal(a['count'], b['count'])
    assert all(np.array_equal(np.isnan(u), np.isnan(v)) for u, v in pairs)
    live = [(u, v) for u, v in pairs if u.size and (~np.isnan(u)).any()]
    noise = max(float(np.nanmax(np.abs(u - v))) for u, v in live)
    scale = max(float(np.nanmax(np.abs(u))) for u, _ in live)
    return scale, noise, 1e-5 * scale + 4 * noise


def hotspot_pair(model, cfg, items, rec, rec_feats, radius, crop_radius, layers):
    """({layer: fp64 map}, {layer: bound}) for `model` (on the CPU)."""
    import torch
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    a = oracle_cropped_hotspots(sd, cfg, items, rec, rec_feats, radius, crop_radius, layers, torch.float64)
    b = single_thread(lambda: oracle_cropped_hotspots(sd, cfg, items, rec, rec_feats, radius, crop_radius, layers,
                                                      torch.float32))
    return a, {layer: bound_of(a[layer], b[layer])[2] for layer in layers}


def cam_pair(model, cfg, items, rec, rec_feats, radius, crop_radius, **kw):
    """(the fp64 map, its bound) for `model` (on the CPU)."""
    import torch
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    a = oracle_cropped_cam(sd, cfg, items, rec, rec_feats, radius, crop_radius, torch.float64, **kw)
    b = single_thread(lambda: oracle_cropped_cam(sd, cfg, items, rec, rec_feats, radius, crop_radius, torch.float32, **kw))
    return a, bound_of(a, b)[2]


# ---- the set-up of the sweep tests: tests/test_gpu_contact_attention.py's hits, receptor and model ----

CROPS = (7.0, 4.0)
_YARD = {}


def sweep_yardstick():
    """Hits, receptor and attention_model(31) of tests/test_gpu_contact_attention.py; per crop radius of CROPS the fp64
    maps of layers 1 and 3 and of the CAM on the cropped complexes with their bounds, and the uncropped fp64 attention
    maps beside them; computed once."""
    if not _YARD:
        import torch
        from tests import test_gpu_contact_attention as setup
        from tests._contact_ref import oracle_hotspots
        items, rec, rec_feats = setup.hits_and_receptor()
        model = setup.attention_model(31)
        cfg = dict(setup.KW, edge_attention=True, num_layers=3, _class='SartorrasEGNN')
        sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
        _YARD.update(items=items, rec=rec, rec_feats=rec_feats, model=model, cfg=cfg, radius=setup.RADIUS, att={},
                     att_bound={}, cam={}, cam_bound={}, kept={},
                     uncropped=oracle_hotspots(sd, cfg, items, rec, rec_feats, setup.RADIUS, (1, 3), torch.float64))
        for crop in CROPS:
            _YARD['kept'][crop] = kept_counts(items, rec, rec_feats, crop)
            _YARD['att'][crop], _YARD['att_bound'][crop] = hotspot_pair(model, cfg, items, rec, rec_feats, setup.RADIUS,
                                                                        crop, (1, 3))
            _YARD['cam'][crop], _YARD['cam_bound'][crop] = cam_pair(model, cfg, items, rec, rec_feats, setup.RADIUS, crop)
            print(f"crop {crop:g}: kept {_YARD['kept'][crop]} attention bounds "
                  f"{ {k: f'{v:.3e}' for k, v in _YARD['att_bound'][crop].items()} } cam bound "
                  f"{_YARD['cam_bound'][crop]:.3e}")
    return _YARD
