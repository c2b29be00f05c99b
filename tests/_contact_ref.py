"""Test helper: a numpy restatement of the contact-attention reduction (pvs_contact_attention, PF.contact_attention) over
the compact pose-batch layout - slot p owns the rows node_ptr[p] .. node_ptr[p + 1], its ligand atoms first, then the
n_rec receptor atoms - written as plain loops: per row the largest attention value over the edges of class 1 that are
not NaN (NaN without one), per receptor atom the running sum (float64, slot order), count and maximum over the slots.
"""
import numpy as np


def row_max(att, etype, e0, e1):
    """float32: max of att[e0:e1] over the entries with etype == 1 that are not NaN; NaN when there is none. (+0.0 is
    above -0.0.)"""
    vals = np.asarray(att[e0:e1], dtype=np.float32)[np.asarray(etype[e0:e1]) == 1]
    vals = vals[~np.isnan(vals)]
    if vals.size == 0:
        return np.float32(np.nan)
    top = vals.max()
    if top == 0 and np.any((vals == 0) & ~np.signbit(vals)):
        top = np.float32(0.0)
    return np.float32(top)


def contact_attention(rowptr, etype, att, node_ptr, lig_ptr, n_rec, rec_sum, rec_count, rec_max, lig_att):
    """Returns (lig_att, slot_rec_att [n_slots, n_rec], rec_sum, rec_count, rec_max) after one call: lig_att and the
    three accumulators are copies of the arrays given, updated (lig_att: the rows below lig_ptr[n_slots] only)."""
    n_slots = len(node_ptr) - 1
    lig_att = np.array(lig_att, dtype=np.float32)
    rec_sum, rec_count = np.array(rec_sum, dtype=np.float64), np.array(rec_count, dtype=np.int32)
    rec_max = np.array(rec_max, dtype=np.float32)
    slot_rec_att = np.full((n_slots, n_rec), np.nan, dtype=np.float32)
    for p in range(n_slots):
        n_lig = int(lig_ptr[p + 1] - lig_ptr[p])
        assert int(node_ptr[p]) == int(lig_ptr[p]) + p * n_rec and int(node_ptr[p + 1] - node_ptr[p]) == n_lig + n_rec
        for i in range(n_lig):
            row = int(node_ptr[p]) + i
            lig_att[int(lig_ptr[p]) + i] = row_max(att, etype, rowptr[row], rowptr[row + 1])
        for j in range(n_rec):
            row = int(node_ptr[p]) + n_lig + j
            slot_rec_att[p, j] = row_max(att, etype, rowptr[row], rowptr[row + 1])
    for j in range(n_rec):
        for p in range(n_slots):                 # slot order: what the float64 sum is rounded in
            v = slot_rec_att[p, j]
            if not np.isnan(v):
                rec_sum[j] = rec_sum[j] + np.float64(v)
                rec_count[j] += 1
                if np.isnan(rec_max[j]) or v > rec_max[j] or (v == rec_max[j] and np.signbit(rec_max[j])):
                    rec_max[j] = v
    return lig_att, slot_rec_att, rec_sum, rec_count, rec_max


def fresh_accumulators(n_rec):
    return np.zeros(n_rec, dtype=np.float64), np.zeros(n_rec, dtype=np.int32), np.full(n_rec, np.nan, dtype=np.float32)


# ---- the hotspot map of a set of hits from the CPU oracle (the yardstick of ScreeningSweep.receptor_hotspots) ----

def radius_gap(items, rec, radius):
    """The smallest | d - radius | over the fp64 distances of every atom pair of every complex (ligand atoms of item k
    + the receptor): how far the nearest pair is from being decided the other way."""
    from oracle.generate_edges_oracle import cdist_euclidean
    gap = np.inf
    for _, _, pose in items:
        d = cdist_euclidean(np.concatenate([np.asarray(pose, dtype=np.float64), np.asarray(rec, dtype=np.float64)]))
        gap = min(gap, float(np.abs(d - radius).min()))
    return gap


def oracle_hotspots(sd, cfg, items, rec, rec_feats, radius, layers, dtype):
    """{layer: dict(ligand {name: [n]}, per_hit [hits, n_rec], mean, count, max [n_rec])} in float64 from the oracle run
    in `dtype`: per hit the oracle's generate_edges list (inter = intra radius, no pruning), its model_forward with a
    trace, per atom the max of att{layer} over the row's class-1 edges (NaN without one); then per receptor atom the
    mean / count / max over the hits that are not NaN. sd: numpy state dict; items: (name, lig_feats, pose) on the CPU;
    layers: indices into model.layers (1 = the first EGNN layer)."""
    import torch
    from oracle import egnn_oracle as orc
    from oracle.generate_edges_oracle import generate_edges
    sd = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}
    n_rec = int(rec.shape[0])
    rows_of = {layer: dict(ligand={}, per_hit=[]) for layer in layers}
    with torch.no_grad():
        for name, feats, pose in items:
            n = int(pose.shape[0])
            pos, x = torch.cat([pose, rec], 0), torch.cat([feats, rec_feats], 0)
            _, (rows, cols), attrs = generate_edges(pos.numpy(), x[:, -1].numpy(), radius, radius, prune=False)
            trace = {}
            orc.model_forward(sd, cfg, x, pos, torch.from_numpy(np.vstack([rows, cols])).long(),
                              torch.nn.functional.one_hot(torch.from_numpy(attrs).long(), 3),
                              torch.zeros(n + n_rec, dtype=torch.long), n_graphs=1, trace=trace)
            for layer in layers:
                att = trace[f'att{layer}'].double().reshape(-1).numpy()[attrs == 1]
                top = np.full(n + n_rec, -np.inf)
                np.maximum.at(top, rows[attrs == 1], att)
                top[np.isinf(top)] = np.nan
                rows_of[layer]['ligand'][name] = top[:n]
                rows_of[layer]['per_hit'].append(top[n:])
    out = {}
    for layer, r in rows_of.items():
        per_hit = np.stack(r['per_hit']) if r['per_hit'] else np.zeros((0, n_rec))
        has = ~np.isnan(per_hit)
        count = has.sum(0).astype(np.int32)
        total = np.where(has, per_hit, 0.0).sum(0)
        with np.errstate(invalid='ignore', divide='ignore'):
            mean = np.where(count > 0, total / count, np.nan)
        top = np.where(count > 0, np.where(has, per_hit, -np.inf).max(0, initial=-np.inf), np.nan)
        out[layer] = dict(ligand=r['ligand'], per_hit=per_hit, mean=mean, count=count, max=top)
    return out
