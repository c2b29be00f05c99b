"""Test helper: the yardsticks of the class-activation maps. (1) A numpy restatement of the slot operator
(pvs_slot_node_values, PF.slot_node_values) over the compact pose-batch layout - slot p owns the rows node_ptr[p] ..
node_ptr[p + 1], its ligand atoms first, then the n_rec receptor atoms - as plain loops in fp32 in the stated order, with
a double sum in slot order. (2) The CAM of a set of hits from the CPU oracle: the head applied to every row of the
oracle's final embedding (trace['h{L}'])."""
import numpy as np

MAX_SLOT_LIGAND = 1024


def node_value(y, r, col, n_mean):
    """fp32: y[r, col], or ((y[r, col] + y[r, col + 1]) + y[r, col + 2]) / 3 with every step rounded to fp32."""
    if n_mean == 1:
        return np.float32(y[r, col])
    assert n_mean == 3
    s = np.float32(np.float32(y[r, col]) + np.float32(y[r, col + 1]))
    s = np.float32(s + np.float32(y[r, col + 2]))
    return np.float32(s / np.float32(3.0))


def slot_ok(node_ptr, lig_ptr, p, n_slots, n_rec, n_nodes):
    """The slots the operator accepts: both tables agree, 0..1024 ligand atoms, rows inside the ligand room."""
    a0, a1 = int(lig_ptr[p]), int(lig_ptr[p + 1])
    return (a0 >= 0 and a1 >= a0 and a1 - a0 <= MAX_SLOT_LIGAND and a1 <= n_nodes - n_slots * n_rec
            and int(node_ptr[p]) == a0 + p * n_rec and int(node_ptr[p + 1]) == a1 + (p + 1) * n_rec)


def slot_node_values(y, col, n_mean, node_ptr, lig_ptr, n_rec, rec_sum, rec_count, rec_max, lig_val):
    """Returns (lig_val, slot_rec_val [n_slots, n_rec], rec_sum, rec_count, rec_max) after one call: lig_val and the
    three accumulators are copies of the arrays given, updated."""
    y = np.asarray(y, dtype=np.float32)
    n_nodes, n_slots = y.shape[0], len(node_ptr) - 1
    lig_val = np.array(lig_val, dtype=np.float32)
    rec_sum, rec_count = np.array(rec_sum, dtype=np.float64), np.array(rec_count, dtype=np.int32)
    rec_max = np.array(rec_max, dtype=np.float32)
    slot_rec_val = np.full((n_slots, n_rec), np.nan, dtype=np.float32)
    for p in range(n_slots):
        if not slot_ok(node_ptr, lig_ptr, p, n_slots, n_rec, n_nodes):
            continue
        a0, n_lig = int(lig_ptr[p]), int(lig_ptr[p + 1] - lig_ptr[p])
        node0 = a0 + p * n_rec
        for i in range(n_lig):
            lig_val[a0 + i] = node_value(y, node0 + i, col, n_mean)
        if n_lig > 0:
            for j in range(n_rec):
                slot_rec_val[p, j] = node_value(y, node0 + n_lig + j, col, n_mean)
    for j in range(n_rec):
        for p in range(n_slots):                 # slot order: what the float64 sum is rounded in
            v = slot_rec_val[p, j]
            if not np.isnan(v):
                rec_sum[j] = rec_sum[j] + np.float64(v)
                rec_count[j] += 1
                if np.isnan(rec_max[j]) or v > rec_max[j] or (v == rec_max[j] and np.signbit(rec_max[j])):
                    rec_max[j] = v
    return lig_val, slot_rec_val, rec_sum, rec_count, rec_max


def fresh_accumulators(n_rec):
    return np.zeros(n_rec, dtype=np.float64), np.zeros(n_rec, dtype=np.int32), np.full(n_rec, np.nan, dtype=np.float32)


# ---- the CAM of a set of hits from the CPU oracle (the yardstick of receptor_hotspots(attribution='cam')) ----

def oracle_node_outputs(sd, cfg, h, tasks=None):
    """The raw outputs [n, C] of the heads on every row of h (torch, the oracle's dtype): the head code of
    oracle.egnn_oracle.model_forward, applied per node instead of to the pooled row. tasks: 'pose', 'affinity' or 'both'
    (pose first) for a MultitaskSatorrasEGNN."""
    import torch
    import torch.nn.functional as F
    if cfg.get('_class') == 'MultitaskSatorrasEGNN':
        cols = []
        if tasks in ('pose', 'both'):
            cols.append(F.linear(h, sd['feats_linear_layers_pose.0.weight'], sd['feats_linear_layers_pose.0.bias']))
        if tasks in ('affinity', 'both'):
            out = F.linear(h, sd['feats_linear_layers_affinity.0.weight'], sd['feats_linear_layers_affinity.0.bias'])
            cols.append(F.softplus(out) if cfg.get('final_softplus', False) else torch.relu(out))
        return torch.cat(cols, 1)
    idx, out = 0, h
    n_fc = 3 if cfg.get('multi_fc', False) else 1
    for fc in range(n_fc):
        out = F.linear(out, sd[f'feats_linear_layers.{idx}.weight'], sd[f'feats_linear_layers.{idx}.bias'])
        idx += 1
        if fc < n_fc - 1:
            out = F.silu(out)
            idx += 1
    return F.softplus(out) if cfg.get('final_softplus', False) else out


def oracle_cam(sd, cfg, items, rec, rec_feats, radius, dtype, column=0, n_mean=1, tasks=None):
    """dict(ligand {name: [n]}, per_hit [hits, n_rec], mean, count, max [n_rec], score {name: the model's own output
    row}) in float64 from the oracle run in `dtype`: per hit the oracle's generate_edges list (inter = intra radius, no
    pruning), its model_forward with a trace, the heads on every row of the final embedding, and per node column
    `column` of them or the mean of the three columns from it; then per receptor atom mean / count / max over the hits
    that have atoms. sd: numpy state dict; items: (name, lig_feats, pose) on the CPU."""
    import torch
    from oracle import egnn_oracle as orc
    from oracle.generate_edges_oracle import generate_edges
    sd = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in sd.items()}
    n_rec, last = int(rec.shape[0]), int(cfg['num_layers'])
    ligand, per_hit, score = {}, [], {}
    with torch.no_grad():
        for name, feats, pose in items:
            n = int(pose.shape[0])
            if n == 0:
                ligand[name] = np.zeros(0)
                per_hit.append(np.full(n_rec, np.nan))
                continue
            pos, x = torch.cat([pose, rec], 0), torch.cat([feats, rec_feats], 0)
            _, (rows, cols), attrs = generate_edges(pos.numpy(), x[:, -1].numpy(), radius, radius, prune=False)
            trace = {}
            out = orc.model_forward(sd, cfg, x, pos, torch.from_numpy(np.vstack([rows, cols])).long(),
                                    torch.nn.functional.one_hot(torch.from_numpy(attrs).long(), 3),
                                    torch.zeros(n + n_rec, dtype=torch.long), n_graphs=1, trace=trace)
            node_y = oracle_node_outputs(sd, cfg, trace[f'h{last}'], tasks).double().numpy()
            value = node_y[:, column] if n_mean == 1 else node_y[:, column:column + 3].mean(1)
            ligand[name], score[name] = value[:n], out.double().reshape(-1).numpy()
            per_hit.append(value[n:])
    per_hit = np.stack(per_hit) if per_hit else np.zeros((0, n_rec))
    has = ~np.isnan(per_hit)
    count = has.sum(0).astype(np.int32)
    with np.errstate(invalid='ignore', divide='ignore'):
        mean = np.where(count > 0, np.where(has, per_hit, 0.0).sum(0) / count, np.nan)
    top = np.where(count > 0, np.where(has, per_hit, -np.inf).max(0, initial=-np.inf), np.nan)
    return dict(ligand=ligand, per_hit=per_hit, mean=mean, count=count, max=top, score=score)


# ---- the set-up of the sweep tests: tests/test_gpu_contact_attention.py's hits, receptor and model ----

_YARD = {}


def single_thread(fn):
    """fn() with torch on one thread (the fp32 oracle's sums then have one order)."""
    import torch
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return fn()
    finally:
        torch.set_num_threads(threads)


def noise_and_bound(a, b):
    """(max|cam64| over the values compared, noise32: the largest distance of the fp32 oracle's map b from the fp64 map
    a, the parity bound 1e-5 * max|cam64| + 4 * noise32)."""
    pairs = [(a[k], b[k]) for k in ('per_hit', 'mean', 'max')] + [(a['ligand'][n], b['ligand'][n]) for n in a['ligand']]
    assert all(np.array_equal(np.isnan(u), np.isnan(v)) for u, v in pairs)
    noise = max(float(np.nanmax(np.abs(u - v))) for u, v in pairs if u.size)
    scale = max(float(np.nanmax(np.abs(u))) for u, _ in pairs if u.size)      # (every value compared, ligand atoms too)
    return scale, noise, 1e-5 * scale + 4 * noise


def score_bound(a, b):
    """The parity bound of the hits' own scores: 1e-5 * max|score64| + 4 * (the fp32 oracle's distance from them)."""
    names = list(a['score'])
    top = max(float(np.abs(a['score'][n]).max()) for n in names)
    noise = max(float(np.abs(a['score'][n] - b['score'][n]).max()) for n in names)
    return 1e-5 * top + 4 * noise


def oracle_pair(model, cfg, items, rec, rec_feats, radius, **kw):
    """(the fp64 oracle's CAM, max|cam64|, noise32, the bound, the bound of the hits' scores) for `model` (on the CPU)."""
    import torch
    sd = {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}
    a = oracle_cam(sd, cfg, items, rec, rec_feats, radius, torch.float64, **kw)
    b = single_thread(lambda: oracle_cam(sd, cfg, items, rec, rec_feats, radius, torch.float32, **kw))
    return (a,) + noise_and_bound(a, b) + (score_bound(a, b),)


def sweep_yardstick():
    """The fp64 oracle's CAM of the hits of tests/test_gpu_contact_attention.py (seed 8204, 150 receptor atoms, radius
    6.0, hits of 1 / 12 / 12 / 70 atoms, attention_model(31)), max|cam64|, noise32 and the bound; computed once."""
    if not _YARD:
        from tests import test_gpu_contact_attention as setup
        items, rec, rec_feats = setup.hits_and_receptor()
        model = setup.attention_model(31)
        cfg = dict(setup.KW, edge_attention=True, num_layers=3, _class='SartorrasEGNN')
        y64, scale, noise, bound, score = oracle_pair(model, cfg, items, rec, rec_feats, setup.RADIUS)
        print(f'cam: max|cam64| {scale:.4f} noise32 {noise:.3e} bound {bound:.3e}')
        _YARD.update(items=items, rec=rec, rec_feats=rec_feats, model=model, cfg=cfg, y64=y64, scale=scale, noise32=noise,
                     bound=bound, score_bound=score, radius=setup.RADIUS)
    return _YARD
