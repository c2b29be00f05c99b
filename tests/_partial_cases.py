"""Inputs and fp64 references of the partial-first-layer tests (tests/test_gpu_partial_layer.py; pinned on the host by
tests/test_partial_cases_host.py). Screening sums the first layer's receptor-receptor messages once
(pvs_egnn_layer_edge_sums: the BASE set) and runs the layer per batch over the ligand-touching edges only
(pvs_egnn_layer_fwd_partial: the PARTIAL set) on top of those sums.

`case`       one explicit edge list (no radius, so no decision band), split by construction into the two sets, with
             the kind of every row on record. The split is the screens' own: `bp` marks the ligand atoms, the partial
             set holds exactly the edges whose row or column is one, so pvs_graph_filter_ligand_edges of the union
             graph must give the partial set back.
`edge_sums`  the message, attention and coordinate lines of oracle.egnn_oracle.egnn_layer over one edge set
`finish`     the rest of the layer on such sums
`Problem`    a layer, its inputs, the fp64 arbiter (egnn_layer on the union graph) and three fp32 oracle draws
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from tests._golden import assert_strict, edge_permutations

N_NODES = 320
KINDS = ('none', 'base', 'partial', 'mixed')
NONE_ROWS = (5, 6, 77, 130, 131, 200, 255, 300, 317, 318)      # pairs of neighbours, and two rows before the last
N_BASE_ONLY, N_PARTIAL_ONLY = 45, 25        # drawn rows (the end rows of a variant come on top)
ONE_BASE, ONE_PARTIAL, ONE_ONE, HUB = 20, 40, 60, 164       # rows of exactly 1 / 1 / 1 + 1 / HUB_PARTIAL + HUB_BASE edges
HUB_PARTIAL, HUB_BASE = 200, 150
ENDS = ('base', 'partial')                  # the kind of the first and of the last node
CLASS_COUNTS = (0, 2, 3, 5)
POS_SCALE = 2.0


def _classes(rng, n, A, hub_slots):
    """Class vector with shares that fall as 2^-c; the first A of `hub_slots` (edges of the hub) carry every class."""
    p = 0.5 ** np.arange(A)
    et = rng.choice(A, size=n, p=p / p.sum())
    et[hub_slots[:A]] = np.arange(A)
    return et.astype(np.int64)


@functools.lru_cache(maxsize=None)
def case(A=3, ends='base', seed=20260501):
    """-> namespace: n_nodes, pos [N, 3] fp32, bp uint8 [N] (0 = ligand atom), kind int [N] (index into KINDS),
    rows {kind name: row ids}, base_index / part_index int64 [2, E], base_etype / part_etype int64 [E] or None,
    base_attr / part_attr int64 one-hot [E, A] or None. The partial list is CSR-sorted by row; the base list is in
    arbitrary order. Rows, kinds and edges are the same for every A."""
    assert ends in ENDS and A in CLASS_COUNTS
    rng = np.random.default_rng(seed)
    n = N_NODES
    kind = np.full(n, KINDS.index('mixed'))
    kind[list(NONE_ROWS)] = KINDS.index('none')
    fixed = set(NONE_ROWS) | {0, n - 1, ONE_BASE, ONE_PARTIAL, ONE_ONE, HUB}
    free = rng.permutation([i for i in range(n) if i not in fixed])
    kind[free[:N_BASE_ONLY - 1]] = KINDS.index('base')
    kind[free[N_BASE_ONLY - 1:N_BASE_ONLY + N_PARTIAL_ONLY - 2]] = KINDS.index('partial')
    kind[ONE_BASE], kind[ONE_PARTIAL] = KINDS.index('base'), KINDS.index('partial')
    end_draws = rng.integers(2, 21, size=2)            # (drawn whatever the variant: the rest stays the same)
    kind[[0, n - 1]] = KINDS.index(ends)
    bp = (kind != KINDS.index('partial')).astype(np.uint8)       # ligand atoms: the rows that keep all their edges
    ligand, receptor = np.flatnonzero(bp == 0), np.flatnonzero(bp == 1)

    def columns(i, count, pool):
        return rng.choice(pool[pool != i], size=count)

    base_row, base_col, part_row, part_col = [], [], [], []
    everyone = np.arange(n)
    for i in range(n):
        k = KINDS[kind[i]]
        n_base, n_part = rng.integers(1, 13, size=2)          # (drawn for every row: the draws do not depend on the kinds)
        n_only = int(rng.integers(2, 21))
        if i in (0, n - 1):
            n_only = int(end_draws[0 if i == 0 else 1])
        if k == 'none':
            continue
        if k == 'base':
            n_base, n_part = (1 if i == ONE_BASE else n_only), 0
        elif k == 'partial':
            n_base, n_part = 0, (1 if i == ONE_PARTIAL else n_only)
        elif i == ONE_ONE:
            n_base, n_part = 1, 1
        elif i == HUB:
            n_base, n_part = HUB_BASE, HUB_PARTIAL
        base_row += [i] * int(n_base)
        base_col += list(columns(i, int(n_base), receptor))
        part_row += [i] * int(n_part)
        # a ligand row keeps every edge; a receptor row's partial edges are its contacts with ligand atoms
        part_col += list(columns(i, int(n_part), everyone if k == 'partial' else ligand))
    base = np.array([base_row, base_col], dtype=np.int64)
    part = np.array([part_row, part_col], dtype=np.int64)
    base = base[:, rng.permutation(base.shape[1])]
    base_et = part_et = None
    if A:
        base_et = _classes(rng, base.shape[1], A, np.flatnonzero(base[0] == HUB))
        part_et = _classes(rng, part.shape[1], A, np.flatnonzero(part[0] == HUB))
    pos = (rng.normal(size=(n, 3)) * POS_SCALE).astype(np.float32)

    def one_hot(et):
        return None if et is None else F.one_hot(torch.from_numpy(et), A)

    return SimpleNamespace(
        n_nodes=n, A=A, ends=ends, pos=torch.from_numpy(pos), bp=torch.from_numpy(bp), kind=kind,
        rows={k: np.flatnonzero(kind == KINDS.index(k)) for k in KINDS},
        base_index=torch.from_numpy(base), part_index=torch.from_numpy(part),
        base_etype=None if base_et is None else torch.from_numpy(base_et),
        part_etype=None if part_et is None else torch.from_numpy(part_et),
        base_attr=one_hot(base_et), part_attr=one_hot(part_et))


def union(c):
    """(edge_index, edge_attr) of the whole graph: the base list, then the partial list."""
    ei = torch.cat([c.base_index, c.part_index], dim=1)
    return ei, (None if c.A == 0 else torch.cat([c.base_attr, c.part_attr], dim=0))


# ---- the layer in two halves ------------------------------------------------------------------------------------------
_ATT_ACT = {'sigmoid': torch.sigmoid, 'tanh': torch.tanh, 'relu': torch.relu, 'silu': F.silu}


def edge_sums(sd, kw, h, x, edge_index, edge_attr, dtype):
    """The row-side sums of one layer's edge work over `edge_index` only, in `dtype`, edges added in list order:
    (magg [N, H] = sum_j att_ij m_ij, xsum [N, 3] = sum_j (x_i - x_j) s_ij without the 1 / deg (zeros without
    update_coords), deg [N] = edge counts). No edge residual, no softmax attention: sums of two edge sets add."""
    assert not kw['edge_residual'] and not kw['softmax_attention']
    sd = {k: v.detach().to(dtype) for k, v in sd.items()}
    h, x = h.detach().to(dtype), x.detach().to(dtype)
    row, col = edge_index[0], edge_index[1]
    n = h.size(0)
    diff = x[row] - x[col]
    radial = (diff ** 2).sum(1, keepdim=True)
    if kw['normalize']:
        diff = diff / (radial.sqrt() + 1e-8)
    parts = [h[row] + h[col], radial] if kw['permutation_invariance'] else [h[row], h[col], radial]
    if edge_attr is not None:
        parts.append(edge_attr.to(dtype))
    z = F.silu(F.linear(torch.cat(parts, dim=1), sd['edge_mlp.0.weight'], sd['edge_mlp.0.bias']))
    m = F.silu(F.linear(z, sd['edge_mlp.2.weight'], sd['edge_mlp.2.bias']))
    xsum = torch.zeros((n, 3), dtype=dtype)
    if kw['update_coords']:
        s = F.silu(F.linear(m, sd['coord_mlp.0.weight'], sd['coord_mlp.0.bias']))
        s = F.linear(s, sd['coord_mlp.2.weight'])
        if kw['tanh']:
            s = torch.tanh(s)
        xsum.index_add_(0, row, diff * s)
    if kw['edge_attention']:
        att = F.linear(m, sd['att_mlp.0.weight'], sd['att_mlp.0.bias'])
        m = _ATT_ACT[kw['attention_activation_fn']](att) * m
    magg = torch.zeros((n, h.size(1)), dtype=dtype).index_add_(0, row, m)
    deg = torch.zeros(n, dtype=dtype).index_add_(0, row, torch.ones(row.numel(), dtype=dtype))
    return magg, xsum, deg


def finish(sd, kw, h, x, magg, xsum, deg):
    """The rest of the layer on the sums of ALL its edges: -> (h', x', node attention or None), in magg's dtype."""
    from oracle.egnn_oracle import graph_norm
    dtype = magg.dtype
    sd = {k: v.detach().to(dtype) for k, v in sd.items()}
    h, x = h.detach().to(dtype), x.detach().to(dtype)
    if kw['update_coords']:
        x = x + xsum / deg.clamp(min=1).unsqueeze(1)
    out = F.linear(torch.cat([h, magg], dim=1), sd['node_mlp.0.weight'], sd['node_mlp.0.bias'])
    if kw['graphnorm']:
        out = graph_norm(out, sd['node_mlp.1.weight'], sd['node_mlp.1.bias'], sd['node_mlp.1.mean_scale'])
    out = F.linear(F.silu(out), sd['node_mlp.3.weight'], sd['node_mlp.3.bias'])
    natt = None
    if kw['node_attention']:
        natt = _ATT_ACT[kw['attention_activation_fn']](
            F.linear(out, sd['node_att_mlp.0.weight'], sd['node_att_mlp.0.bias']))
        out = out * natt
    if kw['residual']:
        if kw['rezero']:
            out = h + sd['node_gate_parameter'] * out
        elif kw['gated_residual']:
            gate = torch.relu(sd['node_gate_parameter'])
            out = gate * out + (1 - gate) * h
        else:
            out = h + out
    return out, x, natt


# ---- flag sets --------------------------------------------------------------------------------------------------------
def flag_sets():
    """The flag sets of tests/test_gpu_edge_classes.py that the partial entries accept, and two of this file's:
    `full-` (that file's `full` without edge_residual) and `nocoords` (update_coords=False)."""
    from tests.test_gpu_edge_classes import FLAGS
    names = ('plain', 'perm', 'nores', 'gn', 'natt-sigmoid', 'natt-tanh', 'natt-relu', 'natt-silu', 'rezero0', 'rezero',
             'gated+', 'gated0', 'gated-', 'eatt-tanh', 'eatt-relu', 'eatt-silu')
    out = {k: FLAGS[k] for k in names}
    out['full-'] = dict(FLAGS['full'], edge_residual=False)
    out['nocoords'] = dict(update_coords=False)
    return out


def oracle_kwargs(flags):
    from oracle import egnn_oracle as orc
    kw = dict(orc.BUILD_NET_DEFAULTS, residual=True, normalize=False, tanh=False, graphnorm=False)   # EGNNLayer's defaults
    kw.update(flags)
    kw['edge_attention_here'], kw['node_attention_here'] = kw['edge_attention'], kw['node_attention']
    return kw


LAYER_SEED = 11
COORD_GAIN = 4.0      # on top of _new_layer's 100: under tanh + normalize an edge moves its row by at most tanh(s), and
                      # every defect of tests/test_partial_cases_host.py has to clear 100 x the bound there as well


class Problem:
    """A layer (tests/test_gpu_edge_classes.py _new_layer: every parameter away from its symmetric initial value), node
    features, the case's graph, and every compared tensor as numpy: `ref64` from the arbiter - egnn_layer in fp64 on the
    union graph, and edge_sums in fp64 over the base set -, `ref32` the same in fp32, once in list order and twice
    under edge permutations. Built once per (A, hid, flags, ends) and left unchanged."""

    def __init__(self, A, hid, flags_name, ends='base'):
        from tests.test_gpu_edge_classes import _new_layer
        self.A, self.hid, self.flags_name, self.flags = A, hid, flags_name, flag_sets()[flags_name]
        self.case = case(A, ends)
        self.kw = oracle_kwargs(self.flags)
        self.sd = {k: v.detach().clone() for k, v in _new_layer(A, hid, self.flags, LAYER_SEED).state_dict().items()}
        self.sd['coord_mlp.2.weight'] *= COORD_GAIN
        self.h0 = torch.randn((self.case.n_nodes, hid), generator=torch.Generator().manual_seed(7 + A))
        self.n_base, self.n_part = int(self.case.base_index.shape[1]), int(self.case.part_index.shape[1])
        self.ref64 = self.oracle(torch.float64)
        perms = edge_permutations(self.n_base + self.n_part, count=2)
        base_perms = edge_permutations(self.n_base, count=2, seed=20260502)
        self.ref32 = [self.oracle(torch.float32)] + [self.oracle(torch.float32, p, b) for p, b in zip(perms, base_perms)]
        # what a row kind means for a per-edge tensor over the partial list: the kind of the edge's row
        self.part_edges = {k: np.flatnonzero(self.case.kind[self.case.part_index[0].numpy()] == KINDS.index(k))
                           for k in KINDS}

    def new_layer(self):
        from tests.test_gpu_edge_classes import _new_layer
        layer = _new_layer(self.A, self.hid, self.flags, LAYER_SEED)
        layer.load_state_dict(self.sd)
        return layer

    def oracle(self, dtype, perm=None, base_perm=None):
        """h_out, x_out, natt, att over the partial list (in its order) of egnn_layer on the union graph, and base_magg /
        base_xsum / base_deg of edge_sums over the base list; `perm` / `base_perm` reorder the edges first."""
        from oracle import egnn_oracle as orc
        c = self.case
        ei, ea = union(c)
        bi, ba = c.base_index, c.base_attr
        if perm is not None:
            ei, ea = ei[:, perm], (None if ea is None else ea[perm])
            bi, ba = bi[:, base_perm], (None if ba is None else ba[base_perm])
        sd = {k: v.to(dtype) for k, v in self.sd.items()}
        with torch.no_grad():
            h, x, _, att, natt = orc.egnn_layer(sd, '', self.kw, self.h0.to(dtype), ei, c.pos.to(dtype), ea, None)
            magg, xsum, deg = edge_sums(self.sd, self.kw, self.h0, c.pos, bi, ba, dtype)
        res = dict(h_out=h, x_out=x, base_magg=magg, base_xsum=xsum, base_deg=deg)
        if natt is not None:
            res['natt'] = natt.reshape(-1)
        if att is not None:
            if perm is not None:
                back = torch.empty_like(att)
                back[perm] = att
                att = back
            res['att'] = att.reshape(-1)[self.n_base:]
        return {k: v.numpy() for k, v in res.items()}

    def subsets(self, key):
        """(label, index array) of the row kinds of tensor `key` (its edges' rows for `att`)."""
        table = self.part_edges if key == 'att' else self.case.rows
        return [(k, table[k]) for k in KINDS]

    def bound(self, key, rows=None):
        """The strict bound the GPU test applies to `key` (to its rows `rows`): from the oracle's numbers alone."""
        from tests._golden import strict_margin
        pick = (lambda a: a) if rows is None else (lambda a: a[rows])
        ref64 = pick(self.ref64[key])
        return strict_margin(ref64, ref64, [pick(r[key]) for r in self.ref32])[1]

    def check(self, got, tag, log, keys=None, n_rows=None):
        """assert_strict on each tensor of `got` as a whole and on the rows of each kind as tensors of their own.
        n_rows: only that many leading rows of the node tensors are compared (the rest is padding)."""
        for key in (got if keys is None else keys):
            value = np.asarray(got[key])
            assert value.dtype == np.float32, key
            if n_rows is not None and key != 'att':
                value = value[:n_rows]
            ref64, ref32 = self.ref64[key], [r[key] for r in self.ref32]
            value = value.reshape(ref64.shape)
            assert_strict(value, ref64, ref32, f'{tag} {key}', log=log)
            for label, idx in self.subsets(key):
                if idx.size == 0:       # (att: no partial edge has a row without partial edges)
                    continue
                assert_strict(value[idx], ref64[idx], [r[idx] for r in ref32], f'{tag} {key}[{label} rows]', log=log)


@functools.lru_cache(maxsize=None)
def problem(A, hid, flags_name, ends='base'):
    return Problem(A, hid, flags_name, ends)
