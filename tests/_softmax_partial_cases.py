"""Inputs and fp64 references of the softmax partial-first-layer tests (tests/test_gpu_softmax_partial_layer.py; pinned on
the host by tests/test_softmax_partial_cases_host.py): the cases of tests/_partial_cases.py for layers with edge attention
under softmax_attention, whose row sums over two edge sets do not add while their softmax statistics merge exactly.

`stats`      per row of ONE edge set T: mu_T = max l_e, S_T = sum exp(l_e - mu_T), A_T = sum exp(l_e - mu_T) m_e / S_T
             (zeros for a row without an edge), the raw coordinate sums, the degrees and the logits
`merge`      the statistics of the base set and of the partial set -> every row's M, its attention factor a_g / (a_b + a_g)
             and the partial edges' attention normalised over BOTH sets
`finish`     the rest of the layer; under softmax_attention the node attention has NO activation (egnn_satorras.py:66-71),
             so tests/_partial_cases.finish, which applies attention_activation_fn, is not used
`SoftProblem` a layer, its inputs, the fp64 arbiter (egnn_layer on the union graph) and three fp32 oracle draws; `gain`
             multiplies att_mlp.0.weight (the WIDE variant: maxima of the two sets tens of units apart)
"""
import functools
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from tests import _partial_cases as pc
from tests._golden import edge_permutations

GAINS = (60, 20, 6)         # the wide variant's gains, largest first
UNDERFLOW = 104.0           # exp(-x) is exactly 0 in fp32 (denormals included) for x > 103.98
DRY_SCALE = 3.0             # the wide variant's h0 on the two columns of row dry[0]: ligand columns are few, and the widest
                            # gap below zero that one of them gives at gain 60 is -98; with the features tripled, -108


def flag_sets():
    from tests.test_gpu_edge_classes import FLAGS
    soft = FLAGS['soft']
    return {'soft': soft,
            'soft-natt': dict(soft, node_attention=True),
            'soft-full': dict(soft, node_attention=True, normalize=True, tanh=True, graphnorm=True, gated_residual=True),
            'soft-nocoords': dict(soft, update_coords=False)}


def _messages(sd, kw, h, x, edge_index, edge_attr):
    """m [E, H], s * diff [E, 3] or None, logits [E] of one edge list: the lines of egnn_layer up to the attention."""
    row, col = edge_index[0], edge_index[1]
    diff = x[row] - x[col]
    radial = (diff ** 2).sum(1, keepdim=True)
    if kw['normalize']:
        diff = diff / (radial.sqrt() + 1e-8)
    parts = [h[row] + h[col], radial] if kw['permutation_invariance'] else [h[row], h[col], radial]
    if edge_attr is not None:
        parts.append(edge_attr.to(h.dtype))
    z = F.silu(F.linear(torch.cat(parts, dim=1), sd['edge_mlp.0.weight'], sd['edge_mlp.0.bias']))
    m = F.silu(F.linear(z, sd['edge_mlp.2.weight'], sd['edge_mlp.2.bias']))
    moves = None
    if kw['update_coords']:
        s = F.silu(F.linear(m, sd['coord_mlp.0.weight'], sd['coord_mlp.0.bias']))
        s = F.linear(s, sd['coord_mlp.2.weight'])
        moves = diff * (torch.tanh(s) if kw['tanh'] else s)
    logits = F.linear(m, sd['att_mlp.0.weight'], sd['att_mlp.0.bias']).reshape(-1)
    return m, moves, logits


def stats(sd, kw, h, x, edge_index, edge_attr, dtype):
    """-> namespace(A [N, H], mu [N], S [N], xsum [N, 3], deg [N], logits [E], row) of one edge set, in `dtype`, edges
    added in list order. A row without an edge has A = mu = S = 0: its base row is the all-zero row."""
    assert kw['softmax_attention'] and kw['edge_attention'] and not kw['edge_residual']
    sd = {k: v.detach().to(dtype) for k, v in sd.items()}
    h, x = h.detach().to(dtype), x.detach().to(dtype)
    n, row = h.size(0), edge_index[0]
    m, moves, logits = _messages(sd, kw, h, x, edge_index, edge_attr)
    mu = torch.full((n,), float('-inf'), dtype=dtype).scatter_reduce(0, row, logits, 'amax', include_self=True)
    deg = torch.zeros(n, dtype=dtype).index_add_(0, row, torch.ones(row.numel(), dtype=dtype))
    mu = torch.where(deg > 0, mu, torch.zeros_like(mu))
    w = (logits - mu[row]).exp()
    S = torch.zeros(n, dtype=dtype).index_add_(0, row, w)
    A = torch.zeros((n, h.size(1)), dtype=dtype).index_add_(0, row, w.unsqueeze(1) * m) / S.clamp(min=1).unsqueeze(1)
    xsum = torch.zeros((n, 3), dtype=dtype)
    if moves is not None:
        xsum.index_add_(0, row, moves)
    return SimpleNamespace(A=A, mu=mu, S=S, xsum=xsum, deg=deg, logits=logits, row=row)


def merge(b, g, shift=True):
    """The statistics of base set b and partial set g -> (M [N, H], factor [N], att [E_g] over ALL edges of each row).
    shift=False: the defect of weighting by S alone, without the shift to the common maximum."""
    has_b, has_g = b.deg > 0, g.deg > 0
    mu = torch.maximum(b.mu, g.mu)
    a_b = torch.where(has_b, b.S * ((b.mu - mu).exp() if shift else 1.0), torch.zeros_like(mu))
    a_g = torch.where(has_g, g.S * ((g.mu - mu).exp() if shift else 1.0), torch.zeros_like(mu))
    # (a set without an edge has mu = 0 on record, not -inf: where only one set has edges its own weight is all there is)
    a_b = torch.where(has_b & ~has_g, b.S, a_b)
    a_g = torch.where(has_g & ~has_b, g.S, a_g)
    total = (a_b + a_g).clamp(min=torch.finfo(mu.dtype).tiny)
    wb, wg = a_b / total, a_g / total
    M = wb.unsqueeze(1) * b.A + wg.unsqueeze(1) * g.A
    att = (g.logits - g.mu[g.row]).exp() / g.S.clamp(min=1)[g.row] * wg[g.row]
    return M, wg, att


def finish(sd, kw, h, x, M, xsum, deg, node_activation=None):
    """The rest of the layer on M and the coordinate sums of ALL edges -> (h', x', node attention or None).
    node_activation: None for the reference's Identity under softmax_attention, else the activation (a defect)."""
    from oracle.egnn_oracle import graph_norm
    dtype = M.dtype
    sd = {k: v.detach().to(dtype) for k, v in sd.items()}
    h, x = h.detach().to(dtype), x.detach().to(dtype)
    if kw['update_coords']:
        x = x + xsum / deg.clamp(min=1).unsqueeze(1)
    out = F.linear(torch.cat([h, M], dim=1), sd['node_mlp.0.weight'], sd['node_mlp.0.bias'])
    if kw['graphnorm']:
        out = graph_norm(out, sd['node_mlp.1.weight'], sd['node_mlp.1.bias'], sd['node_mlp.1.mean_scale'])
    out = F.linear(F.silu(out), sd['node_mlp.3.weight'], sd['node_mlp.3.bias'])
    natt = None
    if kw['node_attention']:
        natt = F.linear(out, sd['node_att_mlp.0.weight'], sd['node_att_mlp.0.bias'])
        if node_activation is not None:
            natt = node_activation(natt)
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


def merged_layer(p, dtype, **defect):
    """The whole layer through stats / merge / finish in `dtype` -> dict of numpy arrays with the keys of ref64.
    defect: drop_base, partial_att, no_shift, sigmoid_node (each True switches one defect on)."""
    c = p.case
    b = stats(p.sd, p.kw, p.h0, c.pos, c.base_index, c.base_attr, dtype)
    g = stats(p.sd, p.kw, p.h0, c.pos, c.part_index, c.part_attr, dtype)
    M, fac, att = merge(b, g, shift=not defect.get('no_shift'))
    if defect.get('drop_base'):
        M = g.A
    if defect.get('partial_att'):
        att = (g.logits - g.mu[g.row]).exp() / g.S.clamp(min=1)[g.row]
    h, x, natt = finish(p.sd, p.kw, p.h0, c.pos, M, b.xsum + g.xsum, b.deg + g.deg,
                        torch.sigmoid if defect.get('sigmoid_node') else None)
    out = dict(h_out=h, x_out=x, att=att)
    if natt is not None:
        out['natt'] = natt.reshape(-1)
    return {k: v.numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def wide_case(A, ends, hid, flags_name, gain):
    """`case` with 1 + 1 edges (class 0) added to two of its rows without edges, chosen from the layer's own fp64 logits
    at `gain`: the row `dry[0]` is the one whose lowest-logit receptor column (its base edge) lies furthest below its
    highest-logit ligand column (its partial edge) - the base side's weight underflows -, `dry[1]` the one, of the others,
    with the widest gap the other way round. `scaled`: the two columns of row dry[0], whose features SoftProblem multiplies
    by DRY_SCALE. The partial list stays CSR-sorted; both rows become mixed rows."""
    c = pc.case(A, ends)
    p = SoftProblem(A, hid, flags_name, ends, gain, _case=c)
    ligand, receptor = np.flatnonzero(c.bp.numpy() == 0), np.flatnonzero(c.bp.numpy() == 1)
    sd = {k: v.double() for k, v in p.sd.items()}
    found = {}          # row -> ((lowest base logit, its column), (highest, column), the same two of the ligand pool)
    for r in pc.NONE_ROWS:
        assert c.kind[r] == pc.KINDS.index('none') and c.bp[r] == 1
        ends_of = []
        for pool in (receptor[receptor != r], ligand):
            ei = torch.from_numpy(np.stack([np.full(pool.size, r), pool]))
            ea = None if A == 0 else F.one_hot(torch.zeros(pool.size, dtype=torch.int64), A)
            logits = _messages(sd, p.kw, p.h0.double(), c.pos.double(), ei, ea)[2].numpy()
            ends_of += [(float(logits.min()), int(pool[logits.argmin()])), (float(logits.max()), int(pool[logits.argmax()]))]
        found[r] = ends_of
    base_dry = min(found, key=lambda r: found[r][0][0] - found[r][3][0])
    part_dry = max((r for r in found if r != base_dry), key=lambda r: found[r][1][0] - found[r][2][0])
    extra_b = [(base_dry, found[base_dry][0][1]), (part_dry, found[part_dry][1][1])]
    extra_p = [(base_dry, found[base_dry][3][1]), (part_dry, found[part_dry][2][1])]
    kind = c.kind.copy()
    kind[[base_dry, part_dry]] = pc.KINDS.index('mixed')
    base = np.concatenate([c.base_index.numpy(), np.array(extra_b, dtype=np.int64).T], 1)
    part = np.concatenate([c.part_index.numpy(), np.array(extra_p, dtype=np.int64).T], 1)
    order = np.argsort(part[0], kind='stable')
    part = part[:, order]
    zeros = np.zeros(2, dtype=np.int64)
    base_et = None if A == 0 else np.concatenate([c.base_etype.numpy(), zeros])
    part_et = None if A == 0 else np.concatenate([c.part_etype.numpy(), zeros])[order]

    def one_hot(et):
        return None if et is None else F.one_hot(torch.from_numpy(et), A)

    return SimpleNamespace(
        n_nodes=c.n_nodes, A=A, ends=ends, pos=c.pos, bp=c.bp, kind=kind, dry=(base_dry, part_dry),
        scaled=(found[base_dry][0][1], found[base_dry][3][1]),
        rows={k: np.flatnonzero(kind == pc.KINDS.index(k)) for k in pc.KINDS},
        base_index=torch.from_numpy(base), part_index=torch.from_numpy(part),
        base_etype=None if base_et is None else torch.from_numpy(base_et),
        part_etype=None if part_et is None else torch.from_numpy(part_et),
        base_attr=one_hot(base_et), part_attr=one_hot(part_et))


class SoftProblem(pc.Problem):
    """tests/_partial_cases.Problem for a softmax layer: `ref64` holds h_out, x_out, natt, att over the partial list (of
    egnn_layer on the union graph) and base_A / base_mu / base_S / base_xsum / base_deg of `stats` over the base list;
    `ref32` the same in fp32, once in list order and twice under edge permutations. gain != 1: att_mlp.0.weight times
    gain, on `wide_case`."""

    def __init__(self, A, hid, flags_name, ends='base', gain=1, _case=None):
        from tests.test_gpu_edge_classes import _new_layer
        self.A, self.hid, self.flags_name, self.flags, self.gain = A, hid, flags_name, flag_sets()[flags_name], gain
        self.kw = pc.oracle_kwargs(self.flags)
        self.sd = {k: v.detach().clone() for k, v in _new_layer(A, hid, self.flags, pc.LAYER_SEED).state_dict().items()}
        self.sd['coord_mlp.2.weight'] *= pc.COORD_GAIN
        self.sd['att_mlp.0.weight'] *= float(gain)
        self.h0 = torch.randn((pc.N_NODES, hid), generator=torch.Generator().manual_seed(7 + A))
        if _case is not None:       # (wide_case's own use: the layer and inputs, no references)
            self.case = _case
            return
        self.case = pc.case(A, ends) if gain == 1 else wide_case(A, ends, hid, flags_name, gain)
        if gain != 1:
            self.h0[list(self.case.scaled)] *= DRY_SCALE
        self.n_base, self.n_part = int(self.case.base_index.shape[1]), int(self.case.part_index.shape[1])
        self.ref64 = self.oracle(torch.float64)
        perms = edge_permutations(self.n_base + self.n_part, count=2)
        base_perms = edge_permutations(self.n_base, count=2, seed=20260502)
        self.ref32 = [self.oracle(torch.float32)] + [self.oracle(torch.float32, p, b) for p, b in zip(perms, base_perms)]
        self.part_edges = {k: np.flatnonzero(self.case.kind[self.case.part_index[0].numpy()] == pc.KINDS.index(k))
                           for k in pc.KINDS}

    def oracle(self, dtype, perm=None, base_perm=None):
        from oracle import egnn_oracle as orc
        c = self.case
        ei, ea = pc.union(c)
        bi, ba = c.base_index, c.base_attr
        if perm is not None:
            ei, ea = ei[:, perm], (None if ea is None else ea[perm])
            bi, ba = bi[:, base_perm], (None if ba is None else ba[base_perm])
        sd = {k: v.to(dtype) for k, v in self.sd.items()}
        with torch.no_grad():
            h, x, _, att, natt = orc.egnn_layer(sd, '', self.kw, self.h0.to(dtype), ei, c.pos.to(dtype), ea, None)
            b = stats(self.sd, self.kw, self.h0, c.pos, bi, ba, dtype)
        if perm is not None:
            back = torch.empty_like(att)
            back[perm] = att
            att = back
        res = dict(h_out=h, x_out=x, att=att.reshape(-1)[self.n_base:], base_A=b.A, base_mu=b.mu, base_S=b.S,
                   base_xsum=b.xsum, base_deg=b.deg)
        if natt is not None:
            res['natt'] = natt.reshape(-1)
        return {k: v.numpy() for k, v in res.items()}

    def reference_base_rows(self):
        """[N, H + 4] fp32: the fp64 reference statistics over the base list, rounded."""
        r = self.ref64
        z = np.zeros_like(r['base_mu'])
        return np.concatenate([r['base_A'], np.stack([r['base_mu'], r['base_S'], z, z], 1)], 1).astype(np.float32)

    def gaps(self):
        """(mu_b - mu_g of every row from the fp64 statistics, the mixed rows)."""
        c = self.case
        b = stats(self.sd, self.kw, self.h0, c.pos, c.base_index, c.base_attr, torch.float64)
        g = stats(self.sd, self.kw, self.h0, c.pos, c.part_index, c.part_attr, torch.float64)
        d = (b.mu - g.mu).numpy()
        return d, c.rows['mixed']


@functools.lru_cache(maxsize=None)
def problem(A, hid, flags_name, ends='base', gain=1):
    return SoftProblem(A, hid, flags_name, ends, gain)
