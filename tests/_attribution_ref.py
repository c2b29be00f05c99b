"""Test helper for the attribution tests: the attribution fixtures (tests/golden/attr_*.npz, made by
tests/golden/make_golden_attribution.py from the real reference) and a numpy restatement of how the reference builds a
masked graph (attribution_fns.py:58-100, 405-422): drop the atoms, drop every edge that touches one, shift the ids
above each dropped atom down by one. Fed through oracle.egnn_oracle's fp64 forward it is the yardstick of the GPU tests.
"""
import json
from pathlib import Path

import numpy as np
import torch

GOLDEN_DIR = Path(__file__).resolve().parent / 'golden'
ATTR_CASES = sorted(p.stem for p in GOLDEN_DIR.glob('attr_*.npz'))
REL, NOISE = 1e-5, 4.0          # README "Parity": 1e-5 * max|ref64| + 4 * noise32


class AttrCase:
    def __init__(self, name):
        self.name = name
        z = np.load(GOLDEN_DIR / f'{name}.npz')
        self.z = z
        self.meta = json.loads(str(z['cfg']))
        self.cfg = dict(self.meta['kwargs'], _class=self.meta['class'])
        self.sd = {k[3:]: z[k] for k in z.files if k.startswith('sd/')}
        self.x, self.pos = torch.from_numpy(z['in/x']), torch.from_numpy(z['in/pos'])
        self.edge_index = torch.from_numpy(z['in/edge_index'].astype(np.int64))
        self.edge_type = torch.from_numpy(z['in/edge_type'].astype(np.int64))
        self.edge_attr = torch.nn.functional.one_hot(self.edge_type, 3)
        self.visited = z['visited'].astype(np.int64)
        self.raw32, self.raw64 = z['raw32'].astype(np.float64), z['raw64']
        self.scores, self.noise32 = z['scores'], float(z['noise32'])
        self.fn, self.sigmoid = self.meta['fn'], bool(self.meta['sigmoid'])
        self.n = int(self.x.shape[0])

    def drop_table(self):
        """[M, 2]: what each visited mask leaves out (second slot -1: one atom)."""
        if self.fn == 'atom_masking':
            return np.stack([np.arange(self.n), np.full(self.n, -1)], axis=1)
        ei = self.edge_index.numpy()[:, self.visited]
        return np.stack([ei.min(0), ei.max(0)], axis=1)

    def bound(self, ref64=None):
        ref64 = self.raw64 if ref64 is None else ref64
        return REL * float(np.abs(ref64).max()) + NOISE * self.noise32


def masked_coo(edge_index, edge_type, drop):
    """(edge_index' [2, E'], edge_type' [E'], kept node ids) of the graph without the atoms in `drop` (entries < 0 are
    empty slots); numpy int64."""
    edge_index = np.asarray(edge_index, dtype=np.int64)
    gone = sorted({int(d) for d in np.asarray(drop).reshape(-1) if d >= 0})
    keep = ~np.isin(edge_index[0], gone) & ~np.isin(edge_index[1], gone)
    ei = edge_index[:, keep]
    shift = np.zeros_like(ei)
    for d in gone:
        shift += ei > d
    n = None if edge_type is None else np.asarray(edge_type)[keep]
    return ei - shift, n, gone


def kept_nodes(n_nodes, drop):
    gone = {int(d) for d in np.asarray(drop).reshape(-1) if d >= 0}
    return np.array([i for i in range(n_nodes) if i not in gone], dtype=np.int64)


def oracle_outputs(case, dtype=torch.float64, drop=None):
    """[1 + M, dim_output]: the oracle's output for the unmasked graph, then for every masked graph of `drop`."""
    from oracle import egnn_oracle as orc
    sd = {k: torch.from_numpy(np.asarray(v)).to(dtype) for k, v in case.sd.items()}
    drop = case.drop_table() if drop is None else np.asarray(drop).reshape(-1, 2)
    outs = []
    ei0, et0 = case.edge_index.numpy(), case.edge_type.numpy()
    with torch.no_grad():
        for d in [np.array([-1, -1])] + list(drop):
            ei, et, _ = masked_coo(ei0, et0, d)
            keep = torch.from_numpy(kept_nodes(case.n, d))
            batch = torch.zeros(len(keep), dtype=torch.long)
            out = orc.model_forward(sd, case.cfg, case.x[keep].to(dtype), case.pos[keep].to(dtype),
                                    torch.from_numpy(ei), torch.nn.functional.one_hot(torch.from_numpy(et), 3),
                                    batch, n_graphs=1)
            outs.append(out.double().reshape(-1).numpy())
    return np.stack(outs)


def unique_pair_first(case):
    """Positions in `visited` of the first edge of every unordered atom pair (a contact is listed once per direction and
    both directions leave out the same two atoms, so their scores tie exactly: rankings are over pairs)."""
    d = case.drop_table()
    _, first = np.unique(d[:, 0] * case.n + d[:, 1], return_index=True)
    return np.sort(first)


def ranked_scores(case, scores):
    """The scores the ranking is over: every atom, or one per contact pair."""
    scores = np.asarray(scores, dtype=np.float64)
    if case.fn == 'atom_masking':
        return scores
    return scores[case.visited[unique_pair_first(case)]]
