"""Masking attribution of a GraphNorm model with per_graph_norm=True: the leave-out copies run `bs` per forward, every
copy normalised by its own statistics (PreparedGraph.set_norm_segments on the leave-out batch), and give what one copy
per forward gives - the reference's semantics.

On the reference-made GraphNorm fixture tests/golden/attr_testkwargs_g1.npz: the raw outputs against the oracle's fp64
run of every masked graph ALONE and the scores against the fixture's reference values, at the bounds of
tests/test_gpu_attribution.py (1e-5 * max|ref64| + 4 * noise32, twice that for the scores); the number of model forwards
is counted.
"""
import math

import numpy as np
import pytest
import torch

from tests._attribution_ref import AttrCase, oracle_outputs
from tests.test_gpu_attribution import _args, _model, _ref64

pytestmark = pytest.mark.gpu
NAME = 'attr_testkwargs_g1'
OTHER_ROWS = 40          # masks of the method the fixture was not made with (the oracle runs each one on the CPU)


class _Forwards:
    """Counts the model's forwards."""

    def __init__(self, model):
        self.model, self.n = model, 0

    def __enter__(self):
        self.handle = self.model.register_forward_hook(lambda *a: setattr(self, 'n', self.n + 1))
        return self

    def __exit__(self, *exc):
        self.handle.remove()


def _raw(c, model, drop, **kw):
    from pointvs_amd import attribution as T
    orig, masked = T.masked_outputs(model, c.pos[None], c.x[None], drop, 32, **_args(c), **kw)
    return np.concatenate([orig.reshape(1, -1).double().cpu().numpy(), masked.double().cpu().numpy()])


def _other_table(c):
    """The mask table of the method the fixture was NOT made with, its first OTHER_ROWS rows."""
    from pointvs_amd.attribution import bond_mask_table
    if c.fn == 'atom_masking':
        _, drop = bond_mask_table(c.edge_index.numpy(), c.edge_attr.numpy())
    else:
        drop = np.stack([np.arange(c.n), np.full(c.n, -1)], axis=1)
    return np.asarray(drop).reshape(-1, 2)[:OTHER_ROWS]


def test_batched_copies_meet_the_bound_of_one_copy_per_forward_and_run_in_chunks():
    from pointvs_amd import attribution as T
    c = AttrCase(NAME)
    model = _model(c)
    assert T.couples_graphs(model) and T.segments_refusal(model) is None
    ref64 = _ref64(c)
    bound = c.bound(ref64)
    drop = c.drop_table()
    m = len(drop)
    step = T.chunk_size(32, m, c.n, int(c.edge_index.shape[1]))
    assert 1 < step <= 32 and m > step        # (more than one copy per forward, more than one forward)
    with _Forwards(model) as batched:
        got = _raw(c, model, drop, per_graph_norm=True)
    assert batched.n == 1 + math.ceil(m / step)          # the unmasked complex, then ceil(M / step) - not M
    assert got.shape == ref64.shape
    err = float(np.abs(got - ref64).max())
    print(f'{NAME}: per_graph_norm raw err {err:.3e} bound {bound:.3e} (noise32 {c.noise32:.2e})')
    assert err <= bound, f'|raw - ref64| = {err:.3e} > {bound:.3e}'
    # the default call still runs one copy per forward, and gives the same within the bound
    with _Forwards(model) as looped:
        one = _raw(c, model, drop)
    assert looped.n == 1 + m
    assert float(np.abs(one - ref64).max()) <= bound
    # a model WITHOUT GraphNorm: the keyword changes nothing, bit for bit
    plain = AttrCase('attr_clidefault_g1')
    if not T.couples_graphs(_model(plain)):
        pm = _model(plain)
        a, b = _raw(plain, pm, plain.drop_table()), _raw(plain, pm, plain.drop_table(), per_graph_norm=True)
        assert np.array_equal(a, b)


def test_scores_of_both_methods():
    from pointvs_amd import attribution as T
    c = AttrCase(NAME)
    model = _model(c)
    ref64 = _ref64(c)
    bound = c.bound(ref64)
    fn = getattr(T, c.fn)
    was = T.SIGMOID
    try:
        T.SIGMOID = c.sigmoid
        scores = fn(model, c.pos[None].cuda(), c.x[None].cuda(), per_graph_norm=True, **_args(c))
    finally:
        T.SIGMOID = was
    assert isinstance(scores, np.ndarray) and scores.shape == c.scores.shape
    sig = (lambda a: 1.0 / (1.0 + np.exp(-a))) if c.sigmoid else (lambda a: a)
    pick = 0 if ref64.shape[1] == 1 else 1
    want = np.zeros_like(c.scores)
    want[c.visited if c.fn == 'bond_masking' else slice(None)] = sig(ref64[0, pick]) - sig(ref64[1:, pick])
    s_err = float(np.abs(scores - want).max())
    print(f'{NAME}: {c.fn} per_graph_norm score err {s_err:.3e} bound {2 * bound:.3e}')
    assert s_err <= 2 * bound
    assert float(np.abs(scores - c.scores).max()) <= 2 * bound + 2 * c.noise32      # the fixture's reference values
    # the other masking method: its first masks against the oracle on each masked graph alone
    drop = _other_table(c)
    ref_other = oracle_outputs(c, drop=drop)
    got = _raw(c, model, drop, per_graph_norm=True)
    b_other = c.bound(ref_other)
    err = float(np.abs(got - ref_other).max())
    print(f'{NAME}: other method raw err {err:.3e} bound {b_other:.3e}')
    assert err <= b_other
    # and through the public entry: the keyword reaches masked_outputs
    other = T.bond_masking if c.fn == 'atom_masking' else T.atom_masking
    with _Forwards(model) as counted:
        other(model, c.pos[None].cuda(), c.x[None].cuda(), per_graph_norm=True, **_args(c))
    n_masks = (len(T.bond_mask_table(c.edge_index.numpy(), c.edge_attr.numpy())[1]) if c.fn == 'atom_masking' else c.n)
    assert counted.n == 1 + math.ceil(n_masks / T.chunk_size(32, n_masks, c.n, int(c.edge_index.shape[1])))


def test_fp64_and_wide_models_keep_one_copy_per_forward():
    """Where the layers refuse segments the call keeps one copy per forward and raises nothing."""
    from pointvs_amd import attribution as T
    c = AttrCase(NAME)
    model = _model(c, torch.float64)
    assert T.segments_refusal(model) is not None
    drop = c.drop_table()[:5]
    with _Forwards(model) as counted:
        got = _raw(c, model, drop, per_graph_norm=True)
    assert counted.n == 1 + len(drop)
    ref64 = _ref64(c)
    assert float(np.abs(got - ref64[:6]).max()) <= 1e-9 * float(np.abs(ref64).max())
