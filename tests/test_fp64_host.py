"""fp64 (--double) host side without a GPU: the CLI accepts the flag and the C ABI declares the fp64 entries."""
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
F64_SYMBOLS = ('pvs_egnn_layer_saved_doubles_f64', 'pvs_egnn_layer_workspace_bytes_f64', 'pvs_egnn_layer_fwd_f64',
               'pvs_egnn_layer_bwd_f64', 'pvs_linear_fwd_f64', 'pvs_linear_bwd_workspace_bytes_f64',
               'pvs_linear_bwd_f64', 'pvs_mean_pool_fwd_f64', 'pvs_mean_pool_bwd_f64',
               'pvs_segment_workspace_bytes_f64', 'pvs_segment_reduce_fwd_f64', 'pvs_segment_reduce_bwd_f64')


def test_double_is_no_longer_refused():
    from point_vs.parse_args import parse_args, unsupported_in_use
    args = parse_args(['egnn', '/tmp/pvs_fp64_cli', '--double'])
    assert args.double
    assert unsupported_in_use(args) == []


def test_fp64_entries_are_declared_prototyped_and_exported():
    import ctypes
    from pointvs_amd import _lib
    header = (ROOT / 'include' / 'pvs_egnn.h').read_text()
    declared = set(re.findall(r'\b(pvs_[a-z0-9_]+)\s*\(', header))
    for name in F64_SYMBOLS:
        assert name in declared, name
        assert name in _lib.EXPORTED_SYMBOLS, name
    assert 'PvsLayerParamsF64' in header and 'PvsLayerGradsF64' in header
    assert [f for f, _ in _lib.PvsLayerParamsF64._fields_] == list(_lib.PARAM_FIELDS)
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for name in F64_SYMBOLS:
        assert hasattr(handle, name), name
    assert _lib.lib().pvs_version() >= 101


def test_fp64_workspace_and_saved_sizes():
    import ctypes
    from pointvs_amd import _lib
    lib = _lib.lib()
    for hidden in (16, 32, 64):
        desc = _lib.PvsLayerDesc(hidden, 3, _lib.GRAPHNORM | _lib.UPDATE_COORDS, 0)
        n, e = 100, 1000
        assert lib.pvs_egnn_layer_saved_doubles_f64(ctypes.byref(desc), n, e) == 4 * n * hidden + n + 2 * hidden
        fwd = lib.pvs_egnn_layer_workspace_bytes_f64(ctypes.byref(desc), n, e, 0)
        bwd = lib.pvs_egnn_layer_workspace_bytes_f64(ctypes.byref(desc), n, e, 1)
        assert 2 * n * hidden * 8 < fwd < bwd
        assert bwd >= 5 * e * hidden * 8


def test_both_dtype_kinds_name_the_same_operators():
    """functional.KINDS: an operator added to one kind only, an entry that is not exported or not in the built library, or
    an fp64 entry whose argument count differs from its fp32 twin's fails here, without a GPU."""
    import ctypes
    import torch
    from pointvs_amd import _lib
    from pointvs_amd import functional as PF
    assert set(PF.KINDS) == {torch.float32, torch.float64}
    k32, k64 = PF.KINDS[torch.float32], PF.KINDS[torch.float64]
    assert (k32.dtype, k32.words, k64.dtype, k64.words) == (torch.float32, 1, torch.float64, 2)
    assert list(k32.entry) == list(k64.entry) and len(k32.entry) >= 14
    handle = ctypes.CDLL(str(_lib.LIB_PATH))
    for kind in (k32, k64):
        for op, symbol in kind.entry.items():
            assert symbol in _lib.EXPORTED_SYMBOLS, (op, symbol)
            assert hasattr(handle, symbol), (op, symbol)
            assert getattr(kind, op).argtypes == _lib._PROTOTYPES[symbol][1], (op, symbol)      # (bound on first use)
        for struct in (kind.params_t, kind.grads_t):
            assert [f for f, _ in struct._fields_] == list(_lib.PARAM_FIELDS), struct
    for op in k32.entry:
        r32, a32 = _lib._PROTOTYPES[k32.entry[op]]
        r64, a64 = _lib._PROTOTYPES[k64.entry[op]]
        assert len(a32) == len(a64) and r32 is r64, op
    assert set(k64.entry.values()) - set(k32.entry.values()) == set(F64_SYMBOLS)
    assert (k32.params_t, k32.grads_t) == (_lib.PvsLayerParams, _lib.PvsLayerGrads)
    assert (k64.params_t, k64.grads_t) == (_lib.PvsLayerParamsF64, _lib.PvsLayerGradsF64)
    assert PF.STACK_KIND is k32
    assert not hasattr(k32, 'no_such_operator')


def test_dead_gradients_follow_one_rule():
    """functional.dead_grads, the rule shared by _EGNNLayerFn.backward and the stack's _GradLayout."""
    from pointvs_amd import _lib
    from pointvs_amd.functional import dead_grads
    coord = {'coord_w1', 'coord_b1', 'coord_w2'}
    uc, rz, gr = _lib.UPDATE_COORDS, _lib.REZERO, _lib.GATED_RESIDUAL
    assert set(dead_grads(uc, True, False)) == {'edge_gate'}
    assert set(dead_grads(uc, False, False)) == coord | {'edge_gate'}
    assert set(dead_grads(0, True, True)) == coord | {'edge_gate'}
    assert set(dead_grads(uc | rz, True, True)) == set()
    assert set(dead_grads(uc | gr, False, True)) == coord
    assert set(dead_grads(uc | gr, True, False)) == {'edge_gate'}
    assert set(dead_grads(rz | _lib.EDGE_RESIDUAL, True, True)) == coord
