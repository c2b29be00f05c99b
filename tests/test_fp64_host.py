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
