"""The five partial-layer entries (pvs_egnn_layer_edge_sums / _edge_stats_softmax / _fwd_partial / _fwd_partial_att /
_fwd_partial_softmax) on the host, without a GPU: every refusal below comes before the entry's first HIP call, so dummy
pointers are never followed. The sizes are literals recorded from the build before the entries shared one host path
(modes 2 and 3 of pvs_egnn_layer_workspace_bytes, and the arena need a too-small workspace is refused with): callers hold
buffers of these sizes, so the numbers are part of the interface."""
import ctypes as C

import pytest

from pointvs_amd import _lib

HIDDEN = (32, 64, 128)
# (N, E): around the 256-byte steps of att [max(E, 1)] and fac [N] (64 floats), with E = 0 and a larger pair
SHAPES = ((1, 0), (63, 64), (64, 65), (65, 1), (257, 4099))
SIGMOID = _lib.EDGE_ATTENTION | _lib.UPDATE_COORDS | _lib.RESIDUAL
SOFTMAX = SIGMOID | _lib.SOFTMAX_ATT

# pvs_egnn_layer_workspace_bytes(desc, N, E, mode): WORKSPACE[mode][hidden] in the order of SHAPES
WORKSPACE = {
    2: {32: (2832, 42512, 43024, 44304, 185360), 64: (3088, 82448, 83984, 85520, 349712),
        128: (5376, 196352, 199680, 169728, 2778368)},
    3: {32: (3088, 42768, 43280, 44816, 186640), 64: (3344, 82704, 84240, 86032, 350992),
        128: (5632, 196608, 199936, 170240, 2779648)},
}
# the second number of "workspace too small (0 < NEED)": NEED[mode][hidden] in the order of SHAPES
NEED = {
    2: {32: (2308, 42240, 42500, 43780, 184844), 64: (2564, 82176, 83460, 84996, 349196),
        128: (4612, 195840, 198916, 168964, 2777612)},
    3: {32: (2564, 42492, 43008, 44292, 186116), 64: (2820, 82428, 83968, 85508, 350468),
        128: (4868, 196092, 199424, 169476, 2778884)},
}
# entry -> (the name its messages carry, tensor arguments between params and workspace, workspace mode)
ENTRIES = {
    'pvs_egnn_layer_edge_sums': ('pvs_egnn_layer_edge_sums', 4, 2),
    'pvs_egnn_layer_fwd_partial': ('pvs_egnn_layer_fwd_partial', 9, 2),
    'pvs_egnn_layer_fwd_partial_att': ('pvs_egnn_layer_fwd_partial', 10, 2),
    'pvs_egnn_layer_edge_stats_softmax': ('pvs_egnn_layer_edge_stats_softmax', 4, 3),
    'pvs_egnn_layer_fwd_partial_softmax': ('pvs_egnn_layer_fwd_partial_softmax', 10, 3),
}


def _call(entry, hidden, flags, n, e, workspace_bytes=0):
    """The entry on dummy, distinct, 16-byte aligned, non-NULL pointers -> (return code, pvs_last_error())."""
    lib = _lib.lib()
    desc = _lib.PvsLayerDesc(hidden, 0, flags, 0)
    graph = _lib.PvsGraph(n_nodes=n, n_edges=e, rowptr=0x1000, row=0x2000, col=0x3000, inv_deg=0x4000)
    params = _lib.PvsLayerParams(*[0x10000 + 0x100 * i for i in range(len(_lib.PARAM_FIELDS))])
    tensors = [0x100000 + 0x1000 * i for i in range(ENTRIES[entry][1])]
    rc = getattr(lib, entry)(C.byref(desc), C.byref(graph), C.byref(params), *tensors, 0x800000, workspace_bytes, None)
    return rc, lib.pvs_last_error().decode()


def _flags_for(entry):
    return SOFTMAX if ENTRIES[entry][2] == 3 else SIGMOID


@pytest.mark.parametrize('mode', (2, 3))
@pytest.mark.parametrize('hidden', HIDDEN)
def test_workspace_sizes_are_the_recorded_ones(hidden, mode):
    lib = _lib.lib()
    desc = _lib.PvsLayerDesc(hidden, 0, SOFTMAX if mode == 3 else SIGMOID, 0)
    got = tuple(lib.pvs_egnn_layer_workspace_bytes(C.byref(desc), n, e, mode) for n, e in SHAPES)
    print(hidden, mode, got)
    assert got == WORKSPACE[mode][hidden]


@pytest.mark.parametrize('entry', sorted(ENTRIES))
@pytest.mark.parametrize('hidden', HIDDEN)
def test_too_small_workspace_is_refused_with_the_recorded_need(hidden, entry):
    who, _, mode = ENTRIES[entry]
    for (n, e), need, size in zip(SHAPES, NEED[mode][hidden], WORKSPACE[mode][hidden]):
        rc, msg = _call(entry, hidden, _flags_for(entry), n, e)
        print(entry, hidden, n, e, rc, msg)
        assert rc != 0
        assert msg == f'{who}: workspace too small (0 < {need})'
        assert need <= size


@pytest.mark.parametrize('entry', sorted(ENTRIES))
def test_kind_refusals(entry):
    soft = ENTRIES[entry][2] == 3
    own, other = (SOFTMAX, SIGMOID) if soft else (SIGMOID, SOFTMAX)
    cases = [(64, other, 'for layers with edge attention and softmax attention only' if soft
              else 'softmax attention is not supported'),
             (64, own | _lib.EDGE_RESIDUAL, 'edge_residual layers are not supported'),
             (16, own, 'needs the MFMA edge kernel')]
    if soft:      # (a softmax flag without edge attention is no softmax layer)
        cases.append((64, _lib.SOFTMAX_ATT | _lib.UPDATE_COORDS, 'for layers with edge attention and softmax attention only'))
    for hidden, flags, text in cases:
        rc, msg = _call(entry, hidden, flags, 65, 64)
        print(entry, hidden, hex(flags), rc, msg)
        assert rc != 0 and text in msg
        assert msg.startswith('softmax partial forward' if soft else 'partial-sum forward')
