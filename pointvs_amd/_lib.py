"""ctypes binding of libpvs_egnn.so (C ABI declared in include/pvs_egnn.h)."""
import ctypes as C
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get('PVS_EGNN_LIB', _HERE / 'libpvs_egnn.so'))

# PVS_* layer flags (pvs_egnn.h)
RESIDUAL, EDGE_RESIDUAL, EDGE_ATTENTION, NORMALIZE = 1 << 0, 1 << 1, 1 << 2, 1 << 3
TANH, GRAPHNORM, UPDATE_COORDS, PERM_INVARIANT = 1 << 4, 1 << 5, 1 << 6, 1 << 7
NODE_ATTENTION, GATED_RESIDUAL, REZERO, SOFTMAX_ATT = 1 << 8, 1 << 9, 1 << 10, 1 << 11
# forward only, with GRAPHNORM: PvsGraph.n_norm_rows_dev is a segment table [n_graphs + 1], GraphNorm runs per segment
GRAPHNORM_SEGMENTS = 1 << 12
ACT_CODES = {'sigmoid': 0, 'tanh': 1, 'relu': 2, 'silu': 3, 'identity': 4}

PARAM_FIELDS = (
    'edge_w1', 'edge_b1', 'edge_w2', 'edge_b2', 'coord_w1', 'coord_b1', 'coord_w2', 'att_w',
    'att_b', 'node_w1', 'node_b1', 'node_w2', 'node_b2', 'gn_weight', 'gn_bias', 'gn_mean_scale',
    'node_att_w', 'node_att_b', 'edge_gate', 'node_gate')


class PvsLayerDesc(C.Structure):
    _fields_ = [('hidden', C.c_int32), ('n_edge_attr', C.c_int32), ('flags', C.c_uint32),
                ('att_act', C.c_int32)]


class PvsGraph(C.Structure):
    _fields_ = [('n_nodes', C.c_int32), ('n_edges', C.c_int32), ('rowptr', C.c_void_p),
                ('row', C.c_void_p), ('col', C.c_void_p), ('etype', C.c_void_p),
                ('perm', C.c_void_p), ('colptr', C.c_void_p), ('cedge', C.c_void_p),
                ('inv_deg', C.c_void_p), ('n_edges_dev', C.c_void_p), ('graph_eptr', C.c_void_p),
                ('n_graphs', C.c_int32), ('n_norm_rows_dev', C.c_void_p)]


# sizeof(PvsGraph) and offsetof(PvsGraph, n_norm_rows_dev) as include/pvs_egnn.h states (and static_asserts) them
PVS_GRAPH_SIZEOF, PVS_GRAPH_NORM_ROWS_OFFSET = 104, 96


class PvsLayerParams(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in PARAM_FIELDS]


class PvsLayerGrads(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in PARAM_FIELDS]


class PvsLayerParamsF64(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in PARAM_FIELDS]


class PvsLayerGradsF64(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in PARAM_FIELDS]


class PvsRaggedNodeTables(C.Structure):
    _fields_ = [('n_feats', C.c_int32), ('hidden', C.c_int32)] + [(name, C.c_void_p) for name in (
        'lig_feats', 'rec_feats', 'rec_magg', 'rec_xsum', 'rec_deg', 'feats', 'base_magg', 'base_xsum', 'base_deg')]


class PvsCsrOut(C.Structure):
    _fields_ = [('rowptr', C.c_void_p), ('row', C.c_void_p), ('col', C.c_void_p), ('etype', C.c_void_p),
                ('capacity', C.c_int32)]


SLOTS_RAGGED, SLOTS_STRUCK, SLOTS_CROPPED = 0, 1, 2       # PVS_SLOTS_* (pvs_egnn.h)


class PvsScreenSlotsJob(C.Structure):
    """The pose-batch slot builders' job, field for field as pvs_egnn.h declares it (tests/test_screen_job_host.py
    compares every offset with the C compiler's). Pointer fields take a device address (`ptr(tensor)`) or None."""
    _fields_ = ([('layout', C.c_int32)] +
                [(name, C.c_void_p) for name in ('lig_pos', 'lig_ptr', 'rec_drop', 'rec_pos', 'rr_rowptr', 'rr_col')] +
                [(name, C.c_int32) for name in ('n_slots', 'lig_cap', 'n_rec', 'slot_cap')] +
                [(name, C.c_double) for name in ('inter_radius', 'intra_radius', 'crop_radius')] +
                [('full', PvsCsrOut), ('lig', PvsCsrOut)] +
                [(name, C.c_void_p) for name in ('inv_deg', 'node_ptr', 'node_graph', 'pos', 'keep')] +
                [('tables', PvsRaggedNodeTables), ('status', C.c_void_p)])


class PvsScreenCopiesJob(C.Structure):
    """The cropped-copies builder's job (pvs_screen_copies_build), field for field as pvs_egnn.h declares it
    (tests/test_crop_copies_host.py compares every offset with the C compiler's): a PVS_SLOTS_CROPPED job by value, then
    the crop table and the copies' rec_drop."""
    _fields_ = [('slots', PvsScreenSlotsJob), ('crop_pos', C.c_void_p), ('crop_ptr', C.c_void_p),
                ('rec_drop', C.c_void_p), ('crop_cap', C.c_int32)]


class PvsComplexPool(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in ('rec_xyz', 'lig_xyz', 'rec_types', 'lig_types', 'rec_z', 'lig_z',
                                                'rec_ptr', 'lig_ptr')] + [('n_rec', C.c_int32), ('n_lig', C.c_int32)]


class PvsHead(C.Structure):
    _fields_ = [('w', C.c_void_p), ('b', C.c_void_p), ('n_out', C.c_int32), ('act', C.c_int32), ('col', C.c_int32)]


HEAD_NONE, HEAD_RELU, HEAD_SOFTPLUS = 0, 1, 2       # PVS_HEAD_* (pvs_egnn.h)
# PVS_CAP_* (pvs_egnn.h): status bits of the capacity batch builders
CAP_NODE_OVERFLOW, CAP_GRAPH_OVERFLOW, CAP_EDGE_OVERFLOW, CAP_EMPTY_SAMPLE = 32, 64, 128, 256
MAX_POOL_HEADS = 4


class PvsStackStrides(C.Structure):
    _fields_ = [(name, C.c_int64) for name in ('h_mid', 'x_mid', 'att', 'node_att', 'saved')]


_PROTOTYPES = {
    'pvs_last_error': (C.c_char_p, []),
    'pvs_version': (C.c_int, []),
    'pvs_graph_prepare_workspace_bytes': (C.c_size_t, [C.c_int32, C.c_int32]),
    'pvs_graph_prepare': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32] +
                          [C.c_void_p] * 9 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_graph_prepare_runs_workspace_bytes': (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    'pvs_graph_prepare_runs': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] +
                               [C.c_void_p] * 11 + [C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_radius_graph_state_bytes': (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    'pvs_radius_graph_workspace_bytes': (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    'pvs_radius_graph_count': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_double, C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_radius_graph_fill': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] +
                              [C.c_void_p] * 10 + [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_graph_min_label_step': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_void_p]),
    'pvs_dropout_adj_workspace_bytes': (C.c_size_t, [C.c_int32]),
    'pvs_dropout_adj_mark': (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_uint64, C.c_uint64, C.c_void_p,
                                       C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_dropout_adj_fill': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                       C.c_void_p, C.c_void_p, C.c_void_p]),
    'pvs_dropout_key_write': (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
    'pvs_dropout_adj_mark_dev': (C.c_int, [C.c_void_p, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_size_t, C.c_void_p]),
    'pvs_dropout_adj_fill_padded': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                              C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'pvs_rows_to_input_order': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                          C.c_void_p]),
    'pvs_rows_to_sorted_order': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                           C.c_void_p]),
    'pvs_egnn_layer_saved_floats': (C.c_size_t, [C.POINTER(PvsLayerDesc), C.c_int32, C.c_int32]),
    'pvs_egnn_layer_workspace_bytes': (C.c_size_t, [C.POINTER(PvsLayerDesc), C.c_int32, C.c_int32,
                                                    C.c_int32]),
    'pvs_egnn_layer_fwd': (C.c_int, [C.POINTER(PvsLayerDesc), C.POINTER(PvsGraph),
                                     C.POINTER(PvsLayerParams)] + [C.c_void_p] * 9 +
                           [C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_screen_graph_state_bytes': (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    'pvs_screen_graph_build': (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 3 + [C.c_double, C.c_double, C.c_int32,
                                                                              C.c_int32] + [C.c_void_p] * 10 +
                               [C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_screen_slots_state_bytes': (C.c_size_t, [C.POINTER(PvsScreenSlotsJob)]),
    'pvs_screen_slots_build': (C.c_int, [C.POINTER(PvsScreenSlotsJob), C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_screen_copies_state_bytes': (C.c_size_t, [C.POINTER(PvsScreenCopiesJob)]),
    'pvs_screen_copies_build': (C.c_int, [C.POINTER(PvsScreenCopiesJob), C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_crop_keep': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_double,
                                C.c_void_p, C.c_void_p, C.c_void_p]),
    'pvs_mask_graph_workspace_bytes': (C.c_size_t, [C.c_int32, C.c_int32]),
    'pvs_mask_graph_build': (C.c_int, [C.POINTER(PvsGraph), C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32] +
                             [C.c_void_p] * 9 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_complex_batch_workspace_bytes': (C.c_size_t, [C.c_int32, C.c_int32]),
    'pvs_complex_batch_count': (C.c_int, [C.POINTER(PvsComplexPool), C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                          C.c_double, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                                          C.c_void_p]),
    'pvs_complex_batch_fill': (C.c_int, [C.POINTER(PvsComplexPool), C.c_void_p, C.c_void_p, C.c_void_p] +
                               [C.c_int32] * 6 + [C.c_void_p] * 9 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_complex_edges': (C.c_int, [C.c_int32] * 3 + [C.c_void_p] * 12),
    'pvs_complex_batch_build_cap': (C.c_int, [C.POINTER(PvsComplexPool), C.c_void_p, C.c_void_p, C.c_void_p] +
                                    [C.c_int32] * 3 + [C.c_double] + [C.c_int32] * 4 + [C.c_void_p] * 9 +
                                    [C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_radius_graph_build_cap': (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_double, C.c_double, C.c_int32,
                                                                                  C.c_int32] + [C.c_void_p] * 7 +
                                   [C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_graph_filter_workspace_bytes': (C.c_size_t, [C.c_int32]),
    'pvs_graph_filter_ligand_edges': (C.c_int, [C.POINTER(PvsGraph), C.c_void_p, C.c_int32] + [C.c_void_p] * 5 +
                                      [C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_egnn_layer_edge_sums': (C.c_int, [C.POINTER(PvsLayerDesc), C.POINTER(PvsGraph),
                                           C.POINTER(PvsLayerParams)] + [C.c_void_p] * 4 +
                                 [C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_egnn_layer_fwd_partial': (C.c_int, [C.POINTER(PvsLayerDesc), C.POINTER(PvsGraph),
                                             C.POINTER(PvsLayerParams)] + [C.c_void_p] * 9 +
                                   [C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_egnn_layer_fwd_partial_att': (C.c_int, [C.POINTER(PvsLayerDesc), C.POINTER(PvsGraph),
                                                 C.POINTER(PvsLayerParams)] + [C.c_void_p] * 10 +
                                       [C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_egnn_layer_edge_stats_softmax': (C.c_int, [C.POINTER(PvsLayerDesc), C.POINTER(PvsGraph),
                                                    C.POINTER(PvsLayerParams)] + [C.c_void_p] * 4 +
                                          [C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_egnn_layer_fwd_partial_softmax': (C.c_int, [C.POINTER(PvsLayerDesc), C.POINTER(PvsGraph),
                                                     C.POINTER(PvsLayerParams)] + [C.c_void_p] * 10 +
                                           [C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_egnn_layer_bwd':(C.c_int, [C.POINTER(PvsLayerDesc), C.POINTER(PvsGraph),
                                     C.POINTER(PvsLayerParams)] + [C.c_void_p] * 11 +
                           [C.POINTER(PvsLayerGrads), C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_egnn_stack_workspace_bytes': (C.c_size_t, [C.POINTER(PvsLayerDesc), C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    'pvs_egnn_stack_fwd': (C.c_int, [C.POINTER(PvsLayerDesc), C.POINTER(PvsLayerParams), C.c_int32, C.POINTER(PvsGraph),
                                     C.POINTER(PvsStackStrides)] + [C.c_void_p] * 9 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_egnn_stack_bwd': (C.c_int, [C.POINTER(PvsLayerDesc), C.POINTER(PvsLayerParams), C.c_int32, C.POINTER(PvsGraph),
                                     C.POINTER(PvsStackStrides)] + [C.c_void_p] * 10 +
                           [C.POINTER(PvsLayerGrads), C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_graphnorm_stats_rows_workspace_bytes': (C.c_size_t, [C.c_int32, C.c_int32]),
    'pvs_graphnorm_stats_rows': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_graphnorm_stats_segments_workspace_bytes': (C.c_size_t, [C.c_int32, C.c_int32, C.c_int32]),
    'pvs_graphnorm_stats_segments': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                               C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_linear_fwd': (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 3 + [C.c_void_p]),
    'pvs_linear_bwd_workspace_bytes': (C.c_size_t, [C.c_int32] * 3),
    'pvs_linear_bwd': (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 3 + [C.c_void_p, C.c_size_t,
                                                                      C.c_void_p]),
    'pvs_mean_pool_fwd': (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 2 + [C.c_void_p]),
    'pvs_mean_pool_bwd': (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_void_p]),
    'pvs_pool_head_fwd': (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 3 + [C.c_void_p]),
    'pvs_pool_head_bwd': (C.c_int, [C.c_void_p] * 7 + [C.c_int32] * 4 + [C.c_void_p]),
    'pvs_pool_heads_fwd': (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(PvsHead), C.c_int32, C.c_void_p, C.c_void_p] +
                           [C.c_int32] * 3 + [C.c_void_p]),
    'pvs_segment_argmax': (C.c_int, [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    'pvs_leave_out_ligand_pack': (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_void_p, C.c_int32, C.c_int32] +
                                  [C.c_void_p] * 4 + [C.c_void_p]),
    'pvs_contact_pairs_count': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                          C.c_double, C.c_void_p, C.c_void_p]),
    'pvs_contact_pairs_fill': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                         C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'pvs_leave_out_pair_pack': (C.c_int, [C.c_void_p] * 5 + [C.c_int32] * 5 + [C.c_void_p, C.c_int32, C.c_int32] +
                                [C.c_void_p] * 5 + [C.c_void_p]),
    'pvs_leave_out_parent_pack': (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 2 + [C.c_void_p, C.c_int32, C.c_int32] +
                                  [C.c_void_p] * 3 + [C.c_void_p]),
    'pvs_contact_attention': (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 2 + [C.c_void_p] * 2 + [C.c_int32] * 2 +
                              [C.c_void_p] * 5 + [C.c_void_p]),
    'pvs_node_heads_fwd': (C.c_int, [C.c_void_p, C.POINTER(PvsHead), C.c_int32, C.c_void_p] + [C.c_int32] * 3 +
                           [C.c_void_p]),
    'pvs_slot_node_values': (C.c_int, [C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p] * 2 + [C.c_int32] * 2 +
                             [C.c_void_p] * 5 + [C.c_void_p]),
    'pvs_contact_attention_cropped': (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 2 + [C.c_void_p] * 3 +
                                      [C.c_int32] * 2 + [C.c_void_p] * 5 + [C.c_void_p]),
    'pvs_slot_node_values_cropped': (C.c_int, [C.c_void_p] + [C.c_int32] * 4 + [C.c_void_p] * 3 + [C.c_int32] * 2 +
                                     [C.c_void_p] * 5 + [C.c_void_p]),
    'pvs_hit_rows_accumulate': (C.c_int, [C.c_void_p] + [C.c_int32] * 2 + [C.c_void_p] * 3 + [C.c_void_p]),
    'pvs_hit_value_ranks': (C.c_int, [C.c_void_p] + [C.c_int32] * 2 + [C.c_void_p] * 7 + [C.c_void_p]),
    'pvs_bce_logits_fwd': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    'pvs_scale_by_device_scalar': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]),
    'pvs_segment_workspace_bytes': (C.c_size_t, [C.c_int32, C.c_int32]),
    'pvs_segment_reduce_fwd': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_size_t, C.c_void_p]),
    'pvs_segment_reduce_bwd': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                         C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    'pvs_adam_clip_step': (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_float, C.c_float,
                                     C.c_double, C.c_double, C.c_float, C.c_void_p]),
    'pvs_adam_clip_step_dev': (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_float, C.c_float,
                                         C.c_void_p, C.c_float, C.c_void_p]),
    'pvs_hyper_write': (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    'pvs_adam_clip_step_hyper': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_float, C.c_void_p, C.c_float,
                                           C.c_void_p]),
    'pvs_sgd_clip_step': (C.c_int, [C.c_void_p, C.c_int32, C.c_double, C.c_double, C.c_float, C.c_int32, C.c_int32,
                                    C.c_float, C.c_void_p]),
    'pvs_sgd_clip_step_hyper': (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_int32, C.c_float, C.c_void_p]),
    # fp64 (--double)
    'pvs_egnn_layer_saved_doubles_f64': (C.c_size_t, [C.POINTER(PvsLayerDesc), C.c_int32, C.c_int32]),
    'pvs_egnn_layer_workspace_bytes_f64': (C.c_size_t, [C.POINTER(PvsLayerDesc), C.c_int32, C.c_int32, C.c_int32]),
    'pvs_egnn_layer_fwd_f64': (C.c_int, [C.POINTER(PvsLayerDesc), C.POINTER(PvsGraph), C.POINTER(PvsLayerParamsF64)] +
                               [C.c_void_p] * 9 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_egnn_layer_bwd_f64': (C.c_int, [C.POINTER(PvsLayerDesc), C.POINTER(PvsGraph), C.POINTER(PvsLayerParamsF64)] +
                               [C.c_void_p] * 11 + [C.POINTER(PvsLayerGradsF64), C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_linear_fwd_f64': (C.c_int, [C.c_void_p] * 4 + [C.c_int32] * 3 + [C.c_void_p]),
    'pvs_linear_bwd_workspace_bytes_f64': (C.c_size_t, [C.c_int32] * 3),
    'pvs_linear_bwd_f64': (C.c_int, [C.c_void_p] * 6 + [C.c_int32] * 3 + [C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_mean_pool_fwd_f64': (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 2 + [C.c_void_p]),
    'pvs_mean_pool_bwd_f64': (C.c_int, [C.c_void_p] * 3 + [C.c_int32] * 3 + [C.c_void_p]),
    'pvs_segment_workspace_bytes_f64': (C.c_size_t, [C.c_int32, C.c_int32]),
    'pvs_segment_reduce_fwd_f64': (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    'pvs_segment_reduce_bwd_f64': (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_void_p, C.c_void_p]),
    'pvs_profile_enable': (C.c_int, [C.c_int]),
    'pvs_profile_reset': (C.c_int, []),
    'pvs_profile_read': (C.c_int, [C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    'pvs_profile_read_each': (C.c_int, [C.c_char_p, C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_int64)]),
    'pvs_edge_bwd_last_variant': (C.c_int, []),
}

EXPORTED_SYMBOLS = tuple(_PROTOTYPES)
MIN_VERSION = 113       # pvs_version() of the library these prototypes describe (113: the slot builders take one job)
_lib = None


def lib():
    """The loaded library. Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise RuntimeError(
                f'{LIB_PATH} not found: build it with `python -c "import __graft_entry__ as g; '
                f'g.build()"` (or `make -C pointvs_amd/csrc`). pointvs_amd has no CPU fallback.')
        # torch FIRST: it brings its own copy of the HIP runtime (SONAME libamdhip64.so.7, like the system's one this
        # library is linked against). Loaded before torch, the library would bind the system runtime and torch its
        # bundled one - two runtimes in one process, and the streams / device state of one are nothing to the other
        # ("no ROCm-capable device is detected" from the first launch; seen when build() and smoke() ran in one process).
        import torch  # noqa: F401
        handle = C.CDLL(str(LIB_PATH))
        handle.pvs_version.restype, handle.pvs_version.argtypes = _PROTOTYPES['pvs_version']
        if handle.pvs_version() < MIN_VERSION:
            raise RuntimeError(
                f'{LIB_PATH} is version {handle.pvs_version()}, this package needs {MIN_VERSION} or newer: it was built '
                f'from older sources - rebuild it (`python -c "import __graft_entry__ as g; g.build()"` or '
                f'`make -C pointvs_amd/csrc`)')
        for name, (restype, argtypes) in _PROTOTYPES.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = restype, argtypes
        _lib = handle
    return _lib


def check(rc, what):
    if rc != 0:
        msg = lib().pvs_last_error().decode(errors='replace')
        raise RuntimeError(f'{what} failed ({rc}): {msg}')


def ptr(t):
    """Device pointer of a tensor (None -> NULL). The tensor must be contiguous."""
    if t is None:
        return None
    if not t.is_contiguous():
        raise ValueError('non-contiguous tensor handed to the C ABI')
    return t.data_ptr()


def require_hip(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                'pointvs_amd kernels run on a HIP device only (got a CPU tensor); there is no CPU '
                'path in the product - the CPU oracle lives in oracle/ and is test-only')


def stream(dev):
    """Raw handle (hipStream_t as an int) of torch's CURRENT stream on `dev`, as every C-ABI call takes it. The raw
    accessor, not torch.cuda.current_stream(dev).cuda_stream: that builds a Stream object (5 us a call on the host, a
    dozen calls per training step of a small batch)."""
    import torch
    idx = dev.index
    if idx is None:
        idx = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(idx)

