"""Host reference of the fixed-shape edge dropout (pvs_dropout_adj_fill_padded), numpy only, built on dropout_adj_ref.

Layout: out_index [2, cap], out_attr [cap, A]. The first 2K columns are dropout_adj_ref's list (K survivors, then their
reverses). Slot j in [2K, cap) is a padding edge: d = j - 2K, pair k = (d // 2) mod (n_pad // 2), a = N + 2k, b = a + 1;
even d holds (a, b), odd d holds (b, a); its attribute row is one-hot class 0.
"""
import numpy as np

from tests._dropout_ref import dropout_adj_ref


def half_count(edge_index):
    """Number of row <= col edges: the candidates of the draw (a self-loop is one)."""
    edge_index = np.asarray(edge_index)
    return int((edge_index[0] <= edge_index[1]).sum())


def dropout_adj_padded_ref(edge_index, edge_attr, p, seed, step, cap, n_nodes, n_pad):
    """(out_index [2, cap], out_attr [cap, A] or None, K)."""
    assert cap % 2 == 0 and n_pad >= 2 and n_pad % 2 == 0
    drawn_i, drawn_a = dropout_adj_ref(edge_index, edge_attr, p, seed, step)
    two_k = drawn_i.shape[1]
    assert two_k <= cap, 'the capacity does not hold the draw'
    d = np.arange(cap - two_k, dtype=np.int64)
    a = n_nodes + 2 * ((d // 2) % (n_pad // 2))
    b = a + 1
    odd = (d % 2).astype(bool)
    pad = np.stack([np.where(odd, b, a), np.where(odd, a, b)])
    out_index = np.concatenate([drawn_i, pad], axis=1).astype(np.int64)
    if edge_attr is None:
        return out_index, None, two_k // 2
    width = np.asarray(edge_attr).shape[1]
    pad_attr = np.zeros((cap - two_k, width), dtype=np.int64)
    if width:
        pad_attr[:, 0] = 1
    return out_index, np.concatenate([drawn_a, pad_attr]).astype(np.int64), two_k // 2
