"""Host reference of the edge dropout (pointvs_amd/csrc/dropout_adj.hip), numpy only.

The draw is counter-based and integer: Philox4x32-10 with counter (edge id, step) and key seed, the first output word's
top 24 bits as a float32 in [0, 1). Every output element of PF.dropout_adj is therefore predicted exactly.
"""
import numpy as np

M32 = np.uint64(0xFFFFFFFF)
PHILOX_M0, PHILOX_M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
PHILOX_W0, PHILOX_W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
S32 = np.uint64(32)

# (seed, step) pairs of the host and the GPU tests: full 64-bit values, and pairs that differ in ONE 32-bit half only
SEED_STEPS = [(5, 1), (2 ** 64 - 1, 2 ** 63 + 12345), (0x9E3779B97F4A7C15, 7 << 32), (7, 7), (7, 7 + 2 ** 32),
              (7 + 2 ** 32, 7)]
# found by a host search over steps: counter ZERO_DRAW[2] has the 24-bit value 0, counter MAX_DRAW[2] the value
# 2**24 - 1 (tests/test_dropout_ref_host.py checks both)
ZERO_DRAW = (7 + 2 ** 32, (3 << 32) + 104711, 196)
MAX_DRAW = (7 + 2 ** 32, (3 << 32) + 57479, 65)


def philox4x32_10(counter4, key2):
    """Philox4x32-10 over arrays of 32-bit words held in uint64: counter4 = (c0, c1, c2, c3), key2 = (k0, k1), each a
    scalar or an array (broadcast). Returns the four output words as uint64 arrays."""
    c0, c1, c2, c3 = np.broadcast_arrays(*(np.asarray(c, dtype=np.uint64) & M32 for c in counter4))
    k0, k1 = (np.asarray(k, dtype=np.uint64) & M32 for k in key2)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ k0, p1 & M32, (p0 >> S32) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + PHILOX_W0) & M32, (k1 + PHILOX_W1) & M32
    return c0, c1, c2, c3


def uniform24(seed, step, e):
    """float32 in [0, 1 - 2**-24] of counter `e` (an int or an integer array) under the 64-bit (seed, step)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    e = np.asarray(e, dtype=np.uint64)
    word0 = philox4x32_10((e & M32, e >> S32, step & 0xFFFFFFFF, step >> 32), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return (word0 >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def dropout_adj_ref(edge_index, edge_attr, p, seed, step):
    """torch_geometric's dropout_adj(force_undirected=True) on this library's stream: edge e survives iff
    row[e] <= col[e] and uniform24(seed, step, e) >= float32(p); the survivors in input order, then their reverses,
    attribute rows repeated. int64 arrays in, int64 arrays out: ([2, 2K], [2K, A] or None)."""
    edge_index = np.asarray(edge_index, dtype=np.int64)
    row, col = edge_index[0], edge_index[1]
    keep = (row <= col) & (uniform24(seed, step, np.arange(row.size)) >= np.float32(p))
    out_index = np.stack([np.concatenate([row[keep], col[keep]]), np.concatenate([col[keep], row[keep]])])
    if edge_attr is None:
        return out_index, None
    edge_attr = np.asarray(edge_attr, dtype=np.int64)
    return out_index, np.concatenate([edge_attr[keep], edge_attr[keep]])
