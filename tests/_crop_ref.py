"""Numpy reference of the cropped pose-batch slots (pvs_screen_slots_build with PVS_SLOTS_CROPPED, LibraryScreen(crop_radius=...)):
which receptor atoms a slot keeps, the keep mask's 64-bit words and their rank table, and the cropped complex that the
slot's graph is generate_edges of. Pure host code; tests/test_screen_crop_host.py pins the keep decision against scipy's
cdist."""
import numpy as np


def keep_mask(lig_pos, rec_pos, radius):
    """[n_rec] bool: receptor atom j is kept iff some ligand atom is closer than `radius` - strict, no lower bound (a
    coincident atom is kept), no ligand atom: nothing kept. Decided in fp64 on the coordinates as given (fp32 inputs are
    widened exactly), the squares summed in index order and the root taken, as scipy's euclidean cdist does."""
    lig = np.asarray(lig_pos).astype(np.float64).reshape(-1, 3)
    rec = np.asarray(rec_pos).astype(np.float64).reshape(-1, 3)
    if lig.shape[0] == 0:
        return np.zeros(rec.shape[0], dtype=bool)
    d = lig[:, None, :] - rec[None, :, :]
    s = d[..., 0] * d[..., 0]
    s = s + d[..., 1] * d[..., 1]
    s = s + d[..., 2] * d[..., 2]
    return (np.sqrt(s) < float(radius)).any(axis=0)


def mask_words(mask):
    """The mask as ceil(n / 64) uint64 words: atom j is bit j % 64 of word j / 64; the bits from n on are clear."""
    mask = np.asarray(mask, dtype=bool)
    n_words = (len(mask) + 63) // 64
    bits = np.zeros(64 * n_words, dtype=np.uint64)
    bits[:len(mask)] = mask
    return (bits.reshape(n_words, 64) << np.arange(64, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


def words_mask(words, n):
    """mask_words backwards: [n] bool."""
    words = np.asarray(words).astype(np.uint64).reshape(-1)
    return (((words[:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)) != 0).reshape(-1)[:n]


def rank_table(mask):
    """[W + 1] int: the kept atoms in the words before word w; entry W is the kept count."""
    mask = np.asarray(mask, dtype=bool)
    n_words = (len(mask) + 63) // 64
    padded = np.zeros(64 * n_words, dtype=np.int64)
    padded[:len(mask)] = mask
    return np.concatenate([[0], np.cumsum(padded.reshape(n_words, 64).sum(axis=1))])


def cropped_complex(lig_feats, lig_pos, rec_feats, rec_pos, radius):
    """(x, pos, kept): the slot's rows - the ligand atoms, then the kept receptor atoms in receptor order - and the
    kept atoms' receptor indices."""
    kept = np.flatnonzero(keep_mask(lig_pos, rec_pos, radius))
    x = np.concatenate([np.asarray(lig_feats), np.asarray(rec_feats)[kept]], axis=0)
    pos = np.concatenate([np.asarray(lig_pos).reshape(-1, 3), np.asarray(rec_pos)[kept]], axis=0)
    return x, pos, kept
