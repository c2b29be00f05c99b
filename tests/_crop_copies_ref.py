"""Numpy reference of cropped copies (pvs_screen_copies_build, pvs_crop_keep, pvs_leave_out_parent_pack;
LibraryScreen(crop_parents=True)), built on tests/_crop_ref.py: the keep mask of a slot that is cropped around OTHER atoms
than its own (a leave-out copy's parent) with one receptor atom struck, the copy's complex, the parent packer's layout
and the packed hits' kept counts. Pure host code; tests/test_crop_copies_host.py pins the decisions against scipy's
cdist."""
import numpy as np

from tests import _crop_ref as ref


def keep_mask(parent_pos, rec_pos, radius, rec_drop=-1):
    """[n_rec] bool: receptor atom j is kept iff some atom of `parent_pos` (what the slot is cropped AROUND) is closer
    than `radius` (tests/_crop_ref.keep_mask: fp64, strict, no lower bound, an empty set keeps nothing) and j is not
    rec_drop (-1: none). A rec_drop that the crop does not keep changes nothing."""
    mask = ref.keep_mask(parent_pos, rec_pos, radius).copy()
    if rec_drop >= 0:
        mask[rec_drop] = False
    return mask


def copy_complex(lig_feats, lig_pos, rec_feats, rec_pos, radius, skip=-1, rec_drop=-1, parent_pos=None):
    """(x, pos, kept) of one copy of a hit: the hit's ligand atoms without atom `skip` (-1: all of them), then the
    receptor atoms that the crop around the WHOLE hit (parent_pos; None: lig_pos, the hit itself) keeps, without
    rec_drop, in receptor order."""
    lig_feats, lig_pos = np.asarray(lig_feats), np.asarray(lig_pos).reshape(-1, 3)
    parent = lig_pos if parent_pos is None else np.asarray(parent_pos).reshape(-1, 3)
    kept = np.flatnonzero(keep_mask(parent, rec_pos, radius, rec_drop))
    rows = [a for a in range(lig_pos.shape[0]) if a != skip]
    x = np.concatenate([lig_feats[rows], np.asarray(rec_feats)[kept]], axis=0)
    pos = np.concatenate([lig_pos[rows], np.asarray(rec_pos)[kept]], axis=0)
    return x, pos, kept


def recropped_complex(lig_feats, lig_pos, rec_feats, rec_pos, radius, skip=-1, rec_drop=-1):
    """The WRONG copy: cropped again around what is left of the ligand (what a plain cropped slot would do)."""
    lig_pos = np.asarray(lig_pos).reshape(-1, 3)
    rows = [a for a in range(lig_pos.shape[0]) if a != skip]
    return copy_complex(lig_feats, lig_pos, rec_feats, rec_pos, radius, skip, rec_drop, parent_pos=lig_pos[rows])


def copy_hits(copy_ptr, first_copy, n_slots):
    """Per slot the hit that owns copy first_copy + k when hit s owns the copies copy_ptr[s] + s .. copy_ptr[s + 1] + s
    (both ends included); -1 for a copy number that is no copy."""
    copy_ptr = [int(v) for v in copy_ptr]
    n_hits = len(copy_ptr) - 1
    owner = [s for s in range(n_hits) for _ in range(copy_ptr[s + 1] - copy_ptr[s] + 1)]
    return [owner[c] if 0 <= c < len(owner) else -1 for c in range(int(first_copy), int(first_copy) + n_slots)]


def parent_pack(lig_pos, lig_ptr, copy_ptr, first_copy, n_slots):
    """(out_pos [sum, 3], out_ptr [n_slots + 1]) of pvs_leave_out_parent_pack: slot k gets the WHOLE hit behind copy
    first_copy + k, nothing for a copy number that is no copy."""
    lig_pos = np.asarray(lig_pos, dtype=np.float32).reshape(-1, 3)
    rows, ptr = [], [0]
    for hit in copy_hits(copy_ptr, first_copy, n_slots):
        if hit >= 0:
            rows.append(lig_pos[int(lig_ptr[hit]):int(lig_ptr[hit + 1])])
        ptr.append(ptr[-1] + (rows[-1].shape[0] if hit >= 0 else 0))
    out = np.concatenate(rows, axis=0) if rows else np.zeros((0, 3), dtype=np.float32)
    return out, np.asarray(ptr, dtype=np.int32)


def hits_keep(lig_pos, lig_ptr, rec_pos, radius):
    """(keep words [n_hits, W] uint64, kept_ptr [n_hits + 1] int32) of pvs_crop_keep."""
    lig_pos = np.asarray(lig_pos).reshape(-1, 3)
    masks = [ref.keep_mask(lig_pos[int(lig_ptr[s]):int(lig_ptr[s + 1])], rec_pos, radius)
             for s in range(len(lig_ptr) - 1)]
    n_words = (np.asarray(rec_pos).reshape(-1, 3).shape[0] + 63) // 64
    words = np.stack([ref.mask_words(m) for m in masks]) if masks else np.zeros((0, n_words), dtype=np.uint64)
    ptr = np.concatenate([[0], np.cumsum([int(m.sum()) for m in masks])]).astype(np.int32)
    return words, ptr
