"""The cases and references of tests/_many_slots_cases.py, pinned on the host (CPU): where the special sizes sit, the
prefix property, that no ligand-receptor distance is near a radius the GPU tests use, that every count has slots with
and without contacts and crops from nothing to the whole receptor, and that the references agree with each other where
two routes lead to the same arrays and with the small-count references of the existing tests."""
import numpy as np
import pytest

from tests import _crop_copies_ref as cref
from tests import _crop_ref as ref
from tests import _many_slots_cases as mc
from tests._attribution_ref import AttrCase


def test_sizes_land_at_the_promised_positions():
    assert mc.COUNTS == (65, 255, 256, 257, 513)
    for b in mc.COUNTS:
        sizes = mc.slot_sizes(b)
        assert len(sizes) == b
        for p in (0, 63, 64, 255, 256, b - 1):
            if p < b:
                assert sizes[p] == 0, (b, p)
        for p, n in ((1, 64), (65, 65), (257, 130)):
            if p < b - 1:
                assert sizes[p] == n, (b, p)
        rest = [n for p, n in enumerate(sizes) if p not in (0, 63, 64, 255, 256, b - 1, 1, 65, 257)]
        assert set(rest) == {1, 2, 3, 4, 5} and max(sizes) <= mc.SLOT_CAP
    assert 130 in mc.slot_sizes(513) and 65 in mc.slot_sizes(255) and 65 not in mc.slot_sizes(65)
    # the hit tables of the packers and listers: empty hits at the ends, at 255 / 256 and in the middle
    for s in (257, 513):
        sizes = mc.hit_sizes(s)
        assert [sizes[h] for h in (0, 50, 255, 256, s - 1)] == [0] * 5 and sizes[3] == 9 and max(sizes) == 9
        pairs = mc.hit_pairs(sizes, mc.N_REC)
        assert all(not hit for hit, n in zip(pairs, sizes) if n == 0) and max(len(hit) for hit in pairs) == 3
        flat = [p for hit in pairs for p in hit]
        assert any(a == -1 for a, _ in flat) and any(r == -1 for _, r in flat) and any(r == mc.N_REC - 1 for _, r in flat)
        assert all(-1 <= a < n and -1 <= r < mc.N_REC for hit, n in zip(pairs, sizes) for a, r in hit)
        assert all(not (a == -1 and r == -1) for a, r in flat)


def test_prefix_property():
    big = mc.slots(513)
    for b in mc.COUNTS[:-1]:
        small = mc.slots(b)
        for p in range(b - 1):
            assert all(np.array_equal(x, y) for x, y in zip(small[p], big[p])), (b, p)
        assert small[b - 1][1].shape == (0, 3) and small[b - 1][0].shape == (0, mc.F)
    rec, rec_feats = mc.receptor()
    assert rec.shape == (mc.N_REC, 3) and rec.dtype == np.float32 and bool((rec_feats[:, -1] == 1).all())
    assert all(bool((f[:, -1] == 0).all()) and f.dtype == np.float32 and q.dtype == np.float32 for f, q in big)


def test_no_distance_in_the_excluded_band_and_every_count_has_both_kinds_of_slot():
    rec, _ = mc.receptor()
    crop = mc.RADII[1]
    for b in mc.COUNTS:
        with_contact = without = 0
        kept = set()
        for _, pose in mc.slots(b):
            d = mc.distances(pose, rec)
            for radius in mc.RADII:
                assert not (np.abs(d - radius) <= mc.BAND).any()
            assert not (d <= 1e-6).any()
            kept.add(int((d < crop).any(0).sum()) if len(pose) else 0)
            if len(pose):
                with_contact += bool((d < 4.0).any())
                without += not (d < 4.0).any()
        assert without >= 1 and with_contact >= 20, (b, without, with_contact)
        assert 0 in kept and mc.N_REC in kept and any(0 < k < mc.N_REC for k in kept), (b, sorted(kept))
    for s in mc.COUNTS:                                         # the listers' hits: the same atoms, and the far hit
        for swap in (False, True):
            pos, ptr = mc.lister_hits(s, swap)
            d = mc.distances(pos, rec)
            assert not any((np.abs(d - radius) <= mc.BAND).any() for radius in mc.RADII)
            n = np.diff(ptr)
            hits_d = [d[ptr[h]:ptr[h + 1]] for h in range(s)]
            for h in (0, 255, 256, s - 1):
                if h < s:
                    assert n[h] == 0 or not (hits_d[h] < 7.0).any(), (s, h)
            assert ptr[-1] == len(pos) and sum(bool((x < 4.0).any()) for x in hits_d) >= 20
        assert {int(mc.lister_hits(s)[1][1]), int(mc.lister_hits(s, True)[1][1])} == {0, 3}


def test_contact_list_equals_the_fixtures_unique_pairs_and_the_class_1_edges():
    """What tests/test_gpu_struck_slots.py asks of PF.contact_pairs on the reference's fixture, asked of the brute-force
    list; and per slot the list is the class-1 edges out of ligand rows of the oracle's edge list."""
    c = AttrCase('attr_dimout3_ball120')
    d = c.drop_table()
    _, first = np.unique(d[:, 0] * c.n + d[:, 1], return_index=True)
    want = d[first] - np.array([0, 12])
    pairs, ptr = mc.contact_list(c.pos[:12].numpy(), [0, 12], c.pos[12:].numpy(), 4.0)
    assert ptr.tolist() == [0, 85] and np.array_equal(pairs, want)
    rec, _ = mc.receptor()
    slots = mc.slots(65)
    pos = np.concatenate([pose for _, pose in slots])
    lig_ptr = np.concatenate([[0], np.cumsum([len(pose) for _, pose in slots])])
    pairs, ptr = mc.contact_list(pos, lig_ptr, rec, 4.0)
    for p, ((ei, et), (_, pose)) in enumerate(zip(mc.slot_edges(65, 4.0), slots)):
        m = (et == 1) & (ei[0] < len(pose))
        assert np.array_equal(pairs[ptr[p]:ptr[p + 1]], np.stack([ei[0][m], ei[1][m] - len(pose)], 1)), p
    assert ptr[-1] > 200 and pairs.dtype == np.int32


def _sums(k=8):
    """Stand-ins for the screen's receptor sums: distinct numbers per receptor atom."""
    j = np.arange(mc.N_REC, dtype=np.float32)
    return (j[:, None] * 100 + np.arange(k, dtype=np.float32) + 1, j[:, None] * 10 + np.arange(3, dtype=np.float32) + 0.5,
            j + 0.25)


def test_two_routes_to_the_same_batch_agree():
    """On the 65-slot batch: the unstruck slot_batch is the cropped_batch of a crop that drops nothing; a struck slot's
    full CSR is the oracle's edge list of the complex WITHOUT the atom (not the masking of the whole one); a slot's
    ligand-touching CSR is the full one's edges with a ligand end; the cropped masks are cref.hits_keep's."""
    b, radius = 65, 4.0
    rec, rec_feats = mc.receptor()
    slots, edges = mc.slots(b), mc.slot_edges(b, radius)
    n_cap = b * (mc.SLOT_CAP + mc.N_REC)
    plain = mc.slot_batch(edges, slots, [-1] * b, rec, rec_feats, _sums(), n_cap)
    full = [p for p in range(b) if len(slots[p][1])]            # (an empty slot keeps nothing, whatever the radius)
    some = mc.slot_batch([edges[p] for p in full], [slots[p] for p in full], [-1] * len(full), rec, rec_feats, _sums(), n_cap)
    whole = mc.cropped_batch([slots[p] for p in full], rec, rec_feats, 1e6, radius, n_cap)
    for k in ('rowptr', 'row', 'col', 'etype', 'inv_deg', 'node_ptr', 'node_graph', 'pos', 'x'):
        assert some[k].dtype == whole[k].dtype and some[k].tobytes() == whole[k].tobytes(), k
    assert len(full) == b - 3 and len(some['row']) > 50000          # (slots 0, 63 and 64, the last)
    assert plain['node_ptr'][-1] == sum(len(p) for _, p in slots) + b * mc.N_REC and len(plain['row']) > 50000
    lig_rows = np.zeros(n_cap, dtype=bool)
    for p, (_, pose) in enumerate(slots):
        lig_rows[plain['node_ptr'][p]:plain['node_ptr'][p] + len(pose)] = True
    m = lig_rows[plain['row']] | lig_rows[plain['col']]
    assert np.array_equal(plain['row_l'], plain['row'][m]) and np.array_equal(plain['col_l'], plain['col'][m])
    assert bool((plain['base_deg'][~lig_rows][:b * mc.N_REC] > 0).all()) and not plain['base_deg'][lig_rows].any()
    # struck: atoms 0, n_rec - 1, 17 and none, slot by slot
    drops = [(-1, 0, mc.N_REC - 1, 17)[p % 4] for p in range(b)]
    struck = mc.slot_batch(edges, slots, drops, rec, rec_feats, _sums(), n_cap)
    assert struck['node_ptr'][-1] == plain['node_ptr'][-1] - sum(r >= 0 for r in drops)
    for p, ((feats, pose), r) in enumerate(zip(slots, drops)):
        keep = [j for j in range(mc.N_REC) if j != r]
        ei, et = mc.complex_edges(np.concatenate([pose, rec[keep]]), np.concatenate([np.zeros(len(pose)), np.ones(len(keep))]),
                                  radius)
        n0, n1 = struck['node_ptr'][p], struck['node_ptr'][p + 1]
        lo, hi = struck['rowptr'][n0], struck['rowptr'][n1]
        assert n1 - n0 == len(pose) + len(keep) and hi - lo == ei.shape[1], p
        assert np.array_equal(struck['row'][lo:hi], ei[0] + n0) and np.array_equal(struck['col'][lo:hi], ei[1] + n0), p
        assert np.array_equal(struck['etype'][lo:hi], et), p
        assert np.array_equal(struck['pos'][n0:n1], np.concatenate([pose, rec[keep]])), p
    assert len(struck['row_l']) > len(plain['row_l']) and len(struck['row']) < len(plain['row'])
    # cropped: the masks and ranks against cref.hits_keep and the rank table
    crop = mc.RADII[1]
    cropped = mc.cropped_batch(slots, rec, rec_feats, crop, radius, n_cap)
    pos = np.concatenate([pose for _, pose in slots])
    lig_ptr = np.concatenate([[0], np.cumsum([len(pose) for _, pose in slots])])
    words, kept_ptr = cref.hits_keep(pos, lig_ptr, rec, crop)
    assert np.array_equal(cropped['keep'], words) and np.array_equal(cropped['keep_rank'][:, -1], np.diff(kept_ptr))
    assert cropped['node_ptr'][-1] == lig_ptr[-1] + kept_ptr[-1] < plain['node_ptr'][-1]
    for p in (1, 2, 7):
        mask = ref.words_mask(cropped['keep'][p], mc.N_REC)
        assert cropped['keep_rank'][p].tolist() == [0, int(mask[:64].sum()), int(mask.sum())]
    # copies: a slot cropped around a parent that is not itself, without one receptor atom
    parents = [slots[(p + 1) % b][1] for p in range(b)]
    copies = mc.cropped_batch(slots, rec, rec_feats, crop, radius, n_cap, parents=parents, rec_drop=drops)
    for p in range(b):
        mask = ref.keep_mask(parents[p], rec, crop)
        if drops[p] >= 0:
            mask[drops[p]] = False
        assert np.array_equal(ref.words_mask(copies['keep'][p], mc.N_REC), mask), p
    assert not np.array_equal(copies['keep'], cropped['keep'])


def test_packed_batches_agree_with_the_plan_and_the_parent_packer():
    """On the hit table the existing packer tests use: the copies' sizes are leave_out_plan's, a batch's out_ptr that of
    the plan's sizes; on a 257-hit table the pair copies' owners are cref.copy_hits' and their count pair_ptr's."""
    from pointvs_amd.screening import leave_out_pair_plan, leave_out_plan
    sizes = [0, 1, 2, 5, 64, 65, 130]
    pos, feats, ptr = mc.ligands(sizes)
    copies = mc.ligand_copies(pos, feats, ptr)
    assert len(copies) == sum(sizes) + len(sizes) == 274
    flat = [n for batch in leave_out_plan(sizes, 7) for n in batch]
    assert flat[:274] == [len(c[0]) for c in copies]
    for first in (0, 35, 270, 280):
        got = mc.packed_batch(copies, first, 7, 130)
        assert np.diff(got[2]).tolist() == (flat + [0] * 20)[first:first + 7] and bool((got[3] == -1).all())
        assert bool((got[0][got[2][-1]:] == -7.0).all()) and not (got[0][:got[2][-1]] == -7.0).any()
    sizes = mc.hit_sizes(257)
    pairs = mc.hit_pairs(sizes, mc.N_REC)
    pos, feats, ptr = mc.ligands(sizes)
    table, pair_ptr = mc.pair_table(pairs)
    copies = mc.pair_copies(pos, feats, ptr, pairs)
    assert len(copies) == pair_ptr[-1] + 257 == len(table) + 257
    # (leave_out_pair_plan sizes tables whose every pair names a ligand atom: those copies)
    named = [[(a, r) for a, r in hit if a >= 0] for hit in pairs]
    plan = leave_out_pair_plan([len(hit) for hit in named], sizes, 65)
    named_copies = mc.pair_copies(pos, feats, ptr, named)
    assert [n for batch, _ in plan for n in batch][:len(named_copies)] == [len(c[0]) for c in named_copies]
    for first in (0, 130, len(copies) - 3):
        owners = cref.copy_hits(pair_ptr, first, 65)
        got = mc.packed_batch(copies, first, 65, 9)
        assert np.diff(got[2]).tolist() == [0 if h < 0 else len(copies[first + k][0]) for k, h in enumerate(owners)]
        parent_pos, parent_ptr = cref.parent_pack(pos, ptr, pair_ptr, first, 65)
        assert np.diff(parent_ptr).tolist() == [0 if h < 0 else sizes[h] for h in owners]
        assert all(parent_ptr[k + 1] - parent_ptr[k] - (got[2][k + 1] - got[2][k])
                   == (0 if h < 0 else int(copies[first + k][0].shape[0] < sizes[h])) for k, h in enumerate(owners))
    with pytest.raises(ValueError):
        leave_out_plan(sizes, 0)
