"""Struck slots, the device side: the pose-batch builder for slots whose receptor lacks one atom
(pvs_screen_slots_build with PVS_SLOTS_STRUCK, through LibraryScreen(struck=True)), the contact lister (PF.contact_pairs) and the pair
packer (PF.leave_out_pair_pack). All three are integer work or copies: every array is compared for equality - the
builder with the existing ragged builder's output for the same slots after the numpy masking of the reference
(tests/_attribution_ref.masked_coo: drop the atom, drop its edges, shift the ids above it), the lister with the class-1
edges of that builder, the packer with a numpy construction over integer-named rows."""
import numpy as np
import pytest
import torch

from tests import _many_slots_cases as mc
from tests._attribution_ref import AttrCase
from tests.test_gpu_ligand_masking import N_REC, _set, _single_head

pytestmark = pytest.mark.gpu

SLOT_SIZES = [0, 1, 5, 64, 65, 130]
B = len(SLOT_SIZES)


# ---------------------------------------------------------------- the builder

_CACHE = {}


def _case():
    """The synthetic receptor of 150 atoms, one pose per slot size, and a model whose first layer the screens reuse."""
    if 'case' not in _CACHE:
        from pointvs_amd.synthetic import random_poses
        lig, rec, lig_feats, rec_feats = _set(8201, 130)
        slots = []
        for k, n in enumerate(SLOT_SIZES):
            pose = random_poses(lig[:max(n, 1)], 1, seed=500 + k, max_shift=3.0)[0][:n].contiguous()
            slots.append((lig_feats[:n].roll(k, 0).contiguous(), pose))
        _CACHE['case'] = (slots, rec, rec_feats, _single_head(21))
    return _CACHE['case']


def _screen(radius, struck):
    from pointvs_amd.screening import LibraryScreen
    slots, rec, rec_feats, model = _case()
    return LibraryScreen(model, rec.cuda(), rec_feats, B, 130, radius, struck=struck)


def _np(f, screen):
    """The builder's outputs as numpy, the edge arrays cut at their device-side counts."""
    torch.cuda.synchronize()
    out = {k: f[k].cpu().numpy() for k in ('rowptr', 'rowptr_l', 'inv_deg', 'node_ptr', 'node_graph', 'pos', 'x',
                                           'base_magg', 'base_xsum', 'base_deg', 'status')}
    for tag in ('', '_l'):
        e = int(out['rowptr' + tag][screen.n_cap])
        for k in ('row', 'col', 'etype'):
            out[k + tag] = f[k + tag][:e].cpu().numpy()
    return out


def _plain(radius):
    """The ragged builder's output for the whole slots (the yardstick), once per radius."""
    if ('plain', radius) not in _CACHE:
        screen = _screen(radius, None)
        f = screen.load(_case()[0])._build()
        screen.check()
        out = _np(f, screen)
        out['sums'] = tuple(t.cpu().numpy() for t in (screen.rec_magg, screen.rec_xsum, screen.rec_deg))
        _CACHE['plain', radius] = out
    return _CACHE['plain', radius]


def _slot_edges(g, p):
    """Slot p of a built batch: (edge_index [2, E] in slot-local ids, etype [E]) in CSR order."""
    n0, n1 = int(g['node_ptr'][p]), int(g['node_ptr'][p + 1])
    e0, e1 = int(g['rowptr'][n0]), int(g['rowptr'][n1])
    return np.stack([g['row'][e0:e1], g['col'][e0:e1]]).astype(np.int64) - n0, g['etype'][e0:e1]


def _kinds(radius):
    """Per slot: a receptor atom with ligand contacts (-1 when the slot has none) and one without ligand contacts but
    with template neighbours."""
    g = _plain(radius)
    with_contact, without = [], []
    for p, n in enumerate(SLOT_SIZES):
        ei, et = _slot_edges(g, p)
        touched_by_ligand = set((ei[1][(ei[0] < n) & (ei[1] >= n)] - n).tolist())
        has_rr = set((ei[0][et == 2] - n).tolist())
        with_contact.append(min(touched_by_ligand) if touched_by_ligand else -1)
        free = sorted(has_rr - touched_by_ligand)
        without.append(free[len(free) // 2] if free else -1)
    return with_contact, without


def _rec_drops(radius):
    """Three tables that between them give every slot size each kind of entry: -1, atom 0, atom n_rec - 1, an atom with
    ligand contacts, an atom without ligand contacts but with template neighbours."""
    with_contact, without = _kinds(radius)
    # (the empty slot has no contact and a slot may touch every receptor atom: such a slot takes the other kind)
    assert with_contact[0] == -1 and without[0] >= 0 and sum(r >= 0 for r in with_contact) >= 3
    assert sum(r >= 0 for r in without) >= 3
    tables = []
    for rot in (0, 2, 4):
        table = []
        for p in range(B):
            kind = ('whole', 'first', 'last', 'contact', 'free', 'contact')[(p + rot) % 6]
            r = {'whole': -1, 'first': 0, 'last': N_REC - 1,
                 'free': without[p] if without[p] >= 0 else with_contact[p],
                 'contact': with_contact[p] if with_contact[p] >= 0 else without[p]}[kind]
            table.append(int(r))
        tables.append(table)
    return tables


def _expected(radius, rec_drop):
    """What the struck builder must write, from the ragged builder's output and the reference's masking per slot."""
    g = _plain(radius)
    slots, rec, rec_feats, _ = _case()
    return mc.slot_batch([_slot_edges(g, p) for p in range(B)], [(f.numpy(), pose.numpy()) for f, pose in slots], rec_drop,
                         rec.numpy(), rec_feats.numpy(), g['sums'], len(g['node_graph']))


def _struck_build(radius, rec_drop, capacities=None):
    screen = _screen(radius, True)
    screen.load(_case()[0])._build()                 # sized as every screen is: from the whole slots
    screen.check()
    if capacities is not None:
        screen._fast = None
    f = screen.load(_case()[0], rec_drop=rec_drop)._build(capacities)
    return screen, f


@pytest.mark.parametrize('radius', [7.0, 4.0])
def test_builder_is_exact(radius):
    g = _plain(radius)
    for rec_drop in _rec_drops(radius):
        screen, f = _struck_build(radius, rec_drop)
        screen.check()
        got = _np(f, screen)
        want = _expected(radius, rec_drop)
        assert got['status'][0] == 0
        n_struck = sum(r >= 0 for r in rec_drop)
        assert want['node_ptr'][-1] == g['node_ptr'][-1] - n_struck and n_struck >= 4
        assert len(want['row']) < len(g['row']) and len(want['row_l']) > len(g['row_l'])     # (edges go; whole rows come)
        for k, w in want.items():
            assert got[k].dtype == w.dtype and got[k].tobytes() == w.tobytes(), (radius, rec_drop, k)
        # two runs write the same bytes
        again = _np(screen.load(_case()[0], rec_drop=rec_drop)._build(), screen)
        assert all(again[k].tobytes() == got[k].tobytes() for k in got)


@pytest.mark.parametrize('radius', [7.0, 4.0])
def test_unstruck_table_writes_what_the_ragged_builder_writes(radius):
    g = _plain(radius)
    screen, f = _struck_build(radius, [-1] * B)
    screen.check()
    got = _np(f, screen)
    for k in got:
        assert got[k].tobytes() == g[k].tobytes(), k
    assert len(g['row']) > 0 and len(g['row_l']) > 0


def test_bad_rec_drop_and_too_little_room():
    radius = 4.0
    for bad in (N_REC, -2):
        screen, f = _struck_build(radius, [-1] * B)
        screen.check()
        screen.rec_drop[3] = bad                      # (load() refuses such a list on the host: straight into the table)
        f = screen._build()
        got = _np(f, screen)
        assert got['status'][0] & 8 and not got['rowptr'].any() and not got['rowptr_l'].any(), bad
        assert len(got['row']) == 0 and (got['node_graph'] == -1).all() and (got['inv_deg'] == 1).all()
        with pytest.raises(ValueError, match='rec_drop'):
            screen.check()
    with pytest.raises(ValueError, match='rec_drop'):
        _screen(radius, True).load(_case()[0], rec_drop=[-1] * (B - 1) + [N_REC])
    with pytest.raises(ValueError, match='struck=True'):
        _screen(radius, None).load(_case()[0], rec_drop=[-1] * B)
    # the ligand-touching room of the unstruck batch does not hold the touched rows: bit 2, nothing written past it
    g = _plain(radius)
    rec_drop = _rec_drops(radius)[0]
    screen, f = _struck_build(radius, rec_drop, capacities=(len(g['row']), len(g['row_l'])))
    assert int(f['status'].item()) & 4
    with pytest.raises(RuntimeError, match='overflow'):
        screen.check()


# ---------------------------------------------------------------- the contact list

def _class1(g, sizes):
    """(pairs [K, 2], pair_ptr) of a built batch's class-1 edges out of ligand rows, slot by slot."""
    pairs, ptr = [], [0]
    for p, n in enumerate(sizes):
        ei, et = _slot_edges(g, p)
        m = (et == 1) & (ei[0] < n)
        pairs.append(np.stack([ei[0][m], ei[1][m] - n], 1))
        ptr.append(ptr[-1] + int(m.sum()))
    return np.concatenate(pairs).astype(np.int32), np.array(ptr, np.int32)


def _contact_pairs(slots, rec, radius):
    from pointvs_amd import functional as PF
    sizes = [int(p.shape[0]) for _, p in slots]
    pos = torch.cat([p.float() for _, p in slots], 0).cuda()
    ptr = torch.tensor([0] + sizes).cumsum(0).to(torch.int32).cuda()
    pairs, pair_ptr = PF.contact_pairs(pos, ptr, rec.float().cuda(), radius)
    assert pairs.dtype == torch.int32 and pair_ptr.dtype == torch.int32 and pairs.shape == (int(pair_ptr[-1]), 2)
    return pairs.cpu().numpy(), pair_ptr.cpu().numpy()


def test_contact_list_equals_the_fixtures_unique_pairs():
    c = AttrCase('attr_dimout3_ball120')
    d = c.drop_table()
    _, first = np.unique(d[:, 0] * c.n + d[:, 1], return_index=True)          # (by ligand atom, then receptor atom)
    want = d[first] - np.array([0, 12])
    assert want.shape == (85, 2) and want[:, 0].max() < 12 and want[:, 1].min() >= 0
    pairs, pair_ptr = _contact_pairs([(None, c.pos[:12])], c.pos[12:], 4.0)
    assert pair_ptr.tolist() == [0, 85] and np.array_equal(pairs, want)


def test_contact_list_equals_the_builders_class_1_edges():
    slots, rec, rec_feats, model = _case()
    far = (slots[2][0], slots[2][1] + 100.0)                    # a hit with no contact, beside the hit of 0 atoms
    hits = list(slots) + [far]
    for radius in (4.0, 7.0):
        want, want_ptr = _class1(_plain(radius), SLOT_SIZES)
        pairs, pair_ptr = _contact_pairs(hits, rec, radius)
        assert pair_ptr.tolist() == want_ptr.tolist() + [int(want_ptr[-1])] and np.array_equal(pairs, want)
        assert pair_ptr[1] == 0 and len(want) > 100
    # a radius that is one pair's own distance: the strict < leaves that pair out, one ulp more takes it in
    want, _ = _class1(_plain(4.0), SLOT_SIZES)
    a, r = (int(v) for v in want[len(want) // 2])
    p = int(np.searchsorted(_class1(_plain(4.0), SLOT_SIZES)[1], len(want) // 2, side='right')) - 1
    diff = slots[p][1][a].double().numpy() - rec[r].double().numpy()
    s = 0.0
    for k in range(3):
        s += float(diff[k] * diff[k])
    r0 = float(np.sqrt(np.float64(s)))
    from pointvs_amd.screening import LibraryScreen
    counts = []
    for radius in (r0, float(np.nextafter(r0, np.inf))):
        screen = LibraryScreen(model, rec.cuda(), rec_feats, B, 130, radius)
        f = screen.load(slots)._build()
        screen.check()
        edges, edges_ptr = _class1(_np(f, screen), SLOT_SIZES)
        pairs, pair_ptr = _contact_pairs(slots, rec, radius)
        assert np.array_equal(pairs, edges) and np.array_equal(pair_ptr, edges_ptr)
        mine = pairs[pair_ptr[p]:pair_ptr[p + 1]]
        counts.append(int(((mine[:, 0] == a) & (mine[:, 1] == r)).sum()))
    assert counts == [0, 1]


def test_contact_list_refuses_wrong_arguments():
    from pointvs_amd import functional as PF
    slots, rec, _, _ = _case()
    pos, ptr = slots[2][1].cuda(), torch.tensor([0, 5], dtype=torch.int32).cuda()
    with pytest.raises(ValueError, match='not an ascending table'):
        PF.contact_pairs(pos, torch.tensor([0, 3, 2, 5], dtype=torch.int32).cuda(), rec.cuda(), 4.0)
    with pytest.raises(ValueError, match='not an ascending table'):
        PF.contact_pairs(pos, torch.tensor([0, 6], dtype=torch.int32).cuda(), rec.cuda(), 4.0)
    with pytest.raises(ValueError):
        PF.contact_pairs(pos, ptr.long(), rec.cuda(), 4.0)
    with pytest.raises(ValueError):
        PF.contact_pairs(pos, ptr, rec.cuda(), 0.0)
    with pytest.raises(TypeError):
        PF.contact_pairs(pos.double(), ptr, rec.cuda(), 4.0)
    with pytest.raises(RuntimeError):
        PF.contact_pairs(pos.cpu(), ptr.cpu(), rec, 4.0)
    pairs, pair_ptr = PF.contact_pairs(pos[:0], torch.zeros(1, dtype=torch.int32).cuda(), rec.cuda(), 4.0)   # no hits
    assert pairs.shape == (0, 2) and pair_ptr.tolist() == [0]


# ---------------------------------------------------------------- the packer

SIZES = [0, 1, 2, 5, 64, 65, 130]
PAIRS = [[(-1, 3)], [(0, 0), (-1, 149)], [], [(0, 1), (4, 2), (2, -1)], [(63, 5), (0, 149), (-1, -1)],
         [(64, 7), (10, 11)], [(129, 0), (64, 64), (-1, 10), (0, 0)]]
F, N_SLOTS, SLOT_CAP, SENTINEL = 12, 7, 130, -7.0


def _ligands(sizes):
    return mc.ligands(sizes, F)


_pair_table, _copies = mc.pair_table, mc.pair_copies


def _want(copies, first):
    return mc.packed_batch(copies, first, N_SLOTS, SLOT_CAP, F, SENTINEL)


def _pack(pos, feats, ptr, table, pair_ptr, first, n_slots=N_SLOTS, slot_cap=SLOT_CAP, n_rec=150):
    """One launch into sentinel-filled outputs; (pos, feats, ptr, rec_drop, status) as numpy."""
    from pointvs_amd import functional as PF
    rows = n_slots * slot_cap
    out = (torch.full((rows, 3), SENTINEL).cuda(), torch.full((rows, F), SENTINEL).cuda(),
           torch.full((n_slots + 1,), 12345, dtype=torch.int32).cuda(),
           torch.full((n_slots,), 54321, dtype=torch.int32).cuda(), torch.full((1,), 77, dtype=torch.int32).cuda())
    got = PF.leave_out_pair_pack(torch.from_numpy(pos).cuda(), torch.from_numpy(feats).cuda(),
                                 torch.from_numpy(ptr).cuda(), torch.from_numpy(table).cuda(),
                                 torch.from_numpy(pair_ptr).cuda(), n_rec,
                                 torch.tensor([first], dtype=torch.int32).cuda(), n_slots, slot_cap, out=out)
    assert all(g is o for g, o in zip(got, out))
    return tuple(t.cpu().numpy() for t in got)


def _firsts():
    total = sum(len(hit) for hit in PAIRS) + len(PAIRS)
    firsts = list(range(0, total, N_SLOTS))
    assert total == 22 and total % N_SLOTS and firsts[-1] + N_SLOTS > total     # the last batch is partly empty
    return firsts + [total + 6]                                                  # and one with every slot empty


def _run_all():
    pos, feats, ptr = _ligands(SIZES)
    table, pair_ptr = _pair_table(PAIRS)
    return [_pack(pos, feats, ptr, table, pair_ptr, first) for first in _firsts()]


def test_pair_packer_is_exact_and_reproducible():
    pos, feats, ptr = _ligands(SIZES)
    copies = _copies(pos, feats, ptr, PAIRS)
    runs = _run_all()
    for first, got in zip(_firsts(), runs):
        want = _want(copies, first)
        assert got[4][0] == 0, first
        for g, w in zip(got[:4], want):       # the written rows and the sentinels beyond out_ptr[n_slots], bit for bit
            assert g.tobytes() == w.tobytes(), first
    assert not runs[-1][2].any() and (runs[-1][3] == -1).all()           # first_copy >= total: every slot empty
    for a, b in zip(runs, _run_all()):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    # the allocating form gives the same rows
    from pointvs_amd import functional as PF
    table, pair_ptr = _pair_table(PAIRS)
    out_pos, out_feats, out_ptr, rec_drop, status = PF.leave_out_pair_pack(
        *(torch.from_numpy(a).cuda() for a in (pos, feats, ptr, table, pair_ptr)), 150,
        torch.tensor([9], dtype=torch.int32).cuda(), N_SLOTS, SLOT_CAP)
    want_pos, want_feats, want_ptr, want_drop = _want(copies, 9)
    n = int(want_ptr[-1])
    assert int(status) == 0 and np.array_equal(out_ptr.cpu().numpy(), want_ptr)
    assert np.array_equal(rec_drop.cpu().numpy(), want_drop)
    assert np.array_equal(out_pos[:n].cpu().numpy(), want_pos[:n])
    assert np.array_equal(out_feats[:n].cpu().numpy(), want_feats[:n])


def test_pair_packer_refuses_bad_tables():
    pos, feats, _ = _ligands([9])
    i32 = lambda *v: np.array(v, dtype=np.int32)               # noqa: E731
    one = i32(0, 9)
    bad = [(i32(0, 5, 3, 9), i32(0, 0, 0, 0), i32().reshape(0, 2), 1024),          # lig_ptr descending
           (one, i32(0, 0), i32().reshape(0, 2), 8),                               # a ligand of slot_cap + 1 atoms
           (i32(0, 4, 10), i32(0, 0, 0), i32().reshape(0, 2), 1024),               # ends outside the 9 rows
           (i32(0, 4, 9), i32(0, 2, 1), i32(0, 0, 1, 1).reshape(2, 2), 1024),      # pair_ptr descending
           (one, i32(0, 3), i32(0, 0, 1, 1).reshape(2, 2), 1024),                  # pair_ptr ends outside the pairs
           (one, i32(1, 2), i32(0, 0, 1, 1).reshape(2, 2), 1024),                  # pair_ptr does not start at 0
           (one, i32(0, 2), i32(0, 0, 9, 1).reshape(2, 2), 1024),                  # a outside the hit
           (one, i32(0, 2), i32(-2, 0, 1, 1).reshape(2, 2), 1024),
           (one, i32(0, 2), i32(0, 0, 1, 150).reshape(2, 2), 1024),                # r outside the receptor
           (one, i32(0, 2), i32(0, -2, 1, 1).reshape(2, 2), 1024)]
    for ptr, pair_ptr, table, slot_cap in bad:
        got_pos, got_feats, got_ptr, drop, status = _pack(pos, feats, ptr, table, pair_ptr, 0, 3, slot_cap)
        assert status[0] & 8, (ptr, pair_ptr, table)
        assert not got_ptr.any() and (drop == -1).all(), (ptr, pair_ptr, table)
        assert np.all(got_pos == SENTINEL) and np.all(got_feats == SENTINEL), (ptr, pair_ptr, table)
    got = _pack(pos, feats, one, i32(0, 0, 8, 149).reshape(2, 2), i32(0, 2), 0, 3, 9)     # (the edges of both ranges)
    assert got[4][0] == 0 and got[2].tolist() == [0, 9, 17, 25] and got[3].tolist() == [-1, 0, 149]


def test_pair_packer_wrapper_refuses_wrong_arguments():
    from pointvs_amd import functional as PF
    pos, feats, ptr = (torch.from_numpy(a).cuda() for a in _ligands([3, 2]))
    table = torch.tensor([[0, 1], [1, 2]], dtype=torch.int32).cuda()
    pair_ptr = torch.tensor([0, 1, 2], dtype=torch.int32).cuda()
    first = torch.zeros(1, dtype=torch.int32).cuda()
    with pytest.raises(TypeError):
        PF.leave_out_pair_pack(pos.double(), feats, ptr, table, pair_ptr, 5, first, 2, 4)
    with pytest.raises(ValueError):
        PF.leave_out_pair_pack(pos, feats, ptr.long(), table, pair_ptr, 5, first, 2, 4)
    with pytest.raises(ValueError):
        PF.leave_out_pair_pack(pos, feats[:4], ptr, table, pair_ptr, 5, first, 2, 4)
    with pytest.raises(ValueError):
        PF.leave_out_pair_pack(pos, feats, ptr, table.long(), pair_ptr, 5, first, 2, 4)
    with pytest.raises(ValueError):
        PF.leave_out_pair_pack(pos, feats, ptr, table.reshape(-1), pair_ptr, 5, first, 2, 4)
    with pytest.raises(ValueError):
        PF.leave_out_pair_pack(pos, feats, ptr, table, pair_ptr[:2], 5, first, 2, 4)
    with pytest.raises(ValueError):
        PF.leave_out_pair_pack(pos, feats, ptr, table, pair_ptr, 0, first, 2, 4)
    with pytest.raises(ValueError):
        PF.leave_out_pair_pack(pos, feats, ptr, table, pair_ptr, 5, first.long(), 2, 4)
    with pytest.raises(ValueError):          # rec_drop of the wrong length
        PF.leave_out_pair_pack(pos, feats, ptr, table, pair_ptr, 5, first, 2, 4,
                               out=(pos.new_zeros((8, 3)), feats.new_zeros((8, F)), ptr.new_zeros(3), ptr.new_zeros(3),
                                    ptr.new_zeros(1)))
    with pytest.raises(RuntimeError):
        PF.leave_out_pair_pack(pos.cpu(), feats.cpu(), ptr.cpu(), table.cpu(), pair_ptr.cpu(), 5, first.cpu(), 2, 4)
