"""The pose-batch builders, the leave-out packers and the hit listers at 65-513 slots or hits: the counts at which a
second wave has work (65; 66 slots for the packers' sums over the slots before), the thread behind the last slot is
the last of block 0, the first of block 1 and one past it, every `+= 256` loop makes a second trip and a one-block scan's threads own two entries (255, 256, 257), and
a third trip, a third block and three entries per thread (513). Every array is compared for equality of bytes with the
numpy references of tests/_many_slots_cases.py (the oracle's generate_edges per slot, tests/_attribution_ref.masked_coo,
tests/_crop_ref.py, tests/_crop_copies_ref.py, a brute-force fp64 contact list): no GPU result is a yardstick. The one
exception is the end-to-end check at the bottom, under the bound tests/test_gpu_contact_masking.py states for screens
built on other batches."""
import numpy as np
import pytest
import torch

from tests import _crop_copies_ref as cref
from tests import _many_slots_cases as mc
from tests.test_gpu_ligand_masking import _single_head
from tests.test_gpu_struck_slots import _np

pytestmark = pytest.mark.gpu

COUNTS, N_REC = mc.COUNTS, mc.N_REC
CROP, RADIUS = 6.0, 4.0
CASES = [(b, RADIUS) for b in COUNTS] + [(257, 7.0)]

_CACHE = {}


def _receptor():
    if 'rec' not in _CACHE:
        rec, rec_feats = mc.receptor()
        _CACHE['rec'] = (rec, rec_feats, torch.from_numpy(rec), torch.from_numpy(rec_feats), _single_head(21))
    return _CACHE['rec']


def _torch_slots(slots):
    return [(torch.from_numpy(np.ascontiguousarray(f)), torch.from_numpy(np.ascontiguousarray(p))) for f, p in slots]


def _screen(b, radius, **kw):
    from pointvs_amd.screening import LibraryScreen
    _, _, rec, rec_feats, model = _receptor()
    return LibraryScreen(model, rec.cuda(), rec_feats, b, mc.SLOT_CAP, radius, **kw)


def _sums(screen):
    return tuple(t.cpu().numpy() for t in (screen.rec_magg, screen.rec_xsum, screen.rec_deg))


def _same(got, want, what):
    for k, w in want.items():
        assert got[k].dtype == w.dtype and got[k].shape == w.shape, (what, k, got[k].dtype, got[k].shape, w.shape)
        assert got[k].tobytes() == w.tobytes(), (what, k, np.flatnonzero(got[k].reshape(-1) != w.reshape(-1))[:5])


# ---------------------------------------------------------------- the ragged and the struck builder

def _ragged(b, radius):
    """The ragged builder's output of the batch of b slots, twice (the second run's bytes are compared in the test),
    and the screen's receptor sums."""
    if ('ragged', b, radius) not in _CACHE:
        screen = _screen(b, radius)
        slots = _torch_slots(mc.slots(b))
        f = screen.load(slots)._build()
        screen.check()
        got = _np(f, screen)
        again = _np(screen.load(slots)._build(), screen)
        screen.check()
        _CACHE['ragged', b, radius] = (got, again, _sums(screen), screen.n_cap)
    return _CACHE['ragged', b, radius]


@pytest.mark.parametrize('b,radius', CASES)
def test_ragged_builder_is_exact(b, radius):
    rec, rec_feats = _receptor()[:2]
    got, again, sums, n_cap = _ragged(b, radius)
    assert n_cap == b * (mc.SLOT_CAP + N_REC) and got['status'][0] == 0
    want = mc.slot_batch(mc.slot_edges(b, radius), mc.slots(b), [-1] * b, rec, rec_feats, sums, n_cap)
    assert want['node_ptr'][-1] == sum(mc.slot_sizes(b)) + b * N_REC and len(want['row_l']) > 1000
    _same(got, want, (b, radius))
    assert all(again[k].tobytes() == got[k].tobytes() for k in got)


def _struck_table(b, radius):
    """rec_drop of the batch: per slot -1, atom 0, atom n_rec - 1, an atom with ligand contacts or one without them but
    with template neighbours (from the reference edge lists), the kind by p % 5 - so the slots 0, 63, 64, 255, 256 and
    b - 1 get a contact atom (the free one: they are empty), the last atom, none, ... and every kind is spread between."""
    table = []
    for p, ((ei, et), n) in enumerate(zip(mc.slot_edges(b, radius), mc.slot_sizes(b))):
        touched = set((ei[1][(ei[0] < n) & (ei[1] >= n)] - n).tolist())
        free = sorted(set((ei[0][et == 2] - n).tolist()) - touched)
        contact = min(touched) if touched else -1
        free = free[len(free) // 2] if free else -1
        kind = ('contact', 'free', 'first', 'last', 'whole')[p % 5]
        table.append(int({'whole': -1, 'first': 0, 'last': N_REC - 1, 'free': free if free >= 0 else contact,
                          'contact': contact if contact >= 0 else free}[kind]))
    return table


@pytest.mark.parametrize('b,radius', CASES)
def test_struck_builder_is_exact(b, radius):
    rec, rec_feats = _receptor()[:2]
    plain, _, sums, n_cap = _ragged(b, radius)
    slots = _torch_slots(mc.slots(b))
    screen = _screen(b, radius, struck=True)
    f = screen.load(slots)._build()                      # sized as every screen is: from the whole slots
    screen.check()
    unstruck = _np(f, screen)
    for k in unstruck:                                   # an all -1 table: what the ragged builder writes
        assert unstruck[k].tobytes() == plain[k].tobytes(), (b, k)
    rec_drop = _struck_table(b, radius)
    late = [rec_drop[p] for p in (0, 63, 64, 255, 256, b - 1) if p < b]
    assert sum(r >= 0 for r in rec_drop) >= b // 2 and sum(r >= 0 for r in late) >= 2 and -1 in rec_drop
    got = _np(screen.load(slots, rec_drop=rec_drop)._build(), screen)
    screen.check()
    want = mc.slot_batch(mc.slot_edges(b, radius), mc.slots(b), rec_drop, rec, rec_feats, sums, n_cap)
    assert got['status'][0] == 0
    assert want['node_ptr'][-1] == plain['node_ptr'][-1] - sum(r >= 0 for r in rec_drop)
    assert len(want['row']) < len(plain['row']) and len(want['row_l']) > len(plain['row_l'])
    _same(got, want, (b, radius))
    again = _np(screen.load(slots, rec_drop=rec_drop)._build(), screen)
    screen.check()
    assert all(again[k].tobytes() == got[k].tobytes() for k in got)


# ---------------------------------------------------------------- cropped slots, cropped copies

def _keep_rank(f, screen):
    """keep_rank [B, W + 1] out of the builder's state: behind the three mask tables, the atom -> slot table and the
    degree table of the cropped layout, each carved at the next multiple of 256 bytes (screen_graph.hip: carve_screen)."""
    chunks, words = (screen.n_rec + 63) // 64, (screen.slot_cap + 63) // 64
    off = 0
    for size in (screen.l_cap * chunks * 8, screen.l_cap * chunks * 8, screen.l_cap * words * 8, screen.l_cap * 4,
                 (screen.n_cap + 1) * 4):
        off = -(-off // 256) * 256 + size
    off = -(-off // 256) * 256
    n = screen.b * (chunks + 1)
    assert off + 4 * n <= f['state'].numel()
    return f['state'][off:off + 4 * n].cpu().numpy().view(np.int32).reshape(screen.b, chunks + 1)


def _np_cropped(f, screen):
    torch.cuda.synchronize()
    out = {k: f[k].cpu().numpy() for k in ('rowptr', 'inv_deg', 'node_ptr', 'node_graph', 'pos', 'x', 'status')}
    e = int(out['rowptr'][screen.n_cap])
    for k in ('row', 'col', 'etype'):
        out[k] = f[k][:e].cpu().numpy()
    out['keep'] = f['keep'].cpu().numpy().view(np.uint64)
    out['keep_rank'] = _keep_rank(f, screen)
    assert 'rowptr_l' not in f and 'base_magg' not in f
    return out


@pytest.mark.parametrize('b,radius', CASES)
def test_cropped_builder_is_exact(b, radius):
    rec, rec_feats = _receptor()[:2]
    sizes = mc.slot_sizes(b)
    screen = _screen(b, radius, crop_radius=CROP)
    slots = _torch_slots(mc.slots(b))
    got = _np_cropped(screen.load(slots)._build(), screen)
    screen.check()
    want = mc.cropped_batch(mc.slots(b), rec, rec_feats, CROP, radius, screen.n_cap, cache=list(zip(range(b), sizes)))
    kept = want['keep_rank'][:, -1]
    assert got['status'][0] == 0 and kept.min() == 0 and kept.max() == N_REC and ((kept > 0) & (kept < N_REC)).any()
    assert kept[[p for p in range(b) if sizes[p] == 0]].max() == 0 and len(want['row']) > 1000
    _same(got, want, (b, radius))
    again = _np_cropped(screen.load(slots)._build(), screen)
    screen.check()
    assert all(again[k].tobytes() == got[k].tobytes() for k in got)


def _copies_case(b):
    """Slots that are leave-out copies: an odd slot of two atoms or more holds its parent without atom p % n, every
    tenth slot from 3 is cropped around nothing, every other one around its own atoms; rec_drop by p % 5: -1, an atom
    the crop keeps, atom 0, atom n_rec - 1, an atom the crop does not keep."""
    rec = _receptor()[0]
    slots, parents, drops = [], [], []
    for p, (feats, pose) in enumerate(mc.slots(b)):
        n = len(pose)
        parent = pose
        if p % 10 == 3:
            parent = pose[:0]
        elif p % 2 == 1 and n >= 2:
            rows = [a for a in range(n) if a != p % n]
            feats, pose = feats[rows], pose[rows]
        mask = mc.ref.keep_mask(parent, rec, CROP)
        kept, gone = np.flatnonzero(mask), np.flatnonzero(~mask)
        drops.append(int((-1, kept[len(kept) // 2] if len(kept) else 5, 0, N_REC - 1, gone[0] if len(gone) else -1)[p % 5]))
        slots.append((feats, pose))
        parents.append(parent)
    return slots, parents, drops


def _load_copies(screen, slots, parents, drops):
    """The slots loaded as they are, then the crop table and rec_drop of the screen overwritten with the parents'."""
    screen.load(slots)
    ptr = np.concatenate([[0], np.cumsum([len(p) for p in parents])]).astype(np.int32)
    screen.crop_ptr.copy_(torch.from_numpy(ptr))
    packed = torch.from_numpy(np.concatenate(parents).astype(np.float32).reshape(-1, 3))
    screen.crop_pos[:packed.shape[0]].copy_(packed)
    screen.rec_drop.copy_(torch.tensor(drops, dtype=torch.int32))
    return screen


@pytest.mark.parametrize('b,radius', CASES)
def test_cropped_copies_builder_is_exact(b, radius):
    rec, rec_feats = _receptor()[:2]
    slots, parents, drops = _copies_case(b)
    assert sum(len(s[1]) < len(q) for s, q in zip(slots, parents)) >= 20 and len(set(drops)) >= 5
    screen = _screen(b, radius, crop_radius=CROP, crop_parents=True)
    got = _np_cropped(_load_copies(screen, _torch_slots(slots), parents, drops)._build(), screen)
    screen.check()
    want = mc.cropped_batch(slots, rec, rec_feats, CROP, radius, screen.n_cap, parents=parents, rec_drop=drops)
    assert got['status'][0] == 0 and len(want['row']) > 1000
    _same(got, want, (b, radius))
    again = _np_cropped(_load_copies(screen, _torch_slots(slots), parents, drops)._build(), screen)
    screen.check()
    assert all(again[k].tobytes() == got[k].tobytes() for k in got)


# ---------------------------------------------------------------- bad tables that sit late

B_BAD = 300


def _spoil_lig_ptr(screen):                     # a descending pair at entry 280
    assert int(screen.lig_ptr[281] - screen.lig_ptr[280]) >= 1
    screen.lig_ptr[281] = screen.lig_ptr[280] - 1


def _spoil_width(screen):                       # slot 299, the last, wider than slot_cap (inside L_cap all the same)
    screen.lig_ptr[300] = screen.lig_ptr[299] + screen.slot_cap + 1
    assert int(screen.lig_ptr[300]) <= screen.l_cap


def _spoil_rec_drop(screen):                    # (load() refuses such a list on the host: straight into the table)
    screen.rec_drop[290] = N_REC


def _spoil_crop_ptr(screen):                    # slot 270's crop set ends past crop_cap
    screen.crop_ptr[271:] = screen.l_cap + 1


@pytest.mark.parametrize('kind,kw,spoil', [('lig_ptr', dict(), _spoil_lig_ptr),
                                           ('width', dict(crop_radius=CROP), _spoil_width),
                                           ('rec_drop', dict(struck=True), _spoil_rec_drop),
                                           ('crop_ptr', dict(crop_radius=CROP, crop_parents=True), _spoil_crop_ptr)])
def test_a_bad_entry_behind_slot_256_gives_an_edgeless_batch_and_the_next_build_is_clean(kind, kw, spoil):
    """B = 300: what the builders refuse at 6 slots they refuse when the entry sits where only the second trip of a
    `+= 256` loop, or the table walk of the thread behind the last slot in block 1, sees it: bit 3 of the status, an
    edgeless batch, and the next good build on the same buffers exact."""
    rec, rec_feats = _receptor()[:2]
    cropped = 'crop_radius' in kw
    as_np = _np_cropped if cropped else _np
    slots = _torch_slots(mc.slots(B_BAD))
    screen = _screen(B_BAD, RADIUS, **kw)
    f = screen.load(slots)._build()
    screen.check()
    good = as_np(f, screen)
    if cropped:
        want = mc.cropped_batch(mc.slots(B_BAD), rec, rec_feats, CROP, RADIUS, screen.n_cap,
                                cache=list(zip(range(B_BAD), mc.slot_sizes(B_BAD))))
    else:
        want = mc.slot_batch(mc.slot_edges(B_BAD, RADIUS), mc.slots(B_BAD), [-1] * B_BAD, rec, rec_feats, _sums(screen),
                             screen.n_cap)
    assert good['status'][0] == 0
    _same(good, want, kind)
    screen.load(slots)
    spoil(screen)
    screen._launch_builder(f)
    bad = as_np(f, screen)
    assert bad['status'][0] & 8, kind
    assert not bad['rowptr'].any() and len(bad['row']) == 0 and (bad['node_graph'] == -1).all(), kind
    assert (bad['inv_deg'] == 1).all(), kind
    if cropped:
        assert not bad['node_ptr'].any() and not bad['pos'].any() and not bad['x'].any(), kind
    else:
        assert not bad['rowptr_l'].any() and len(bad['row_l']) == 0, kind
    with pytest.raises(ValueError, match='LibraryScreen: lig_ptr is not a table'):
        screen._raise_for(int(bad['status'][0]))
    screen.load(slots)                                   # one writer of the status word: nothing to clear
    screen._launch_builder(f)
    after = as_np(f, screen)
    assert after['status'][0] == 0
    _same(after, want, kind)


# ---------------------------------------------------------------- the packers

SLOT_CAP, SENTINEL = 9, -7.0
# (a packer's slot k sums the slots before it, t < k: slot 64, the last of 65, still sums wave 0 alone - 66 slots is the
# first count at which a second wave holds a term, and the tests assert that it is not zero)
PACK_SLOTS = (65, 66) + COUNTS[1:]


def _hit_table(n_hits):
    if ('hits', n_hits) not in _CACHE:
        sizes = mc.hit_sizes(n_hits)
        pairs = mc.hit_pairs(sizes, N_REC)
        pos, feats, ptr = mc.ligands(sizes)
        table, pair_ptr = mc.pair_table(pairs)
        _CACHE['hits', n_hits] = dict(sizes=sizes, pairs=pairs, pos=pos, feats=feats, ptr=ptr, table=table,
                                      pair_ptr=pair_ptr, atom_copies=mc.ligand_copies(pos, feats, ptr),
                                      pair_copies=mc.pair_copies(pos, feats, ptr, pairs))
    return _CACHE['hits', n_hits]


def _firsts(total, mid_hit, n_slots):
    """first_copy values: the start, mid-hit (inside the 9-atom hit's copies), the middle of the table, one that leaves
    the last min(260, n_slots - 1) slots behind the final copy, and one with every slot empty."""
    return [0, mid_hit, total // 2, total - (n_slots - min(260, n_slots - 1)), total + 6]


def _dev(*arrays):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays)


def _outputs(n_slots, with_feats=True, with_drop=False):
    rows = n_slots * SLOT_CAP
    out = [torch.full((rows, 3), SENTINEL).cuda()]
    if with_feats:
        out.append(torch.full((rows, mc.F), SENTINEL).cuda())
    out.append(torch.full((n_slots + 1,), 12345, dtype=torch.int32).cuda())
    if with_drop:
        out.append(torch.full((n_slots,), 54321, dtype=torch.int32).cuda())
    out.append(torch.full((1,), 77, dtype=torch.int32).cuda())
    return tuple(out)


def _pack_atoms(t, first, n_slots, ptr=None):
    from pointvs_amd import functional as PF
    got = PF.leave_out_ligand_pack(*_dev(t['pos'], t['feats'], t['ptr'] if ptr is None else ptr),
                                   torch.tensor([first], dtype=torch.int32).cuda(), n_slots, SLOT_CAP,
                                   out=_outputs(n_slots))
    return tuple(g.cpu().numpy() for g in got)


def _pack_pairs(t, first, n_slots, ptr=None, pair_ptr=None, table=None):
    from pointvs_amd import functional as PF
    got = PF.leave_out_pair_pack(*_dev(t['pos'], t['feats'], t['ptr'] if ptr is None else ptr,
                                       t['table'] if table is None else table,
                                       t['pair_ptr'] if pair_ptr is None else pair_ptr), N_REC,
                                 torch.tensor([first], dtype=torch.int32).cuda(), n_slots, SLOT_CAP,
                                 out=_outputs(n_slots, with_drop=True))
    return tuple(g.cpu().numpy() for g in got)


def _pack_parents(t, copy_ptr, first, n_slots, ptr=None):
    from pointvs_amd import functional as PF
    got = PF.leave_out_parent_pack(*_dev(t['pos'], t['ptr'] if ptr is None else ptr, copy_ptr),
                                   torch.tensor([first], dtype=torch.int32).cuda(), n_slots, SLOT_CAP,
                                   out=_outputs(n_slots, with_feats=False))
    return tuple(g.cpu().numpy() for g in got)


@pytest.mark.parametrize('n_hits', [257, 513])
@pytest.mark.parametrize('n_slots', PACK_SLOTS)
def test_ligand_packer_is_exact(n_slots, n_hits):
    t = _hit_table(n_hits)
    copies = t['atom_copies']
    firsts = _firsts(len(copies), int(t['ptr'][3]) + 3 + 4, n_slots)
    assert len(copies[firsts[1]][0]) == 8 and firsts[3] + n_slots - len(copies) == min(260, n_slots - 1)
    assert all(len(copies[first + 64][0]) for first in firsts[:3])       # (slot 65's term from the second wave)
    for first in firsts:
        got = _pack_atoms(t, first, n_slots)
        want = mc.packed_batch(copies, first, n_slots, SLOT_CAP)
        assert got[3][0] == 0, first
        for g, w in zip(got[:3], want[:3]):      # the written rows and the sentinels behind out_ptr[n_slots], bit for bit
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (first, np.flatnonzero(got[2] != want[2])[:5])
        if first in firsts[:3]:
            assert want[2][-1] > n_slots and (want[0][want[2][-1]:] == SENTINEL).all()
    assert not got[2].any()                      # first_copy >= total: every slot empty
    again = _pack_atoms(t, firsts[2], n_slots)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, _pack_atoms(t, firsts[2], n_slots)))


@pytest.mark.parametrize('n_hits', [257, 513])
@pytest.mark.parametrize('n_slots', PACK_SLOTS)
def test_pair_packer_is_exact(n_slots, n_hits):
    t = _hit_table(n_hits)
    copies = t['pair_copies']
    firsts = _firsts(len(copies), int(t['pair_ptr'][3]) + 3 + 2, n_slots)
    assert len(t['pairs'][3]) >= 2 and copies[firsts[1]][2] >= 0 and firsts[3] + n_slots - len(copies) == min(260, n_slots - 1)
    assert any(len(copies[first + 64][0]) for first in firsts[:3])       # (slot 65's term from the second wave)
    for first in firsts:
        got = _pack_pairs(t, first, n_slots)
        want = mc.packed_batch(copies, first, n_slots, SLOT_CAP)
        assert got[4][0] == 0, first
        for g, w in zip(got[:4], want):
            assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (first, np.flatnonzero(got[2] != want[2])[:5])
        if first in firsts[:3]:
            assert want[2][-1] > n_slots and (want[3] >= 0).any() and (want[3] == -1).any()
    assert not got[2].any() and (got[3] == -1).all()
    again = _pack_pairs(t, firsts[2], n_slots)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, _pack_pairs(t, firsts[2], n_slots)))


@pytest.mark.parametrize('n_hits', [257, 513])
@pytest.mark.parametrize('n_slots', PACK_SLOTS)
def test_parent_packer_is_exact(n_slots, n_hits):
    t = _hit_table(n_hits)
    for copy_ptr in (t['ptr'], t['pair_ptr']):               # both numberings: ligand-atom copies, pair copies
        total = int(copy_ptr[-1]) + n_hits
        firsts = _firsts(total, int(copy_ptr[3]) + 3 + 1, n_slots)
        assert any(np.diff(cref.parent_pack(t['pos'], t['ptr'], copy_ptr, first, 65)[1])[64] for first in firsts[:3])
        for first in firsts:
            want_pos, want_ptr = cref.parent_pack(t['pos'], t['ptr'], copy_ptr, first, n_slots)
            got_pos, got_ptr, status = _pack_parents(t, copy_ptr, first, n_slots)
            n = int(want_ptr[-1])
            assert status[0] == 0 and got_ptr.tobytes() == want_ptr.tobytes(), (first, np.flatnonzero(got_ptr != want_ptr)[:5])
            assert got_pos[:n].tobytes() == want_pos.tobytes() and bool((got_pos[n:] == SENTINEL).all()), first
            assert n > n_slots if first <= total // 2 else n == 0 or first < total
        again = _pack_parents(t, copy_ptr, total // 2, n_slots)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, _pack_parents(t, copy_ptr, total // 2, n_slots)))


def test_packers_refuse_a_bad_entry_behind_index_256():
    """513 hits, 513 slots: a descending lig_ptr pair at entry 301, a descending pair_ptr pair at entry 402, and a pair
    row outside its hit that the copy in slot 300 owns (what only the second trip of the packers' loops reads): status
    8, out_ptr zeros, rec_drop -1, no row written."""
    n_hits = n_slots = 513
    t = _hit_table(n_hits)
    bad_lig = t['ptr'].copy()
    assert bad_lig[302] - bad_lig[301] >= 1
    bad_lig[302] = bad_lig[301] - 1
    bad_pairs = t['pair_ptr'].copy()
    assert bad_pairs[403] - bad_pairs[402] >= 1
    bad_pairs[403] = bad_pairs[402] - 1
    owners = [(h, -1 if j == 0 else int(t['pair_ptr'][h]) + j - 1) for h, hit in enumerate(t['pairs'])
              for j in range(len(hit) + 1)]                 # per copy: (hit, the pair row it leaves out or -1)
    first = next(c for c in range(150, 400) if owners[c + 300][1] >= 0)
    hit, row = owners[first + 300]
    assert cref.copy_hits(t['pair_ptr'], first + 300, 1) == [hit] and len(owners) == len(t['pair_copies'])
    bad_table = t['table'].copy()
    bad_table[row, 0] = t['sizes'][hit]                      # a = n: outside the hit
    assert _pack_pairs(t, first, n_slots)[4][0] == 0         # (the good tables pack)
    runs = [_pack_atoms(t, 7, n_slots, ptr=bad_lig), _pack_pairs(t, 7, n_slots, ptr=bad_lig),
            _pack_pairs(t, 7, n_slots, pair_ptr=bad_pairs), _pack_pairs(t, first, n_slots, table=bad_table),
            _pack_parents(t, t['pair_ptr'], 7, n_slots, ptr=bad_lig), _pack_parents(t, bad_pairs, 7, n_slots)]
    for k, got in enumerate(runs):
        assert got[-1][0] == 8, k
        ptr = got[-3] if len(got) == 5 else got[-2]
        assert ptr.shape == (n_slots + 1,) and not ptr.any(), k
        assert (got[0] == SENTINEL).all(), k
        if len(got) >= 4:
            assert (got[1] == SENTINEL).all(), k
        if len(got) == 5:
            assert (got[3] == -1).all(), k
    # the same row in a batch that does not hold its copy: packed (a bad row is refused by the batch that holds it)
    assert _pack_pairs(t, first + 301, n_slots, table=bad_table)[4][0] == 0


# ---------------------------------------------------------------- the listers

def _lister_case(s, swap):
    pos, ptr = mc.lister_hits(s, swap)
    return pos, ptr, torch.from_numpy(pos).cuda(), torch.from_numpy(ptr).cuda(), _receptor()[2].cuda()


@pytest.mark.parametrize('swap', [False, True], ids=['empty-first', 'far-first'])
@pytest.mark.parametrize('s', COUNTS)
def test_contact_lister_is_exact(s, swap):
    from pointvs_amd import functional as PF
    rec = _receptor()[0]
    pos, ptr, pos_dev, ptr_dev, rec_dev = _lister_case(s, swap)
    for radius in (RADIUS, 7.0) if s == 257 else (RADIUS,):
        want, want_ptr = mc.contact_list(pos, ptr, rec, radius)
        runs = [PF.contact_pairs(pos_dev, ptr_dev, rec_dev, radius, host_ptr=True) for _ in range(2)]
        for pairs, pair_ptr, host in runs:
            assert pairs.dtype == torch.int32 and pair_ptr.dtype == torch.int32
            assert pair_ptr.cpu().numpy().tobytes() == want_ptr.tobytes() == host.numpy().tobytes()
            assert pairs.cpu().numpy().tobytes() == want.tobytes()
        counts = np.diff(want_ptr)
        assert len(want) > 1000 and all(counts[h] == 0 for h in (0, 255, 256, s - 1) if h < s)


@pytest.mark.parametrize('swap', [False, True], ids=['empty-first', 'far-first'])
@pytest.mark.parametrize('s', COUNTS)
def test_crop_keep_is_exact(s, swap):
    from pointvs_amd import functional as PF
    rec = _receptor()[0]
    pos, ptr, pos_dev, ptr_dev, rec_dev = _lister_case(s, swap)
    words, kept_ptr = cref.hits_keep(pos, ptr, rec, CROP)
    counts = np.diff(kept_ptr)
    assert counts.max() == N_REC and ((counts > 0) & (counts < N_REC)).any()
    assert all(counts[h] == 0 for h in (0, 255, 256, s - 1) if h < s)
    runs = [PF.crop_keep(pos_dev, ptr_dev, rec_dev, CROP, host_ptr=True) for _ in range(2)]
    for keep, got_ptr, host in runs:
        assert keep.cpu().numpy().view(np.uint64).tobytes() == words.tobytes()
        assert got_ptr.cpu().numpy().tobytes() == kept_ptr.tobytes() == host.numpy().tobytes()
    hit, atom = PF.kept_atoms(runs[0][0], N_REC)
    want = [(h, j) for h in range(s) for j in np.flatnonzero(mc.ref.words_mask(words[h], N_REC))]
    assert list(zip(hit.tolist(), atom.tolist())) == want


def test_contact_fill_stops_at_the_rows_it_is_given():
    """pvs_contact_pairs_fill with n_pairs = total - 3: the first total - 3 rows exact, the three rows behind them
    untouched (the last hit with contacts is cut short: min(pair_ptr[s + 1], K) - p0)."""
    from pointvs_amd import _lib
    rec = _receptor()[0]
    s = 513
    pos, ptr, pos_dev, ptr_dev, rec_dev = _lister_case(s, False)
    want, want_ptr = mc.contact_list(pos, ptr, rec, RADIUS)
    total = int(want_ptr[-1])
    last = max(h for h in range(s) if want_ptr[h + 1] > want_ptr[h])
    assert want_ptr[last + 1] - want_ptr[last] > 3 and last < s - 1         # (one hit loses rows, not all of its rows)
    pair_ptr = torch.from_numpy(want_ptr).cuda()
    pairs = torch.full((total, 2), -99, dtype=torch.int32).cuda()
    _lib.check(_lib.lib().pvs_contact_pairs_fill(_lib.ptr(pos_dev), _lib.ptr(ptr_dev), s, pos.shape[0], _lib.ptr(rec_dev),
                                                 N_REC, RADIUS, _lib.ptr(pair_ptr), total - 3, _lib.ptr(pairs), None),
               'pvs_contact_pairs_fill')
    torch.cuda.synchronize()
    got = pairs.cpu().numpy()
    assert got[:total - 3].tobytes() == want[:total - 3].tobytes() and (got[total - 3:] == -99).all()


def test_listers_refuse_a_bad_entry_at_index_300():
    from pointvs_amd import _lib
    from pointvs_amd import functional as PF
    s = 513
    pos, ptr, pos_dev, _, rec_dev = _lister_case(s, False)
    bad = ptr.copy()
    assert bad[300] - bad[299] >= 1
    bad[300] = bad[299] - 1
    bad_dev = torch.from_numpy(bad).cuda()
    pair_ptr = torch.full((s + 1,), 5, dtype=torch.int32).cuda()
    _lib.check(_lib.lib().pvs_contact_pairs_count(_lib.ptr(pos_dev), _lib.ptr(bad_dev), s, pos.shape[0], _lib.ptr(rec_dev),
                                                  N_REC, RADIUS, _lib.ptr(pair_ptr), None), 'pvs_contact_pairs_count')
    keep = torch.full((s, 2), -1, dtype=torch.int64).cuda()
    kept_ptr = torch.full((s + 1,), 5, dtype=torch.int32).cuda()
    _lib.check(_lib.lib().pvs_crop_keep(_lib.ptr(pos_dev), _lib.ptr(bad_dev), s, pos.shape[0], _lib.ptr(rec_dev), N_REC,
                                        CROP, _lib.ptr(keep), _lib.ptr(kept_ptr), None), 'pvs_crop_keep')
    torch.cuda.synchronize()
    assert pair_ptr.tolist() == [0] * s + [-1]
    assert kept_ptr.tolist() == [0] * s + [-1] and not keep.any()
    with pytest.raises(ValueError, match='not an ascending table'):
        PF.contact_pairs(pos_dev, bad_dev, rec_dev, RADIUS)
    with pytest.raises(ValueError, match='not an ascending table'):
        PF.crop_keep(pos_dev, bad_dev, rec_dev, CROP)


# ---------------------------------------------------------------- end to end

def test_masking_scores_at_batch_257_equal_those_at_batch_4():
    """Five hits of 1-5 atoms: ligand_atom_masking and contact_masking through screens of 257 slots (one batch, mostly
    empty slots behind the copies) against screens of 4. Each raw output of a screen is within 1e-5 * max|raw| of the
    plain forward, so a difference of two outputs of one screen is within 4e-5 * max|raw| of the same difference of
    another (tests/test_gpu_contact_masking.py, tests/test_gpu_ligand_masking.py)."""
    from pointvs_amd.screening import ScreeningSweep
    _, _, rec, rec_feats, model = _receptor()
    slots, sizes = _torch_slots(mc.slots(65)), mc.slot_sizes(65)
    picked = [next(p for p in range(2, 63) if sizes[p] == n and p % mc.FAR_EVERY != mc.FAR_AT) for n in (1, 2, 3, 4, 5)]
    hits = [(f'hit{p}', *slots[p]) for p in picked]
    assert sorted(pose.shape[0] for _, _, pose in hits) == [1, 2, 3, 4, 5]
    small = ScreeningSweep(model, rec.cuda(), rec_feats, RADIUS, batch_size=4, capture=False)
    large = ScreeningSweep(model, rec.cuda(), rec_feats, RADIUS, batch_size=257, capture=False)
    want = small.ligand_atom_masking(hits, sigmoid=False)
    got = large.ligand_atom_masking(hits, sigmoid=False)
    assert large.masking.b == 257 and large.batches_run == 2           # (the sizing batch, then one step)
    for name, _, pose in hits:
        raw = small.atom_masking_raw[name]
        gap, bound = float((got[name] - want[name]).abs().max()), 4e-5 * float(raw.abs().max())
        print(f'ligand atoms {name}: batch 257 against batch 4 {gap:.3e} bound {bound:.3e}')
        assert got[name].shape == (pose.shape[0],) and gap <= bound and float(want[name].abs().max()) > 0
    want = small.contact_masking(hits, sigmoid=False)
    got = large.contact_masking(hits, sigmoid=False)
    assert large.struck.b == 257
    for name, _, _ in hits:
        raw = small.contact_masking_raw[name]
        assert torch.equal(got[name][0], want[name][0]) and got[name][0].shape[0] > 0
        gap, bound = float((got[name][1] - want[name][1]).abs().max()), 4e-5 * float(raw.abs().max())
        print(f'contacts {name}: batch 257 against batch 4 {gap:.3e} bound {bound:.3e}')
        assert gap <= bound and float(want[name][1].abs().max()) > 0
