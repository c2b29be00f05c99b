"""Receptor hotspot maps of hits on a cropped sweep: the two cropped reductions (PF.contact_attention_cropped,
PF.slot_node_values_cropped) bit for bit against their numpy restatements (tests/_crop_maps_ref.py) on hand-built cropped
batches and against the uncropped operators under full masks; ScreeningSweep(crop_radius=..., cropped_hotspots=True)
.receptor_hotspots against the fp64 oracle on the cropped complexes, at a crop above and one below the edge radius,
against the per-complex route, for GraphNorm, softmax-attention and two-headed models, twice on one sweep, end to end
after a cropped run_library; and the keywords off.

Bound of the parity tests: the project's parity bound, 1e-5 * max|value64| + 4 * noise32 - value64: the fp64 oracle's
values that are compared, noise32: the largest distance of the fp32 oracle (one thread) from them
(tests/_crop_maps_ref.py: bound_of; tests/test_crop_maps_host.py prints it: 4.5e-6 to 6.3e-6 on the main set-up; the sweep
was measured 6.7e-8 from the oracle at most for the attention maps and 3.5e-7 for the CAM). Counts
and NaN patterns are exact: no atom pair lies within 1e-4 of the edge radius or of a crop radius (asserted there).
"""
import re

import numpy as np
import pytest
import torch

from tests import _crop_maps_ref as ref
from tests._contact_ref import fresh_accumulators
from tests._crop_ref import cropped_complex, mask_words
from tests._golden import needs_caching_allocator
from tests.test_gpu_contact_attention import KW, N_REC_SCREEN, RADIUS, _close, _library, _set, attention_model, hits_and_receptor

pytestmark = pytest.mark.gpu

# ---------------------------------------------------------------- the operators, exact

SIZES = [0, 1, 5, 64, 65, 130, 0]          # ligand atoms per slot
PAD_ROWS, SENTINEL = 10, -7.0
COLUMNS = [(0, 1), (3, 1), (1, 3)]         # (column, n_mean) of the node values
NAMES = ('lig', 'slot_rec', 'rec_sum', 'rec_count', 'rec_max')
SPECIAL = {7: (-0.0, 0.0), 11: (-0.0, -0.0), 13: (np.nan, np.nan)}       # row % 97 -> its two class-1 values


def _mask(n_rec, atoms):
    m = np.zeros(n_rec, dtype=bool)
    m[list(atoms)] = True
    return m


def _wide_masks(rng):
    """130 receptor atoms - three mask words, two bits in the last: all atoms, none, atom 0 only, the last atom only,
    atoms 63 and 64 only, an empty middle word, random."""
    n = 130
    hollow = rng.random(n) < 0.5
    hollow[64:128] = False
    hollow[[0, 129]] = True
    return [_mask(n, range(n)), _mask(n, []), _mask(n, [0]), _mask(n, [n - 1]), _mask(n, [63, 64]), hollow,
            rng.random(n) < 0.4]


def _tables(sizes, masks):
    lig_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    rows = [n + int(m.sum()) for n, m in zip(sizes, masks)]
    node_ptr = np.concatenate([[0], np.cumsum(rows)]).astype(np.int32)
    return node_ptr, lig_ptr, np.stack([mask_words(m) for m in masks])


def _batch(name):
    """A hand-built cropped batch: dict(n_rec, node_ptr, lig_ptr, keep [S, W] uint64, n_nodes, lig_room).
    'wide' / 'word' / 'one': receptors of 130, 64 and 1 atoms, every slot accepted. 'broken': 70 receptor atoms, eight
    slots of which six are refused, each by one clause of the verdict alone."""
    rng = np.random.default_rng(len(name) + 2024)
    if name == 'wide':
        n_rec, sizes, masks = 130, SIZES, _wide_masks(rng)
    elif name == 'word':                         # one full word: bit 63 is an atom
        n_rec, sizes = 64, [3, 0, 64, 7, 2]
        masks = [_mask(64, range(64)), _mask(64, [63]), _mask(64, [63]), rng.random(64) < 0.5, _mask(64, [])]
    elif name == 'one':
        n_rec, sizes, masks = 1, [2, 0, 1, 3], [_mask(1, [0]), _mask(1, [0]), _mask(1, []), _mask(1, [0])]
    else:
        return _broken(rng)
    node_ptr, lig_ptr, keep = _tables(sizes, masks)
    return dict(n_rec=n_rec, node_ptr=node_ptr, lig_ptr=lig_ptr, keep=keep, n_nodes=int(node_ptr[-1]) + PAD_ROWS,
                lig_room=int(lig_ptr[-1]) + PAD_ROWS)


def _clauses(b, p):
    """The six clauses of the slot verdict, one by one."""
    a0, a1 = int(b['lig_ptr'][p]), int(b['lig_ptr'][p + 1])
    r0, r1 = int(b['node_ptr'][p]), int(b['node_ptr'][p + 1])
    bits = (((b['keep'][p][:, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)) != 0).reshape(-1)
    return (0 <= a0 <= a1, a1 - a0 <= 1024, 0 <= r0, r1 <= b['n_nodes'], r1 - r0 == (a1 - a0) + int(bits.sum()),
            not bits[b['n_rec']:].any())


def _broken(rng):
    """70 receptor atoms, eight slots. Slot 0 starts at row -1; slot 2 owns a row too many; slot 3 has bit 70 set (and the
    row that would go with it); slot 4 has 1,025 ligand atoms; slot 5's ligand table descends by one (and has one row
    less); slot 7 ends beyond the rows: each is refused by that clause alone. Slots 1 and 6 are slots; slot 6's ligand
    atoms lie where the refused slots 4 and 7 would have theirs (no other writer)."""
    n_rec = 70
    masks = [rng.random(n_rec) < 0.5 for _ in range(8)]
    keep = np.stack([mask_words(m) for m in masks])
    keep[3, 1] |= np.uint64(1) << np.uint64(6)              # slot 3: atom 70 of 70
    lig = [0, 3, 7, 9, 14, 1039, 1038, 1040, 1046]
    extra = {2: 1, 3: 1}                                    # slot 2: a row too many; slot 3: the stray bit's row
    nodes = [-1]
    for p in range(8):
        nodes.append(nodes[p] + lig[p + 1] - lig[p] + int(masks[p].sum()) + extra.get(p, 0))
    b = dict(n_rec=n_rec, keep=keep, node_ptr=np.array(nodes, dtype=np.int32), lig_ptr=np.array(lig, dtype=np.int32),
             n_nodes=nodes[8] - 1, lig_room=max(lig) + PAD_ROWS)
    failed = {p: [k for k, ok in enumerate(_clauses(b, p)) if not ok] for p in range(8)}
    assert failed == {0: [2], 1: [], 2: [4], 3: [5], 4: [1], 5: [0], 6: [], 7: [3]}, failed
    return b


def _rows(b, seed):
    """rowptr / etype / att / y over the batch's rows: per row class-1 edges first, last or interleaved with the others,
    a quarter of the rows without one; att: distinct small integers (every float64 sum exact), some NaN, +0.0 and
    -0.0, and five entries behind the edge count that no row reaches. Of every 97 rows one has 300 class-1 edges, one
    the class-1 values -0.0 and +0.0 (-> +0.0), one -0.0 twice (-> -0.0) and one NaN only (-> NaN)."""
    rng = np.random.default_rng(seed)
    n_nodes, rows = b['n_nodes'], []
    for r in range(n_nodes - PAD_ROWS):
        n1 = 0 if rng.random() < 0.25 else int(rng.integers(1, 40))
        if r % 97 == 5:
            n1 = 300                                         # more than one stride of the 16 lanes, and of the 64
        if r % 97 in SPECIAL:
            n1 = 2
        other = rng.choice(np.array([0, 2], dtype=np.uint8), size=int(rng.integers(0, 30)))
        ones = np.ones(n1, dtype=np.uint8)
        rows.append([np.concatenate([ones, other]), np.concatenate([other, ones]),
                     rng.permutation(np.concatenate([ones, other]))][r % 3])
    counts = [len(r) for r in rows] + [0] * (n_nodes - len(rows))
    rowptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    etype = np.concatenate(rows).astype(np.uint8)
    att = np.concatenate([rng.permutation(len(etype)) + 1.0, np.full(5, 1e9)]).astype(np.float32)
    kind = rng.random(len(att))
    att[kind < 0.06] = np.nan
    att[(kind >= 0.06) & (kind < 0.09)] = 0.0
    att[(kind >= 0.09) & (kind < 0.14)] = -0.0
    att[len(etype):] = 1e9
    for r in range(len(rows)):
        if r % 97 in SPECIAL:
            ones = rowptr[r] + np.nonzero(etype[rowptr[r]:rowptr[r + 1]] == 1)[0]
            att[ones] = SPECIAL[r % 97]
    assert len(etype) < 2 ** 24
    y = rng.standard_normal((n_nodes, 4)).astype(np.float32)
    return rowptr, etype, att, y


_BATCHES = {}


def _prepared(name):
    if name not in _BATCHES:
        b = _batch(name)
        b['rowptr'], b['etype'], b['att'], b['y'] = _rows(b, 5 + len(name))
        b['dev'] = {k: torch.from_numpy(b[k]).cuda() for k in ('rowptr', 'etype', 'att', 'y', 'node_ptr', 'lig_ptr')}
        b['dev']['keep'] = torch.from_numpy(b['keep'].view(np.int64)).cuda()
        _BATCHES[name] = b
    return _BATCHES[name]


def _outputs(b):
    from pointvs_amd import functional as PF
    n_slots = len(b['node_ptr']) - 1
    return (torch.full((b['lig_room'],), SENTINEL).cuda(), torch.full((n_slots, b['n_rec']), SENTINEL).cuda()
            ) + PF.new_contact_accumulators(b['n_rec'], 'cuda')


def _run_attention(b, calls):
    from pointvs_amd import functional as PF
    d, out, after = b['dev'], _outputs(b), []
    for _ in range(calls):
        got = PF.contact_attention_cropped(d['rowptr'], d['etype'], d['att'], d['node_ptr'], d['lig_ptr'], d['keep'],
                                           b['n_rec'], out=out)
        assert all(g is o for g, o in zip(got, out))
        after.append(tuple(t.cpu().numpy() for t in got))
    return after


def _run_values(b, calls, column, n_mean):
    from pointvs_amd import functional as PF
    d, out, after = b['dev'], _outputs(b), []
    for _ in range(calls):
        got = PF.slot_node_values_cropped(d['y'], d['node_ptr'], d['lig_ptr'], d['keep'], b['n_rec'], column, n_mean,
                                          out=out)
        after.append(tuple(t.cpu().numpy() for t in got))
    return after


def _same(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert g.tobytes() == w.tobytes(), (what, name, np.nonzero(~((g == w) | (np.isnan(g) & np.isnan(w)))))


@pytest.mark.parametrize('name', ['wide', 'word', 'one', 'broken'])
def test_operators_are_exact_accumulate_and_repeat(name):
    b = _prepared(name)
    n_rec, n_slots = b['n_rec'], len(b['node_ptr']) - 1
    accepted = [p for p in range(n_slots) if all(_clauses(b, p))]
    assert len(accepted) == (2 if name == 'broken' else n_slots)
    written = np.zeros(b['lig_room'], dtype=bool)
    for p in accepted:
        assert not written[b['lig_ptr'][p]:b['lig_ptr'][p + 1]].any()            # one writer per ligand row
        written[b['lig_ptr'][p]:b['lig_ptr'][p + 1]] = True
    # ---- attention
    lig, acc, wants = np.full(b['lig_room'], SENTINEL, dtype=np.float32), fresh_accumulators(n_rec), []
    for _ in range(2):
        lig, slot, *acc = ref.contact_attention_cropped(b['rowptr'], b['etype'], b['att'][:len(b['etype'])], b['node_ptr'],
                                                        b['lig_ptr'], b['keep'], n_rec, *acc, lig)
        wants.append((lig, slot, *acc))
    first = _run_attention(b, 2)
    for k in range(2):
        _same(first[k], wants[k], f'{name} attention call {k}')
    for a, c in zip(first, _run_attention(b, 2)):
        assert all(x.tobytes() == y.tobytes() for x, y in zip(a, c))
    got = first[0]
    assert (got[0][~written] == SENTINEL).all() and not (got[0][written] == SENTINEL).any()
    assert b['dev']['att'].cpu().numpy().tobytes() == b['att'].tobytes()                   # (the inputs are not written)
    assert not (got[1] == SENTINEL).any() and float(np.nanmax(got[1], initial=0)) < 1e9
    kept = np.stack([ref.words_mask(b['keep'][p], n_rec) if p in accepted else np.zeros(n_rec, bool)
                     for p in range(n_slots)])
    assert np.isnan(got[1][~kept]).all()
    if name == 'wide':      # the inputs hold what they should: kept atoms with and without a contact, signed zeros
        assert np.isnan(got[1][kept]).any() and (~np.isnan(got[1][kept])).any()
        zeros = got[1][0][got[1][0] == 0]                                       # (slot 0 keeps all: rows 7 and 11)
        assert np.signbit(zeros).any() and (~np.signbit(zeros)).any() and np.isnan(got[1][0, 13])
        assert len(set(got[3].tolist())) > 1 and np.array_equal(first[1][2], 2 * got[2])
        assert np.array_equal(first[1][3], 2 * got[3])
    # ---- node values
    for column, n_mean in COLUMNS:
        lig, acc, wants = np.full(b['lig_room'], SENTINEL, dtype=np.float32), fresh_accumulators(n_rec), []
        for _ in range(2):
            lig, slot, *acc = ref.slot_node_values_cropped(b['y'], column, n_mean, b['node_ptr'], b['lig_ptr'], b['keep'],
                                                           n_rec, *acc, lig)
            wants.append((lig, slot, *acc))
        runs = _run_values(b, 2, column, n_mean)
        for k in range(2):
            _same(runs[k], wants[k], f'{name} values {column, n_mean} call {k}')
        for a, c in zip(runs, _run_values(b, 2, column, n_mean)):
            assert all(x.tobytes() == y.tobytes() for x, y in zip(a, c))
        with_ligand = kept & (np.diff(b['lig_ptr'])[:, None] > 0)
        assert (~np.isnan(runs[0][1][with_ligand])).all() and np.isnan(runs[0][1][~with_ligand]).all()
        assert (runs[0][0][~written] == SENTINEL).all()
        assert np.array_equal(runs[0][3], with_ligand.sum(0))


def test_full_masks_are_the_uncropped_operators():
    """Every bit of every mask set: the cropped layout is the uncropped one, and all five outputs of both operators are
    the uncropped operators' on the same tables, bit for bit."""
    from pointvs_amd import functional as PF
    from tests.test_gpu_contact_attention import N_REC, _hand_built
    rowptr, etype, att, node_ptr, lig_ptr, _ = _hand_built()
    n_slots, n_nodes = len(node_ptr) - 1, len(rowptr) - 1
    keep = np.stack([mask_words(np.ones(N_REC, dtype=bool))] * n_slots)
    y = np.random.default_rng(3).standard_normal((n_nodes, 4)).astype(np.float32)
    d = [torch.from_numpy(a).cuda() for a in (rowptr, etype, att, node_ptr, lig_ptr)]
    keep_dev, y_dev = torch.from_numpy(keep.view(np.int64)).cuda(), torch.from_numpy(y).cuda()
    lig_room = n_nodes - n_slots * N_REC

    def fresh():
        return (torch.full((lig_room,), SENTINEL).cuda(), torch.full((n_slots, N_REC), SENTINEL).cuda()
                ) + PF.new_contact_accumulators(N_REC, 'cuda')
    for _ in range(2):      # (the second round on accumulators of their own again: two calls each)
        want, got = fresh(), fresh()
        for _ in range(2):
            PF.contact_attention(*d, N_REC, out=want)
            PF.contact_attention_cropped(*d[:5], keep_dev, N_REC, out=got)
        for name, g, w in zip(NAMES, got, want):
            assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), name
    assert int(want[3].max()) >= 3
    for column, n_mean in COLUMNS:
        want, got = fresh(), fresh()
        PF.slot_node_values(y_dev, d[3], d[4], N_REC, column, n_mean, out=want)
        PF.slot_node_values_cropped(y_dev, d[3], d[4], keep_dev, N_REC, column, n_mean, out=got)
        for name, g, w in zip(NAMES, got, want):
            assert g.cpu().numpy().tobytes() == w.cpu().numpy().tobytes(), (name, column, n_mean)
    # without out: lig_room rows of NaN behind the ligand atoms
    alloc = PF.contact_attention_cropped(*d[:5], keep_dev, N_REC, lig_room=lig_room)
    n = int(lig_ptr[-1])
    assert alloc[0].shape == (lig_room,) and bool(torch.isnan(alloc[0][n:]).all())
    assert alloc[0][:n].cpu().numpy().tobytes() == PF.contact_attention(*d, N_REC)[0][:n].cpu().numpy().tobytes()
    alloc = PF.slot_node_values_cropped(y_dev, d[3], d[4], keep_dev, N_REC, lig_room=lig_room + 3)
    assert alloc[0].shape == (lig_room + 3,) and alloc[1].shape == (n_slots, N_REC) and bool((alloc[3] == 5).all())
    # no slots: nothing to do
    empty = torch.zeros(1, dtype=torch.int32).cuda()
    out = PF.contact_attention_cropped(*d[:3], empty, empty, keep_dev[:0], N_REC, lig_room=0)
    assert out[1].shape == (0, N_REC) and not out[3].any() and bool(torch.isnan(out[4]).all())


def test_wrappers_refuse_wrong_arguments():
    from pointvs_amd import functional as PF
    b = _prepared('wide')
    d, n_rec, n_slots = b['dev'], b['n_rec'], len(b['node_ptr']) - 1
    graph = (d['rowptr'], d['etype'], d['att'])
    tables = (d['node_ptr'], d['lig_ptr'], d['keep'])

    def out(lig=b['lig_room'], slots=n_slots, rec=n_rec, sum_dtype=torch.float64):
        return (torch.zeros(lig).cuda(), torch.zeros((slots, n_rec)).cuda(), torch.zeros(rec, dtype=sum_dtype).cuda(),
                torch.zeros(n_rec, dtype=torch.int32).cuda(), torch.zeros(n_rec).cuda())
    with pytest.raises(ValueError, match='give lig_room'):
        PF.contact_attention_cropped(*graph, *tables, n_rec)
    with pytest.raises(ValueError, match='give lig_room'):
        PF.slot_node_values_cropped(d['y'], *tables, n_rec)
    with pytest.raises(TypeError):
        PF.contact_attention_cropped(d['rowptr'], d['etype'], d['att'].double(), *tables, n_rec, lig_room=9)
    with pytest.raises(TypeError):
        PF.slot_node_values_cropped(d['y'].double(), *tables, n_rec, lig_room=9)
    with pytest.raises(ValueError):
        PF.contact_attention_cropped(d['rowptr'].long(), d['etype'], d['att'], *tables, n_rec, lig_room=9)
    with pytest.raises(ValueError):
        PF.contact_attention_cropped(d['rowptr'], d['etype'], d['att'][:-6], *tables, n_rec, lig_room=9)
    for bad_keep in (d['keep'].int(), d['keep'][:, :2], d['keep'][:-1], d['keep'].t().contiguous().t()):
        with pytest.raises(ValueError, match='keep is a contiguous int64 tensor'):
            PF.contact_attention_cropped(*graph, d['node_ptr'], d['lig_ptr'], bad_keep, n_rec, lig_room=9)
        with pytest.raises(ValueError, match='keep is a contiguous int64 tensor'):
            PF.slot_node_values_cropped(d['y'], d['node_ptr'], d['lig_ptr'], bad_keep, n_rec, lig_room=9)
    with pytest.raises(ValueError, match='keep is a contiguous int64 tensor'):
        PF.slot_node_values_cropped(d['y'], *tables, n_rec + 64, lig_room=9)             # another word count
    with pytest.raises(ValueError, match='node_ptr and lig_ptr'):
        PF.slot_node_values_cropped(d['y'], d['node_ptr'], d['lig_ptr'][:-1], d['keep'], n_rec, lig_room=9)
    for column, n_mean in ((4, 1), (2, 3), (-1, 1), (0, 2)):
        with pytest.raises(ValueError, match='one column or the mean of three'):
            PF.slot_node_values_cropped(d['y'], *tables, n_rec, column, n_mean, lig_room=9)
    for bad in (out(slots=n_slots - 1), out(rec=n_rec - 1), out(sum_dtype=torch.float32)):
        with pytest.raises(ValueError, match='out ='):
            PF.contact_attention_cropped(*graph, *tables, n_rec, out=bad)
        with pytest.raises(ValueError, match='out ='):
            PF.slot_node_values_cropped(d['y'], *tables, n_rec, out=bad)
    with pytest.raises(ValueError, match='out ='):
        PF.contact_attention_cropped(*graph, *tables, n_rec, lig_room=b['lig_room'], out=out(lig=b['lig_room'] - 1))
    with pytest.raises(RuntimeError):
        PF.contact_attention_cropped(*(t.cpu() for t in graph + tables), n_rec, lig_room=b['lig_room'])
    with pytest.raises(RuntimeError):
        PF.slot_node_values_cropped(d['y'], *tables, n_rec, out=tuple(t.cpu() for t in out()))
    PF.contact_attention_cropped(*graph, *tables, n_rec, out=out())                      # (the sizes above: fine)
    PF.slot_node_values_cropped(d['y'], *tables, n_rec, out=out())


# ---------------------------------------------------------------- parity with the fp64 oracle

def _sweep(model, rec, rec_feats, capture, crop, batch_size=3, **kw):
    from pointvs_amd.screening import ScreeningSweep
    return ScreeningSweep(model.cuda(), rec.cuda(), rec_feats, RADIUS, batch_size=batch_size, capture=capture,
                          crop_radius=crop, cropped_hotspots=True, **kw)


def _check_map(out, want, bound, what):
    assert out['count'].dtype == torch.int32 and out['mean'].dtype == torch.float64
    count = out['count'].cpu().numpy()
    print(f'{what}: count sum {int(count.sum())} on {int((count > 0).sum())} atoms')
    assert np.array_equal(count, want['count'])
    assert out['per_hit'].shape == want['per_hit'].shape and list(out['ligand']) == list(want['ligand'])
    for name, values in out['ligand'].items():
        _close(values.cpu().numpy(), want['ligand'][name], bound, f'{what} ligand {name}')
    _close(out['per_hit'].cpu().numpy(), want['per_hit'], bound, f'{what} per_hit')
    _close(out['mean'].cpu().numpy(), want['mean'], bound, f'{what} mean')
    _close(out['max'].cpu().numpy(), want['max'], bound, f'{what} max')


@pytest.mark.parametrize('capture', [pytest.param(True, marks=needs_caching_allocator), False], ids=['captured', 'eager'])
@pytest.mark.parametrize('crop', ref.CROPS)
@pytest.mark.parametrize('which', [1, -1, 'cam'])
def test_parity_with_the_fp64_oracle(which, crop, capture):
    """Hits of 1, 12, 12 and 70 atoms at batch 3. At 7.0 they keep 26, 89, 104 and 149 of 150 atoms; at 4.0, below the
    edge radius of 6, they keep 0, 19, 6 and 100 and lose contacts."""
    y = ref.sweep_yardstick()
    sweep = _sweep(y['model'], y['rec'], y['rec_feats'], capture, crop)
    what = f'{which} crop {crop:g} capture={capture}'
    if which == 'cam':
        want, bound = y['cam'][crop], y['cam_bound'][crop]
        out = sweep.receptor_hotspots(y['items'], attribution='cam', per_hit=True)
        screen = sweep.cam_screen
        assert screen.cam is not None and screen.contact is None and sweep.hotspot is None
    else:
        layer = 3 if which == -1 else which
        want, bound = y['att'][crop][layer], y['att_bound'][crop][layer]
        out = sweep.receptor_hotspots(y['items'], gnn_layer=which, per_hit=True)
        screen = sweep.hotspot
        assert screen.contact_attention == layer and screen.cam is None and sweep.cam_screen is None
    assert screen.crop_radius == crop and screen.cropped_maps and screen._captured == capture
    assert sweep.batches_run == 1 + 2                      # the sizing batch, then ceil(4 / 3) steps
    _check_map(out, want, bound, what)
    kept = (~np.isnan(y['cam'][crop]['per_hit']))
    assert np.isnan(out['per_hit'].cpu().numpy()[~kept]).all()
    assert kept.sum(1).tolist() == y['kept'][crop]
    if which == 'cam':
        assert np.array_equal(out['count'].cpu().numpy(), kept.sum(0))


def _cropped_edges(feats, pose, rec, rec_feats, crop):
    """(x, pos, kept, edge_index, edge_attr one-hot) of a hit's cropped complex, the oracle's edge list."""
    from oracle.generate_edges_oracle import generate_edges
    x, pos, kept = cropped_complex(feats.numpy(), pose.numpy(), rec_feats.numpy(), rec.numpy(), crop)
    _, (rows, cols), attrs = generate_edges(pos, x[:, -1], RADIUS, RADIUS, prune=False)
    return (torch.from_numpy(x), torch.from_numpy(pos), kept, rows, attrs,
            torch.from_numpy(np.vstack([rows, cols])).long(), torch.nn.functional.one_hot(torch.from_numpy(attrs).long(), 3))


def test_parity_with_the_per_complex_route():
    """pointvs_amd.attribution.edge_attention / cam, one cropped complex per call on the oracle's edge list."""
    from pointvs_amd import attribution
    y = ref.sweep_yardstick()
    crop = 7.0
    sweep = _sweep(y['model'], y['rec'], y['rec_feats'], False, crop)
    maps = {layer: sweep.receptor_hotspots(y['items'], gnn_layer=layer, per_hit=True) for layer in (1, 3)}
    cams = sweep.receptor_hotspots(y['items'], attribution='cam', per_hit=True)
    model = y['model'].cuda()
    for i, (name, feats, pose) in enumerate(y['items']):
        x, pos, kept, rows, attrs, edge_index, edge_attr = _cropped_edges(feats, pose, y['rec'], y['rec_feats'], crop)
        n = int(pose.shape[0])
        for layer in (1, 3):
            att = attribution.edge_attention(model, pos[None], x[None], edge_indices=edge_index, edge_attrs=edge_attr,
                                             gnn_layer=layer)
            top = np.full(len(x), -np.inf)
            np.maximum.at(top, rows[attrs == 1], np.asarray(att, dtype=np.float64)[attrs == 1])
            top[np.isinf(top)] = np.nan
            got = np.concatenate([maps[layer]['ligand'][name].cpu().numpy(), maps[layer]['per_hit'][i].cpu().numpy()[kept]])
            _close(got, top, y['att_bound'][crop][layer], f'attribution.edge_attention layer {layer} {name}')
        one = attribution.cam(model, pos[None], x[None], edge_indices=edge_index, edge_attrs=edge_attr)
        got = np.concatenate([cams['ligand'][name].cpu().numpy(), cams['per_hit'][i].cpu().numpy()[kept]])
        _close(got, one.reshape(-1), y['cam_bound'][crop], f'attribution.cam {name}')
        assert len(got) == n + len(kept)


# ---------------------------------------------------------------- other models

def test_graphnorm_model_needs_the_padded_statistics():
    """GraphNorm takes its statistics over the batch's nodes: with padded_graphnorm=True and one hit per step they are
    the one complex's, so the oracle's one graph per forward is the yardstick; without the keyword: a cropped screen's
    refusal."""
    items, rec, rec_feats = hits_and_receptor()
    items = items[:3]
    model = attention_model(32, graphnorm=True)
    cfg = dict(KW, edge_attention=True, num_layers=3, graphnorm=True, _class='SartorrasEGNN')
    want, bound = ref.hotspot_pair(model, cfg, items, rec, rec_feats, RADIUS, 7.0, (3,))
    sweep = _sweep(model, rec, rec_feats, False, 7.0, batch_size=1, padded_graphnorm=True)
    out = sweep.receptor_hotspots(items, gnn_layer=-1, per_hit=True)
    assert sweep.hotspot.graphnorm and sweep.hotspot._gn_padded and sweep.batches_run == 1 + 3
    _check_map(out, want[3], bound[3], 'graphnorm layer -1')
    want, bound = ref.cam_pair(model, cfg, items, rec, rec_feats, RADIUS, 7.0)
    _check_map(sweep.receptor_hotspots(items, attribution='cam', per_hit=True), want, bound, 'graphnorm cam')
    with pytest.raises(ValueError, match='a GraphNorm model needs padded_graphnorm=True'):
        _sweep(model, rec, rec_feats, False, 7.0, batch_size=1).receptor_hotspots(items)


@pytest.mark.parametrize('gnn_layer', [1, -1])
def test_softmax_attention_model_without_the_reuse(gnn_layer):
    """A cropped step runs every layer whole, so its attention is normalised over all edges of a row as it is: no
    softmax_reuse needed."""
    items, rec, rec_feats = hits_and_receptor()
    model = attention_model(6, softmax_attention=True)
    cfg = dict(KW, edge_attention=True, num_layers=3, softmax_attention=True, _class='SartorrasEGNN')
    layer = 3 if gnn_layer == -1 else gnn_layer
    want, bound = ref.hotspot_pair(model, cfg, items, rec, rec_feats, RADIUS, 7.0, (layer,))
    sweep = _sweep(model, rec, rec_feats, False, 7.0)
    assert not sweep.softmax_reuse
    out = sweep.receptor_hotspots(items, gnn_layer=gnn_layer, per_hit=True)
    _check_map(out, want[layer], bound[layer], f'softmax attention layer {gnn_layer}')
    top = float(np.nanmax(out['per_hit'].cpu().numpy()))
    assert 0 < top <= 1


def test_two_headed_model_takes_a_column():
    from tests.test_gpu_two_head_screen import KW as KW2, _model
    items, rec, rec_feats = hits_and_receptor()
    flags = dict(k=32, num_layers=2, dim_output=3, final_softplus=True)
    model = _model(3, **flags)
    cfg = dict(KW2, **flags, _class='MultitaskSatorrasEGNN')
    for column in (0, 2):
        want, bound = ref.cam_pair(model, cfg, items, rec, rec_feats, RADIUS, 7.0, column=column, tasks='both')
        sweep = _sweep(model, rec, rec_feats, False, 7.0, tasks='both')
        out = sweep.receptor_hotspots(items, attribution='cam', column=column, per_hit=True)
        assert sweep.cam_screen.cam['node_y'].shape[1] == 4 and sweep.cam_screen.cropped_maps
        _check_map(out, want, bound, f'two heads, column {column}')
    with pytest.raises(ValueError, match='name a column'):
        _sweep(model, rec, rec_feats, False, 7.0, tasks='both').receptor_hotspots(items, attribution='cam')


# ---------------------------------------------------------------- accumulator hygiene, end to end, the keywords off

@needs_caching_allocator
@pytest.mark.parametrize('attribution', ['edge_attention', 'cam'])
def test_nothing_leaks_into_the_accumulators(attribution):
    """A fresh sweep: the sizing batch, the capture (two warm-up steps and the captured one), then the run: the counts
    are the oracle's, and a second call on the same sweep gives the same bytes."""
    y = ref.sweep_yardstick()
    by_cam = attribution == 'cam'
    want = y['cam'][7.0] if by_cam else y['att'][7.0][1]
    sweep = _sweep(y['model'], y['rec'], y['rec_feats'], True, 7.0)
    first = sweep.receptor_hotspots(y['items'], attribution=attribution, per_hit=True)
    screen = sweep.cam_screen if by_cam else sweep.hotspot
    assert sweep.batches_run == 3 and screen._captured
    again = sweep.receptor_hotspots(y['items'], attribution=attribution, per_hit=True)
    assert (sweep.cam_screen if by_cam else sweep.hotspot) is screen and sweep.batches_run == 5
    assert np.array_equal(first['count'].cpu().numpy(), want['count']) and int(want['count'].sum()) > 0
    for key in ('mean', 'count', 'max', 'per_hit'):
        assert first[key].cpu().numpy().tobytes() == again[key].cpu().numpy().tobytes(), key
    for name in first['ligand']:
        assert first['ligand'][name].cpu().numpy().tobytes() == again['ligand'][name].cpu().numpy().tobytes()
    eager = _sweep(y['model'], y['rec'], y['rec_feats'], False, 7.0).receptor_hotspots(y['items'], attribution=attribution)
    assert torch.equal(eager['count'], first['count']) and 'per_hit' not in eager
    none = sweep.receptor_hotspots([], attribution=attribution, per_hit=True)
    assert bool(torch.isnan(none['mean']).all()) and bool(torch.isnan(none['max']).all()) and not none['count'].any()
    assert none['ligand'] == {} and none['per_hit'].shape == (0, N_REC_SCREEN)


@needs_caching_allocator
def test_end_to_end_after_a_cropped_run_library(tmp_path):
    """A cropped run_library with a hits file, then both maps of every hit: best_poses goes straight in."""
    from pointvs_amd.screening import ScreeningSweep
    lig, rec, lig_feats, rec_feats = _set(8102, 70)
    work = _library(lig, lig_feats)
    sweep = ScreeningSweep(attention_model(5).cuda(), rec.cuda(), rec_feats, edge_radius=RADIUS, batch_size=4,
                           crop_radius=7.0, cropped_hotspots=True)
    sweep.run_library(work, hits_file=tmp_path / 'hits.txt')
    assert sweep.hits['ligNone'][0] == -1 and sweep.library.crop_radius == 7.0 and not sweep.library.cropped_maps
    sizes = {'ligA': 12, 'ligB': 9, 'ligC': 70, 'ligD': 12, 'ligE': 1}
    before = sweep.batches_run
    out = sweep.receptor_hotspots(sweep.best_poses(work), scores_file=tmp_path / 'hotspots.txt',
                                  ligand_scores_file=tmp_path / 'ligand.txt')
    assert sweep.batches_run - before == 1 + -(-len(sizes) // 4) and 'per_hit' not in out
    assert {name: int(v.shape[0]) for name, v in out['ligand'].items()} == sizes
    assert sweep.hotspot.max_lig_atoms == 70 and sweep.hotspot._captured and sweep.hotspot.cropped_maps
    assert sweep.library.contact is None and sweep.library.cam is None
    mean, count = out['mean'].cpu().numpy(), out['count'].cpu().numpy()
    assert mean.dtype == np.float64 and 0 < int((count > 0).sum()) < N_REC_SCREEN and int(count.max()) <= len(sizes)
    assert np.array_equal(np.isnan(mean), count == 0)
    lines = (tmp_path / 'hotspots.txt').read_text().splitlines()
    atoms = np.nonzero(count > 0)[0]
    assert len(lines) == len(atoms)
    for line, j in zip(lines, atoms):
        assert re.fullmatch(r'\d\.\d{6} \d+ \| receptor atom\d+', line), line
        assert line == f'{mean[j]:.6f} {count[j]} | receptor atom{j}'
    lines = (tmp_path / 'ligand.txt').read_text().splitlines()
    want = [(name, a, float(out['ligand'][name][a])) for name in out['ligand'] for a in range(sizes[name])]
    assert len(lines) == sum(sizes.values())
    for line, (name, a, v) in zip(lines, want):
        assert re.fullmatch(r'(nan|-?\d+\.\d{6}) \| receptor \w+_atom\d+', line), line
        assert line == f'{v:.6f} | receptor {name}_atom{a}'
    # the CAM of the same hits: an atom counts in the hits that keep it
    before = sweep.batches_run
    cam = sweep.receptor_hotspots(sweep.best_poses(work), attribution='cam', scores_file=tmp_path / 'cam.txt', per_hit=True)
    assert sweep.batches_run - before == 1 + -(-len(sizes) // 4)
    kept = ~torch.isnan(cam['per_hit'])
    assert torch.equal(cam['count'], kept.sum(0).int()) and int(cam['count'].min()) < int(cam['count'].max()) <= 5
    lines = (tmp_path / 'cam.txt').read_text().splitlines()
    assert len(lines) == int((cam['count'] > 0).sum())
    for line in lines:
        assert re.fullmatch(r'-?\d+\.\d{6} \d+ \| receptor atom\d+', line), line


def test_the_keywords_off():
    """Without the keywords everything raises what it raises today, and a screen built with cropped_maps=True but no map
    scores the bits of one built without it."""
    from pointvs_amd.screening import LibraryScreen, ScreeningSweep
    items, rec, rec_feats = hits_and_receptor()
    model = attention_model(31).cuda()
    for kw in (dict(cam=True), dict(contact_attention=1)):
        name = next(iter(kw))
        with pytest.raises(ValueError, match=rf'LibraryScreen\(crop_radius=\.\.\., {name}=\.\.\.\): the {name} path assumes '
                                             r'n_rec receptor rows in every slot, and a cropped slot has those inside the '
                                             r'radius; use two screens'):
            LibraryScreen(model, rec.cuda(), rec_feats, 3, 70, RADIUS, crop_radius=7.0, **kw)
    with pytest.raises(ValueError, match=r'crop_radius=\.\.\., struck=\.\.\.\): the struck path assumes'):
        LibraryScreen(model, rec.cuda(), rec_feats, 3, 70, RADIUS, crop_radius=7.0, cropped_maps=True, struck=True)
    for kw in (dict(), dict(cropped_attribution=True)):
        sweep = ScreeningSweep(model, rec.cuda(), rec_feats, RADIUS, batch_size=3, capture=False, crop_radius=7.0, **kw)
        with pytest.raises(NotImplementedError, match=r'ScreeningSweep\(crop_radius=\.\.\.\)\.receptor_hotspots: the '
                                                      r'reference masks after cropping around the WHOLE ligand, so a copy '
                                                      r'must not be cropped again around what is left of it - and the '
                                                      r'attention and CAM reductions assume n_rec receptor rows per slot\. '
                                                      r'Not built yet: use a sweep without crop_radius'):
            sweep.receptor_hotspots(items[:1])
    slots = [(f, p) for _, f, p in items[:3]]
    plain = LibraryScreen(model, rec.cuda(), rec_feats, 3, 70, RADIUS, crop_radius=7.0)
    keyword = LibraryScreen(model, rec.cuda(), rec_feats, 3, 70, RADIUS, crop_radius=7.0, cropped_maps=True)
    mapped = LibraryScreen(model, rec.cuda(), rec_feats, 3, 70, RADIUS, crop_radius=7.0, cropped_maps=True, cam=True,
                           contact_attention=-1)
    assert keyword.cam is None and keyword.contact is None and keyword._h_final is None
    a, b, c = plain(slots), keyword(slots), mapped(slots)
    assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes() == c.cpu().numpy().tobytes()
    assert torch.equal(plain.keep, mapped.keep)
    kept = ref.kept_counts(items[:3], rec, rec_feats, 7.0)
    assert (~torch.isnan(mapped.cam['slot_rec_val'])).sum(1).tolist() == kept
    assert int(mapped.cam['rec_count'].sum()) == sum(kept) and int(mapped.contact['rec_count'].sum()) > 0
    with pytest.raises(RuntimeError, match='without cam'):
        keyword.reset_cam()
    mapped.reset_cam()
    mapped.reset_contact_attention()
    assert not mapped.cam['rec_count'].any() and not mapped.contact['rec_count'].any()
