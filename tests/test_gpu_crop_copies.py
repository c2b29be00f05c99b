"""Cropped copies on the device: pvs_screen_copies_build (LibraryScreen(crop_radius=..., crop_parents=True)),
pvs_crop_keep, pvs_leave_out_parent_pack and the three masking methods of ScreeningSweep(cropped_attribution=True).
The builder is checked exactly - masks, node tables and the CSR against tests/_crop_copies_ref.py and the oracle's
generate_edges on the reference copy, through the comparison helpers of tests/test_gpu_screen_crop.py -, array for array
against pvs_screen_slots_build(PVS_SLOTS_CROPPED) where the crop table is the ligand table, the scores against the plain
forward on the reference copies and against pointvs_amd.attribution one complex at a time.

Bounds (tests/test_gpu_contact_masking.py, tests/test_gpu_ligand_masking.py): each raw output of a screening route is
within 1e-5 * max|raw| of the plain forward; a difference of two outputs of one route within 4e-5 * max|raw| of the
same difference of another."""
import re

import numpy as np
import pytest
import torch

from tests import _crop_copies_ref as cref
from tests import _crop_ref as ref
from tests._golden import needs_caching_allocator
from tests.test_gpu_screen_crop import KW, N_REC, _assert_exact, _model, _oracle_items, _set

pytestmark = pytest.mark.gpu

ARRAYS = ('rowptr', 'row', 'col', 'etype', 'inv_deg', 'keep', 'node_ptr', 'node_graph', 'pos', 'x')


def _line(n_rec=N_REC, seed=5):
    """Receptor atoms at (j, 0, 0): exactly representable coordinates, three mask words with the last one partial."""
    rng = np.random.default_rng(seed)
    rec = torch.zeros((n_rec, 3))
    rec[:, 0] = torch.arange(n_rec, dtype=torch.float32)
    rec_feats = torch.from_numpy(rng.random((n_rec, 12)).astype(np.float32))
    rec_feats[:, -1] = 1
    return rec, rec_feats, rng


def _atoms(rng, xs, y=0.0):
    pose = torch.zeros((len(xs), 3))
    pose[:, 0] = torch.tensor(list(xs), dtype=torch.float32)
    pose[:, 1] = y
    feats = torch.from_numpy(rng.random((len(xs), 12)).astype(np.float32))
    feats[:, -1] = 0
    return feats, pose


def _load_copies(screen, slots, parents, drops):
    """The slots loaded as they are, then the crop table and rec_drop of the screen overwritten with the parents'."""
    screen.load(slots)
    ptr = np.concatenate([[0], np.cumsum([p.shape[0] for p in parents])]).astype(np.int32)
    screen.crop_ptr.copy_(torch.from_numpy(ptr))
    packed = torch.cat([p.reshape(-1, 3) for p in parents], 0)
    screen.crop_pos[:packed.shape[0]].copy_(packed)
    screen.rec_drop.copy_(torch.tensor(drops, dtype=torch.int32))
    return screen


def _complexes(slots, parents, drops, rec, rec_feats, crop):
    out = []
    for (feats, pose), parent, drop in zip(slots, parents, drops):
        x, pos, kept = cref.copy_complex(feats.numpy(), pose.numpy(), rec_feats.numpy(), rec.numpy(), crop,
                                         rec_drop=drop, parent_pos=parent.numpy())
        out.append((torch.from_numpy(x), torch.from_numpy(pos).reshape(-1, 3), kept))
    return out


def test_builder_is_exact_on_a_line():
    """Crop radius 5, edge radius 2.5. Parents of 1, 2 and 65 atoms; slots that hold their parent without the one atom
    that alone keeps some receptor atoms (they stay); an empty slot with an empty crop set; a ligand alone (empty crop
    set); rec_drop at bits 0, 63, 64 and n_rec - 1, on an atom that is not kept, and -1."""
    from pointvs_amd.screening import LibraryScreen
    crop, r_edge = 5.0, 2.5
    rec, rec_feats, rng = _line()
    one = _atoms(rng, [10.0])
    two = _atoms(rng, [30.0, 33.0])
    wide = _atoms(rng, [40.0 + 0.5 * i for i in range(64)] + [75.0], y=1.0)
    low, mid, high = _atoms(rng, [2.0]), _atoms(rng, [61.0, 66.0]), _atoms(rng, [127.0])
    alone = _atoms(rng, [100.0])
    none = (one[0][:0], one[1][:0])
    cut = lambda hit, a: tuple(t[[i for i in range(t.shape[0]) if i != a]].contiguous() for t in hit)      # noqa: E731
    #        slot            cropped around  rec_drop
    cases = [(one,           one[1],         -1),
             (cut(two, 1),   two[1],         -1),
             (cut(wide, 64), wide[1],        -1),
             (none,          none[1],        -1),
             (alone,         none[1],        -1),
             (low,           low[1],         0),
             (mid,           mid[1],         63),
             (cut(mid, 0),   mid[1],         64),
             (high,          high[1],        N_REC - 1),
             (one,           one[1],         50),
             (cut(two, 0),   two[1],         31)]
    slots, parents, drops = ([c[k] for c in cases] for k in range(3))
    complexes = _complexes(slots, parents, drops, rec, rec_feats, crop)
    kept = [k.tolist() for _, _, k in complexes]
    assert kept[0] == list(range(6, 15)) == kept[9]                                   # (atom 50 was never kept)
    assert kept[1] == list(range(26, 38)) and not ref.keep_mask(slots[1][1].numpy(), rec.numpy(), crop)[35:38].any()
    assert kept[2][-3:] == [77, 78, 79] and not ref.keep_mask(slots[2][1].numpy(), rec.numpy(), crop)[77:80].any()
    assert kept[3] == [] and kept[4] == [] and complexes[4][0].shape[0] == 1
    assert kept[5] == list(range(1, 7)) and kept[6] == [j for j in range(57, 71) if j != 63]
    assert kept[7] == [j for j in range(57, 71) if j != 64] and kept[8] == list(range(123, 129))
    assert kept[10] == [j for j in range(26, 38) if j != 31]
    screen = LibraryScreen(_model(), rec.cuda(), rec_feats, len(cases), 65, r_edge, crop_radius=crop, crop_parents=True)
    f = _load_copies(screen, slots, parents, drops)._build()
    screen.check()
    torch.cuda.synchronize()
    _assert_exact(screen, f, slots, complexes, r_edge, None)
    again = {k: f[k].clone() for k in ARRAYS}
    screen._build()                                        # no atomics: the same bits on every run
    screen.check()
    assert all(torch.equal(f[k], v) for k, v in again.items())


def _wide_case():
    """A 1,024-atom parent (a 32 x 32 grid, 3 apart, in the plane x = 35; its last atom at (60, 0, 1) alone keeps the
    receptor atoms around 60) against 70 receptor atoms on a line; the slot holds the parent without that atom. Beside
    it a two-atom ligand cropped around itself."""
    rec, rec_feats, rng = _line(70)
    g = (torch.arange(32, dtype=torch.float32) - 15.5) * 3.0
    pose = torch.stack([torch.full((1024,), 35.0), g.repeat_interleave(32), g.repeat(32)], 1)
    pose[1023] = torch.tensor([60.0, 0.0, 1.0])
    feats = torch.from_numpy(rng.random((1024, 12)).astype(np.float32))
    feats[:, -1] = 0
    small = _atoms(rng, [5.0, 6.5], y=0.5)
    slots = [(feats[:1023].contiguous(), pose[:1023].contiguous()), small]
    return rec, rec_feats, slots, [pose, small[1]], [-1, 6]


def test_builder_with_a_1024_atom_parent():
    from pointvs_amd.screening import LibraryScreen
    crop, r_edge = 5.0, 2.5
    rec, rec_feats, slots, parents, drops = _wide_case()
    complexes = _complexes(slots, parents, drops, rec, rec_feats, crop)
    own = ref.keep_mask(slots[0][1].numpy(), rec.numpy(), crop)
    assert own.any() and complexes[0][2].tolist() == sorted(set(np.flatnonzero(own)) | set(range(56, 65)))
    assert not own[56:65].any() and 6 not in complexes[1][2] and 5 in complexes[1][2]
    screen = LibraryScreen(_model(), rec.cuda(), rec_feats, 2, 1024, r_edge, crop_radius=crop, crop_parents=True)
    f = _load_copies(screen, slots, parents, drops)._build()
    screen.check()
    torch.cuda.synchronize()
    _assert_exact(screen, f, slots, complexes, r_edge, None)


def _random_slots(lig, lig_feats, sizes, seed):
    from pointvs_amd.synthetic import random_poses
    return [(lig_feats[:n].roll(k, 0).contiguous(),
             random_poses(lig[:n], 1, seed=seed + k, max_shift=3.0)[0].contiguous() if n else lig[:0])
            for k, n in enumerate(sizes)]


def test_the_ligand_table_as_crop_table_gives_the_cropped_layout_array_for_array():
    """crop_pos / crop_ptr = the ligand table with rec_drop all -1 (a plain load of a crop_parents screen) and with
    rec_drop NULL (the job built by hand): every output array of pvs_screen_slots_build(PVS_SLOTS_CROPPED)."""
    from pointvs_amd import _lib
    from pointvs_amd import functional as PF
    from pointvs_amd.screening import LibraryScreen
    lig, rec, lig_feats, rec_feats = _set(6001)
    slots = _random_slots(lig, lig_feats, (1, 64, 0, 7, 33, 20), 10)
    for r_inter, r_intra, crop in ((7.0, None, 8.0), (6.0, 2.5, 5.0)):
        plain = LibraryScreen(_model(), rec.cuda(), rec_feats, len(slots), 64, r_inter, r_intra, crop_radius=crop)
        want = plain.load(slots)._build()
        plain.check()
        e = int(want['rowptr'][plain.n_cap])
        assert e > 0 and bool(want['keep'].any()) and not bool((want['keep'] == -1).all())
        screen = LibraryScreen(_model(), rec.cuda(), rec_feats, len(slots), 64, r_inter, r_intra, crop_radius=crop,
                               crop_parents=True)
        f = screen.load(slots)._build()
        screen.check()
        assert f['cap'] == want['cap'] and bool((screen.rec_drop == -1).all())
        assert torch.equal(screen.crop_ptr, screen.lig_ptr)

        def same(f):
            for k in ARRAYS:
                n = e if k in ('row', 'col', 'etype') else None
                assert torch.equal(f[k][:n], want[k][:n]), (k, crop)
        same(f)
        for k in ARRAYS:                                   # rec_drop NULL, into poisoned outputs
            f[k].fill_(1)
        job = _lib.PvsScreenCopiesJob(slots=screen._job(f), crop_pos=_lib.ptr(screen.lig_pos),
                                      crop_ptr=_lib.ptr(screen.lig_ptr), rec_drop=None, crop_cap=screen.l_cap)
        assert PF.screen_copies_state_bytes(job) == f['state'].numel()
        PF.screen_copies_build(job, f['state'])
        torch.cuda.synchronize()
        assert int(f['status']) == 0
        same(f)


@needs_caching_allocator
def test_a_crop_parents_screen_on_plain_batches_gives_the_cropped_screens_bits():
    """Eager and captured, on three compositions: the scores of a crop_parents=False screen, bit for bit."""
    from pointvs_amd.screening import LibraryScreen
    lig, rec, lig_feats, rec_feats = _set(6004)
    model = _model(2, num_layers=3, residual=True, edge_attention=True, tanh=True)
    batches = [_random_slots(lig, lig_feats, sizes, 70 + 10 * k) for k, sizes in enumerate([(7, 20, 3), (5, 17, 1), (12, 9)])]
    args = (model, rec.cuda(), rec_feats, 3, 20, 7.0)
    plain = LibraryScreen(*args, crop_radius=6.0)
    want = [plain(slots).reshape(-1).clone() for slots in batches]
    plain.check()
    eager = LibraryScreen(*args, crop_radius=6.0, crop_parents=True)
    for k, slots in enumerate(batches):
        assert torch.equal(eager(slots).reshape(-1), want[k]), k
        assert torch.equal(eager.keep, plain.load(batches[k])._build()['keep'])
    eager.check()
    graph = LibraryScreen(*args, crop_radius=6.0, crop_parents=True).capture(batches[0])
    for k in (2, 1, 0):
        assert torch.equal(graph.replay(batches[k]).reshape(-1), want[k]), k
    graph.check()
    assert bool(want[0].abs().sum() > 0)


def test_bad_tables_give_an_edgeless_batch_and_the_next_build_is_clean():
    from pointvs_amd.screening import LibraryScreen
    crop, r_edge = 5.0, 2.5
    rec, rec_feats, slots, parents, drops = _wide_case()
    screen = LibraryScreen(_model(), rec.cuda(), rec_feats, 2, 1024, r_edge, crop_radius=crop, crop_parents=True)
    f = _load_copies(screen, slots, parents, drops)._build()
    screen.check()
    good = {k: f[k].clone() for k in ARRAYS}
    e = int(f['rowptr'][screen.n_cap])
    assert e > 0 and screen.l_cap == 2048
    n_rec = rec.shape[0]
    bad = [('crop_ptr', [0, 1024, 1000]), ('crop_ptr', [0, 1024, 2049]), ('crop_ptr', [0, 1025, 1027]),
           ('crop_ptr', [1, 1024, 1026]), ('rec_drop', [-1, n_rec]), ('rec_drop', [-2, 6])]
    for name, table in bad:
        _load_copies(screen, slots, parents, drops)
        getattr(screen, name).copy_(torch.tensor(table, dtype=torch.int32))
        screen._launch_builder(f)
        torch.cuda.synchronize()
        assert int(f['status']) == 8, (name, table)
        assert not f['node_ptr'].any() and not f['rowptr'].any() and bool((f['node_graph'] == -1).all()), (name, table)
        assert bool((f['inv_deg'] == 1).all()) and not f['pos'].any() and not f['x'].any(), (name, table)
        with pytest.raises(ValueError, match='crop_ptr is no table of crop sets'):
            screen._raise_for(int(f['status']))
        # the next good build on the same state is clean: one writer of the status word, nothing to clear
        _load_copies(screen, slots, parents, drops)
        screen._launch_builder(f)
        torch.cuda.synchronize()
        assert int(f['status']) == 0
        for k in ARRAYS:
            n = e if k in ('row', 'col', 'etype') else None
            assert torch.equal(f[k][:n], good[k][:n]), (name, table, k)
    # a bad lig_ptr, as for every slot builder
    screen.lig_ptr.copy_(torch.tensor([0, 1023, 1000], dtype=torch.int32))
    screen._launch_builder(f)
    assert int(f['status']) == 8 and not f['rowptr'].any()


# ---------------------------------------------------------------- pvs_crop_keep, pvs_leave_out_parent_pack

def test_crop_keep_is_exact():
    from pointvs_amd import functional as PF
    rec, _, rng = _line()
    sizes = [1, 2, 0, 65, 1, 1024]
    xs = [10.0, 61.0, 66.0] + [40.0 + 0.5 * i for i in range(65)] + [200.0] + [float(i % 130) for i in range(1024)]
    pose = _atoms(rng, xs, y=3.0)[1]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    words, kept_ptr = cref.hits_keep(pose.numpy(), ptr, rec.numpy(), 5.0)
    counts = np.diff(kept_ptr).tolist()
    assert counts[0] == 7 and counts[2] == 0 and counts[4] == 0 and counts[5] == N_REC and 0 < counts[3] < N_REC
    runs = [PF.crop_keep(pose.cuda(), torch.from_numpy(ptr).cuda(), rec.cuda(), 5.0, host_ptr=True) for _ in range(2)]
    for keep, got_ptr, host in runs:
        assert np.array_equal(keep.cpu().numpy().view(np.uint64), words)
        assert got_ptr.cpu().tolist() == kept_ptr.tolist() == host.tolist()
    assert torch.equal(runs[0][0], runs[1][0])
    hit, atom = PF.kept_atoms(runs[0][0], N_REC)
    want = [(s, j) for s in range(len(sizes)) for j in np.flatnonzero(ref.words_mask(words[s], N_REC))]
    assert list(zip(hit.tolist(), atom.tolist())) == want
    # bad tables: zeros and -1 in the last entry
    for table in ([0, 1, 3, 3, 68, 67, 1093], [1, 1, 3, 3, 68, 69, 1093], [0, 1, 3, 3, 68, 69, 1094],
                  [0, 1025, 1025, 1025, 1025, 1025, 1093]):
        keep = torch.full((6, 3), -1, dtype=torch.int64).cuda()
        kept = torch.full((7,), 5, dtype=torch.int32).cuda()
        from pointvs_amd import _lib
        pose_dev, rec_dev = pose.cuda(), rec.cuda()          # (held until the launch has run)
        table_dev = torch.tensor(table, dtype=torch.int32).cuda()
        _lib.check(_lib.lib().pvs_crop_keep(_lib.ptr(pose_dev), _lib.ptr(table_dev), 6, pose.shape[0], _lib.ptr(rec_dev),
                                            N_REC, 5.0, _lib.ptr(keep), _lib.ptr(kept), None), 'pvs_crop_keep')
        torch.cuda.synchronize()
        assert kept.tolist() == [0] * 6 + [-1] and not keep.any(), table
        with pytest.raises(ValueError, match='not an ascending table'):
            PF.crop_keep(pose.cuda(), torch.tensor(table, dtype=torch.int32).cuda(), rec.cuda(), 5.0)
    with pytest.raises(TypeError, match='fp32 only'):
        PF.crop_keep(pose.cuda().double(), torch.from_numpy(ptr).cuda(), rec.cuda(), 5.0)
    keep, kept = PF.crop_keep(pose[:0].cuda(), torch.zeros(1, dtype=torch.int32).cuda(), rec.cuda(), 5.0)       # no hit
    assert keep.shape == (0, 3) and kept.tolist() == [0]


def test_parent_packer_is_exact():
    from pointvs_amd import functional as PF
    sizes = [0, 1, 2, 5, 64, 65, 130]
    total = sum(sizes)
    pos = np.arange(total * 3, dtype=np.float32).reshape(total, 3)
    lig_ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pair_ptr = np.array([0, 0, 3, 3, 4, 10, 10, 12], dtype=np.int32)
    n_slots, slot_cap, sentinel = 7, 130, -7.0

    def pack(copy_ptr, first):
        out = (torch.full((n_slots * slot_cap, 3), sentinel).cuda(),
               torch.full((n_slots + 1,), 12345, dtype=torch.int32).cuda(), torch.full((1,), 77, dtype=torch.int32).cuda())
        got = PF.leave_out_parent_pack(torch.from_numpy(pos).cuda(), torch.from_numpy(lig_ptr).cuda(),
                                       torch.from_numpy(np.asarray(copy_ptr, dtype=np.int32)).cuda(),
                                       torch.tensor([first], dtype=torch.int32).cuda(), n_slots, slot_cap, out=out)
        assert all(g is o for g, o in zip(got, out))
        return tuple(t.cpu().numpy() for t in got)

    for copy_ptr in (lig_ptr, pair_ptr):                    # both numberings: ligand-atom copies, pair copies
        copies = int(copy_ptr[-1]) + len(sizes)
        firsts = list(range(0, copies, n_slots)) + [3, copies - 2, copies + 6]      # mid-hit, past the last hit, empty
        for first in firsts:
            want_pos, want_ptr = cref.parent_pack(pos, lig_ptr, copy_ptr, first, n_slots)
            got_pos, got_ptr, status = pack(copy_ptr, first)
            assert status[0] == 0 and np.array_equal(got_ptr, want_ptr), (first, got_ptr, want_ptr)
            n = int(want_ptr[-1])
            assert got_pos[:n].tobytes() == want_pos.tobytes() and bool((got_pos[n:] == sentinel).all()), first
            again = pack(copy_ptr, first)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (got_pos, got_ptr, status)))
        assert not pack(copy_ptr, copies + 6)[1].any()
    # bad tables: status 8, out_ptr zeros, nothing written
    bad_lig = lig_ptr.copy()
    bad_lig[3] = 0
    for lp, cp in ((bad_lig, bad_lig), (lig_ptr, [0, 0, 3, 2, 4, 10, 10, 12]), (lig_ptr, [1, 1, 3, 3, 4, 10, 10, 12])):
        out = (torch.full((n_slots * slot_cap, 3), sentinel).cuda(),
               torch.full((n_slots + 1,), 12345, dtype=torch.int32).cuda(), torch.full((1,), 77, dtype=torch.int32).cuda())
        PF.leave_out_parent_pack(torch.from_numpy(pos).cuda(), torch.from_numpy(np.asarray(lp, dtype=np.int32)).cuda(),
                                 torch.tensor(np.asarray(cp), dtype=torch.int32).cuda(),
                                 torch.tensor([2], dtype=torch.int32).cuda(), n_slots, slot_cap, out=out)
        assert int(out[2]) == 8 and not out[1].any() and bool((out[0] == sentinel).all())
    # a hit wider than slot_cap
    out = PF.leave_out_parent_pack(torch.from_numpy(pos).cuda(), torch.from_numpy(lig_ptr).cuda(),
                                   torch.from_numpy(lig_ptr).cuda(), torch.zeros(1, dtype=torch.int32).cuda(), 4, 129)
    assert int(out[2]) == 8 and not out[1].any()


# ---------------------------------------------------------------- scores

CROP, R_EDGE = 5.0, 4.0
HIT_SIZES = (1, 2, 5, 12, 20)


def _hits():
    from pointvs_amd.synthetic import random_poses
    lig, rec, lig_feats, rec_feats = _set(6003, n_lig=20)
    hits = [(f'hit{n}', lig_feats[:n].roll(k, 0).contiguous(),
             random_poses(lig[:n], 1, seed=500 + k, max_shift=3.0)[0].contiguous()) for k, n in enumerate(HIT_SIZES)]
    return hits, rec, rec_feats


def _copy_complexes(hits, rec, rec_feats, table, recrop=False):
    """table: per copy (hit, ligand atom left out or -1, receptor atom left out or -1)."""
    build = cref.recropped_complex if recrop else cref.copy_complex
    out = []
    for s, a, r in table:
        if s < 0:
            z = torch.zeros((0, 12))
            out.append((z, z[:, :3], np.zeros(0, dtype=np.int64)))
            continue
        _, feats, pose = hits[s]
        x, pos, kept = build(feats.numpy(), pose.numpy(), rec_feats.numpy(), rec.numpy(), CROP, skip=a, rec_drop=r)
        out.append((torch.from_numpy(x), torch.from_numpy(pos).reshape(-1, 3), kept))
    return out


_ORACLE = {}


def _oracle_separation(hits, rec, rec_feats, seed):
    """Per multi-atom hit the largest |right copy - copy cropped again around what is left of the ligand| over its
    ligand-atom copies, and the largest |output|, by the fp64 oracle on single graphs (the model without GraphNorm)."""
    if seed in _ORACLE:
        return _ORACLE[seed]
    from oracle import egnn_oracle as orc
    model = _model(seed, num_layers=3)
    sd = {k: v.detach().cpu().double() for k, v in model.state_dict().items() if v.is_floating_point()}
    cfg = dict(KW, num_layers=3, _class='SartorrasEGNN')

    def run(complexes):
        outs = []
        for item in _oracle_items(complexes, R_EDGE, R_EDGE):
            with torch.no_grad():
                outs.append(float(orc.model_forward(sd, cfg, item.x.double(), item.pos.double(), item.edge_index,
                                                    item.edge_attr.double(), torch.zeros(item.x.shape[0], dtype=torch.long),
                                                    n_graphs=1).reshape(-1)[0]))
        return np.array(outs)
    seps, top = {}, 0.0
    for s, (name, _, pose) in enumerate(hits):
        if pose.shape[0] < 2:
            continue
        table = [(s, a, -1) for a in range(pose.shape[0])]
        right, wrong = run(_copy_complexes(hits, rec, rec_feats, table)), run(_copy_complexes(hits, rec, rec_feats, table, True))
        seps[name], top = float(np.abs(right - wrong).max()), max(top, float(np.abs(right).max()))
    _ORACLE[seed] = (seps, top)
    return _ORACLE[seed]


@pytest.mark.parametrize('graphnorm', [False, True], ids=['plain', 'graphnorm'])
def test_every_batch_of_both_leave_out_streams_equals_the_plain_forward(graphnorm):
    """Hits of 1, 2, 5, 12 and 20 atoms against 130 receptor atoms, crop radius 5, edge radius 4, batches of 6: every
    batch of the ligand-atom stream (load_leave_out) and of the contact stream (load_leave_out_pairs) == model(Batch)
    on the reference copies (each cropped around the WHOLE hit) with oracle edge lists, each raw output within
    1e-5 * max|raw|, the score differences within 4e-5 * max|raw|.
    What tells a right copy from a re-cropped one: in every multi-atom hit some atom is the only one that keeps some
    receptor atom (asserted), and by the fp64 oracle the copy without it differs from the same copy cropped again around
    the rest of the ligand by at least 2.8e-3 (the 20-atom hit; 1.1e-2 for the 2-atom hit), against 10 x the bound =
    5.7e-6."""
    from pointvs_amd import functional as PF
    from pointvs_amd.graph import Batch
    from pointvs_amd.screening import LibraryScreen, leave_out_pair_plan, leave_out_plan
    b = 6
    hits, rec, rec_feats = _hits()
    ns = [pose.shape[0] for _, _, pose in hits]
    for _, _, pose in hits:                                 # the precondition, on the host
        if pose.shape[0] > 1:
            whole = ref.keep_mask(pose.numpy(), rec.numpy(), CROP)
            alone = [int((whole & ~ref.keep_mask(np.delete(pose.numpy(), a, 0), rec.numpy(), CROP)).sum())
                     for a in range(pose.shape[0])]
            assert max(alone) > 0, alone
    seps, top = _oracle_separation(hits, rec, rec_feats, 1)
    print('oracle: right copy against re-cropped copy, per hit', {k: f'{v:.3e}' for k, v in seps.items()},
          f'10 x bound {1e-4 * top:.3e}')
    assert len(seps) == 4 and all(v > 10 * 1e-5 * top for v in seps.values())
    model = _model(1, num_layers=3, graphnorm=graphnorm).cuda()
    screen = LibraryScreen(model, rec.cuda(), rec_feats, b, 20, R_EDGE, crop_radius=CROP, crop_parents=True,
                           padded_graphnorm=graphnorm)
    big = sorted(range(len(hits)), key=lambda i: -ns[i])
    screen([(hits[i][1], hits[i][2]) for i in big])                  # the sizing batch: the largest whole ligands
    pos = torch.cat([pose for _, _, pose in hits], 0).cuda()
    feats = torch.cat([f for _, f, _ in hits], 0).cuda()
    lig_ptr = torch.tensor([0] + ns).cumsum(0).to(device='cuda', dtype=torch.int32)
    pairs, pair_ptr, host_ptr = PF.contact_pairs(pos, lig_ptr, rec.cuda(), R_EDGE, host_ptr=True)
    counts = (host_ptr[1:] - host_ptr[:-1]).tolist()
    pair_list = pairs.cpu().tolist()
    assert all(counts) and sum(counts) > 30
    atom_table = [(s, a, -1) for s, n in enumerate(ns) for a in [-1] + list(range(n))]
    pair_table = [(s, a, r) for s, k in enumerate(counts) for a, r in [(-1, -1)] + pair_list[host_ptr[s]:host_ptr[s] + k]]
    streams = [('atoms', atom_table, leave_out_plan(ns, b),
                lambda sizes, first: screen.load_leave_out(pos, feats, lig_ptr, sizes, first)),
               ('pairs', pair_table, leave_out_pair_plan(counts, ns, b),
                lambda batch, first: screen.load_leave_out_pairs(pos, feats, lig_ptr, pairs, pair_ptr, *batch, first))]
    for tag, table, plan, load in streams:
        assert len(plan) == -(-len(table) // b)
        table = table + [(-1, -1, -1)] * (len(plan) * b - len(table))
        worst = worst_diff = 0.0
        for k, batch in enumerate(plan):
            load(batch, torch.tensor([k * b], dtype=torch.int32).cuda())
            fast = screen().reshape(-1).clone()
            complexes = _copy_complexes(hits, rec, rec_feats, table[k * b:(k + 1) * b])
            kept = [c[2] for c in complexes]
            mask = np.zeros((b, N_REC), dtype=bool)
            for p, idx in enumerate(kept):
                mask[p, idx] = True
            assert torch.equal(screen.keep.cpu(), torch.from_numpy(np.stack([ref.mask_words(m) for m in mask]).view(np.int64)))
            with torch.no_grad():
                slow = model(Batch.from_data_list(_oracle_items(complexes, R_EDGE, R_EDGE)).to('cuda')).reshape(-1)
            scale = float(slow.abs().max())
            err = float((fast - slow).abs().max()) / scale
            diff = float(((fast[0] - fast) - (slow[0] - slow)).abs().max()) / scale
            worst, worst_diff = max(worst, err), max(worst_diff, diff)
            assert err <= 1e-5 and diff <= 4e-5, (tag, k, err, diff)
        print(f'graphnorm={graphnorm} {tag}: {len(plan)} batches, raw err {worst:.3e} (1e-5), differences {worst_diff:.3e} (4e-5)')
    screen.check()
    screen.check_leave_out()


# ---------------------------------------------------------------- end to end

def _one_at_a_time(model, hit, rec, rec_feats):
    """(atom_masking scores over the hit's cropped complex [n + kept], bond_masking's {(a, r): score}, kept atoms)."""
    from pointvs_amd import attribution
    from pointvs_amd.radius_graph import generate_edges
    _, feats, pose = hit
    n = int(pose.shape[0])
    x, pos, kept = cref.copy_complex(feats.cpu().numpy(), pose.cpu().numpy(), rec_feats.numpy(), rec.numpy(), CROP)
    x, pos = torch.from_numpy(x).cuda(), torch.from_numpy(pos).cuda()
    _, ei, attrs = generate_edges(pos, x[:, -1].contiguous(), R_EDGE, R_EDGE, prune=False)
    kw = dict(edge_indices=ei, edge_attrs=torch.nn.functional.one_hot(attrs, 3))
    atoms = attribution.atom_masking(model, pos[None], x[None], **kw)
    bonds = attribution.bond_masking(model, pos[None], x[None], **kw)
    ei, cls = ei.cpu().numpy(), attrs.cpu().numpy()
    by_pair = {(int(a), int(kept[c - n])): float(bonds[e]) for e, (a, c) in enumerate(ei.T) if cls[e] == 1 and a < n}
    return atoms, by_pair, kept


@needs_caching_allocator
def test_end_to_end_after_a_cropped_run_library(tmp_path):
    from pointvs_amd.screening import LibraryScreen, ScreeningSweep
    from tests.test_gpu_ligand_masking import _library
    b = 4
    lig, rec, lig_feats, rec_feats = _set(6005, n_lig=70)
    work = [w for w in _library(lig, lig_feats) if w[0] != 'ligC']              # 12, 9, (none), 12 and 1 atoms
    model = _model(2, num_layers=3).cuda()
    sweep = ScreeningSweep(model, rec.cuda(), rec_feats, edge_radius=R_EDGE, batch_size=b, crop_radius=CROP,
                           cropped_attribution=True)
    sweep.run_library(work, hits_file=tmp_path / 'hits.txt')
    hits = list(sweep.best_poses(work))
    names = [name for name, _, _ in hits]
    ns = [int(pose.shape[0]) for _, _, pose in hits]
    assert names == ['ligA', 'ligB', 'ligD', 'ligE'] and ns == [12, 9, 12, 1]
    # ligE, one atom near the centre of the pocket, keeps no receptor atom at all: its cropped complex is the lone atom,
    # its leave-out copy an empty slot - the sweep takes it, the one-at-a-time route has no forward on a graph without
    # nodes, so it has no reference here
    assert not ref.keep_mask(hits[3][2].cpu().numpy(), rec.numpy(), CROP).any()
    refs = {hit[0]: _one_at_a_time(model, hit, rec, rec_feats) for hit in hits[:3]}
    refs['ligE'] = (None, {}, np.zeros(0, dtype=np.int64))
    assert all(0 < len(refs[name][2]) < N_REC for name in names[:3])

    def close(got, want, raw, what):
        gap, bound = float(np.abs(got.double().cpu().numpy() - want).max()), 4e-5 * float(raw.abs().max())
        print(f'{what}: against pointvs_amd.attribution on the cropped complex {gap:.3e} bound {bound:.3e}')
        assert gap <= bound, what

    # ligand atoms
    before = sweep.batches_run
    out = sweep.ligand_atom_masking(hits, scores_file=tmp_path / 'atoms.txt', sigmoid=False)
    assert sweep.batches_run - before == 1 + -(-(sum(ns) + len(ns)) // b)       # the sizing batch, then the steps
    screen = sweep.cropped_copies
    assert screen.crop_parents and screen._captured and sweep.masking is None and sweep.struck is None
    lines, at = (tmp_path / 'atoms.txt').read_text().splitlines(), 0
    assert len(lines) == sum(ns)
    for name, n in zip(names, ns):
        raw = sweep.atom_masking_raw[name]
        assert raw.shape == (n + 1, 1) and torch.equal(out[name], raw[0, 0] - raw[1:, 0])
        if refs[name][0] is not None:
            close(out[name], refs[name][0][:n], raw, f'ligand_atom_masking {name}')
        for a, v in enumerate(out[name].tolist()):
            assert re.fullmatch(r'-?\d+\.\d{6} \| receptor ' + re.escape(f'{name}_atom{a}'), lines[at]), lines[at]
            assert lines[at] == f'{v:.6f} | receptor {name}_atom{a}'
            at += 1
    # contacts: the same screen, no sizing batch again
    before = sweep.batches_run
    contacts = sweep.contact_masking(hits, scores_file=tmp_path / 'contacts.txt', sigmoid=False)
    counts = [int(contacts[name][0].shape[0]) for name in names]
    assert sum(counts) > 20 and sweep.batches_run - before == -(-(sum(counts) + len(names)) // b)
    assert sweep.cropped_copies is screen
    lines, at = (tmp_path / 'contacts.txt').read_text().splitlines(), 0
    assert len(lines) == sum(counts)
    for name in names:
        pairs, scores = contacts[name]
        raw = sweep.contact_masking_raw[name]
        by_pair = refs[name][1]
        assert sorted(by_pair) == [tuple(p) for p in pairs.tolist()]
        if len(by_pair):
            close(scores, np.array([by_pair[tuple(p)] for p in pairs.tolist()]), raw, f'contact_masking {name}')
        for (a, r), v in zip(pairs.tolist(), scores.tolist()):
            assert lines[at] == f'{v:.6f} | receptor {name}_atom{a} atom{r}'
            at += 1
    # receptor atoms: 'all' is exactly the kept atoms of each hit
    before = sweep.batches_run
    atoms = sweep.receptor_atom_masking(hits, atoms='all', scores_file=tmp_path / 'rec.txt', sigmoid=False)
    m = [int(atoms[name][0].shape[0]) for name in names]
    assert sweep.batches_run - before == -(-(sum(m) + len(names)) // b)
    lines, at = (tmp_path / 'rec.txt').read_text().splitlines(), 0
    assert len(lines) == sum(m)
    for name, n in zip(names, ns):
        which, scores = atoms[name]
        assert which.tolist() == refs[name][2].tolist()
        if refs[name][0] is not None:
            close(scores, refs[name][0][n:], sweep.receptor_atom_masking_raw[name], f'receptor_atom_masking {name}')
        for r, v in zip(which.tolist(), scores.tolist()):
            assert lines[at] == f'{v:.6f} | receptor {name} atom{r}'
            at += 1
    # 'contacts' (every contact atom is kept at crop_radius >= edge_radius), and an index tensor intersected per hit
    by_contact = sweep.receptor_atom_masking(hits, sigmoid=False)
    for name in names:
        assert by_contact[name][0].tolist() == sorted(set(contacts[name][0][:, 1].tolist()))
    kept_a, kept_b = set(refs['ligA'][2].tolist()), set(refs['ligB'][2].tolist())
    both, neither = sorted(kept_a & kept_b), sorted(set(range(N_REC)) - kept_a - kept_b)
    assert both and neither                                   # an atom both hits keep, one that neither keeps
    asked = sorted(kept_a - kept_b)[:1] + both[-1:] + neither[:1] + sorted(kept_b - kept_a)[:1] + both[:1]
    picked = sweep.receptor_atom_masking(hits[:2], atoms=torch.tensor(asked), sigmoid=False)
    assert picked['ligA'][0].tolist() == [r for r in asked if r in kept_a]         # (the order asked for)
    assert picked['ligB'][0].tolist() == [r for r in asked if r in kept_b]
    assert picked['ligB'][1].shape == picked['ligB'][0].shape and neither[0] not in picked['ligA'][0].tolist()
    full = dict(zip(atoms['ligA'][0].tolist(), atoms['ligA'][1].tolist()))
    for r, v in zip(picked['ligA'][0].tolist(), picked['ligA'][1].tolist()):
        assert abs(v - full[r]) <= 4e-5 * float(sweep.receptor_atom_masking_raw['ligA'].abs().max())
    assert sweep.contact_masking([]) == {} and sweep.ligand_atom_masking([]) == {}
    # refusals
    with pytest.raises(NotImplementedError, match='attention and CAM reductions assume n_rec receptor rows'):
        sweep.receptor_hotspots(hits)
    with pytest.raises(ValueError, match='crop_radius 3 is below the edge radius 4'):
        ScreeningSweep(model, rec.cuda(), rec_feats, edge_radius=R_EDGE, crop_radius=3.0, cropped_attribution=True)
    with pytest.raises(ValueError, match=r'crop_parents=True\) needs crop_radius'):
        LibraryScreen(model, rec.cuda(), rec_feats, b, 12, R_EDGE, crop_parents=True)
    with pytest.raises(ValueError, match='it has no rec_drop table'):
        LibraryScreen(model, rec.cuda(), rec_feats, b, 12, R_EDGE, crop_radius=CROP).load_leave_out_pairs(
            lig[:5].cuda(), lig_feats[:5].cuda(), torch.tensor([0, 5], dtype=torch.int32).cuda(),
            torch.zeros((0, 2), dtype=torch.int32).cuda(), torch.tensor([0, 0], dtype=torch.int32).cuda(), [5], 0,
            torch.zeros(1, dtype=torch.int32).cuda())
    with pytest.raises(ValueError, match='struck'):
        LibraryScreen(model, rec.cuda(), rec_feats, b, 12, R_EDGE, crop_radius=CROP, crop_parents=True, struck=True)
    with pytest.raises(NotImplementedError, match='fp32 only'):
        ScreeningSweep(_model(2, num_layers=3).cuda().double(), rec.cuda().double(), rec_feats.double(),
                       edge_radius=R_EDGE, batch_size=b, crop_radius=CROP,
                       cropped_attribution=True).ligand_atom_masking(hits)
    # a parent table the packer refuses, through the screen
    screen.load_leave_out(lig[:5].cuda(), lig_feats[:5].cuda(), torch.tensor([0, 6], dtype=torch.int32).cuda(), [0] * b,
                          torch.zeros(1, dtype=torch.int32).cuda())
    assert not screen.crop_ptr.any() and not screen.lig_ptr.any()
    with pytest.raises(ValueError, match='lig_ptr is not a table'):
        screen.check_leave_out()
