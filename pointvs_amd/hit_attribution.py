"""Attribution of a sweep's hits: the bodies of ScreeningSweep.ligand_atom_masking / contact_masking /
receptor_atom_masking / receptor_hotspots (their docstrings, in screening.py, say what each computes) as plain
functions over the sweep, every step they share written once: `Hits`, `_ready_screen`, `_leave_out_stream`,
`checked_column`, `split_scores`, `_write_scores`. This module imports screening; the sweep's methods import it when
called."""
from itertools import accumulate
from pathlib import Path

import torch

from . import functional as PF
from .screening import MAX_SCREEN_LIGAND_ATOMS, leave_out_pair_plan, leave_out_plan, slot_offsets


class Hits:
    """An iterable of (name, lig_feats [n,F], pose [n,3]) validated - unique names, n <= MAX_SCREEN_LIGAND_ATOMS, one
    pose each, or a ValueError that begins with `who` - as `items` (a list), `names` and `ns` (atom counts); after
    pack(dev) also pos [L,3], feats [L,F] and lig_ptr [S+1] int32 on the device, item order."""

    def __init__(self, items, who):
        self.items = [(name, lig_feats, pose) for name, lig_feats, pose in items]
        self.names = names = [name for name, _, _ in self.items]
        if len(set(names)) != len(names):
            raise ValueError(f'{who}: names must be unique (repeated: '
                             f'{sorted({n for n in names if names.count(n) > 1})})')
        self.ns = []
        for name, lig_feats, pose in self.items:
            n = int(pose.shape[0])
            if n > MAX_SCREEN_LIGAND_ATOMS:
                raise ValueError(f'{who}: ligand {name!r} has {n} atoms: a pose-batch slot holds up to '
                                 f'{MAX_SCREEN_LIGAND_ATOMS}')
            if pose.dim() != 2 or pose.shape[1] != 3 or lig_feats.dim() != 2 or int(lig_feats.shape[0]) != n:
                raise ValueError(f'{who}: ligand {name!r}: lig_feats [n, F] and ONE pose [n, 3]')
            self.ns.append(n)
        self.pos = self.feats = self.lig_ptr = None

    def pack(self, dev, lig_ptr=True):
        """The hits on `dev`, packed at the first call (a method packs where it always did, and once). lig_ptr False:
        without the offsets (receptor_hotspots loads whole batches by slot_offsets: one copy and one launch less)."""
        if self.pos is None:
            self.pos = torch.cat([pose.to(dev).float() for _, _, pose in self.items], 0).contiguous()
            self.feats = torch.cat([lig_feats.to(dev).float() for _, lig_feats, _ in self.items], 0).contiguous()
        if lig_ptr and self.lig_ptr is None:
            self.lig_ptr = torch.tensor([0] + self.ns).cumsum(0).to(device=dev, dtype=torch.int32)
        return self


def _starts(counts):
    """The exclusive prefix sums of a host list."""
    return [0, *accumulate(counts)][:-1]


def ligand_atom_labels(names, ns):
    return [f'{name}_atom{a}' for name, n in zip(names, ns) for a in range(n)]


def contact_labels(names, counts, pairs):
    """pairs: the host's [K, 2] list (ligand atom, receptor atom), counts[s] rows per name."""
    return [f'{name}_atom{a} atom{r}' for name, k, lo in zip(names, counts, _starts(counts)) for a, r in pairs[lo:lo + k]]


def receptor_atom_labels(names, counts, atoms):
    """atoms: the host's [M] list of receptor atoms, counts[s] entries per name."""
    return [f'{name} atom{r}' for name, k, lo in zip(names, counts, _starts(counts)) for r in atoms[lo:lo + k]]


def _write_scores(sweep, path, form, values, labels, touch=False):
    """One line per label through a PredictionsWriter of line format `form`; values: a tensor or array with one row
    per label, or a callable that gives it (called only when there are labels). touch: the file exists afterwards even
    without a line."""
    from .predictions import PredictionsWriter
    with PredictionsWriter(path, form) as writer:
        if labels:
            writer.submit(values() if callable(values) else values, None, [sweep.receptor_name] * len(labels), labels)
    if touch:
        Path(path).expanduser().touch()


def checked_column(who, column, n_outputs):
    if not 0 <= int(column) < n_outputs:
        raise ValueError(f'{who}: column {column} of {n_outputs} outputs')
    return int(column)


def split_scores(names, counts, raw, scored, column):
    """({name: raw rows [K + 1, C]}, {name: s(whole) - s(copy k) [K]}) from the copies' rows in copy order (hit s:
    the whole complex, then its counts[s] copies)."""
    raws, out, at = {}, {}, 0
    scored = scored[:, column]
    for name, k in zip(names, counts):
        raws[name] = raw[at:at + k + 1]
        out[name] = scored[at] - scored[at + 1:at + k + 1]
        at += k + 1
    return raws, out


def _per_hit(names, counts, rows, scores):
    """{name: (the hit's counts[s] rows of `rows`, its scores)}."""
    return {name: (rows[lo:lo + k], scores[name]) for name, k, lo in zip(names, counts, _starts(counts))}


def _ready_screen(sweep, hits, which, **kw):
    """The sweep's LibraryScreen `which` (ScreeningSweep._library_screen) wide enough for the hits, its edge buffers
    sized."""
    screen = sweep._library_screen(max(max(hits.ns), 1), which, **kw)
    if screen.needs_sizing_batch():
        # a new screen sizes its edge buffers from its first batch, and the first leave-out batch may hold the copies
        # of one small ligand: it is shown a batch of the largest whole ligands first (a copy has no more contacts per
        # atom than its whole complex; a struck screen, which always has the reuse, adds the struck rows' room itself)
        big = sorted(range(len(hits.items)), key=lambda i: -hits.ns[i])[:sweep.b]
        screen([(hits.items[i][1], hits.items[i][2]) for i in big])
        sweep.batches_run += 1
    return screen


def _copies_screen(sweep, hits, which, **kw):
    """`_ready_screen` for a stream of leave-out copies: the sweep's screen `which` - on a cropped sweep
    (cropped_attribution=True) the ONE LibraryScreen(crop_parents=True) of all three masking methods,
    `sweep.cropped_copies`, whose slots are cropped around their parents; its sizing batch of whole ligands bounds every
    copy's graph, a subgraph of its whole cropped complex."""
    if sweep.crop_radius is not None:
        return _ready_screen(sweep, hits, 'cropped_copies', crop_parents=True)
    return _ready_screen(sweep, hits, which, **kw)


def _leave_out_stream(sweep, screen, plan, total, load, sigmoid):
    """The batches of `plan` through `screen`: load(batch, first_copy [1] int32 on the device) lays a batch out (one
    packer launch), then the one captured step; the builder's status one batch late, the packer's verdict after the
    last. Returns (raw [total, C], the same with the sweep's sigmoid)."""
    firsts = (torch.arange(len(plan), dtype=torch.int32) * sweep.b).to(sweep.rec_pos.device)    # batch k: copy k * b
    kept = []
    with sweep._sweeping(None, sigmoid, None) as sink:
        for k, batch in enumerate(plan):
            load(batch, firsts[k:k + 1])
            kept.append(sweep._library_step(screen))
            sweep.batches_run += 1
        screen.check()
        screen.check_leave_out()
        raw = torch.cat(kept, 0)[:total]
        return raw, sink.scored(raw)


@torch.no_grad()
def ligand_atom_masking(sweep, items, scores_file=None, sigmoid=None, column=0):
    hits = Hits(items, 'ligand_atom_masking')
    names, ns = hits.names, hits.ns
    sweep.atom_masking_raw = {}
    if not hits.items:
        return {}
    screen = _copies_screen(sweep, hits, 'masking')
    hits.pack(sweep.rec_pos.device)
    raw, scored = _leave_out_stream(
        sweep, screen, leave_out_plan(ns, sweep.b), sum(ns) + len(ns),
        lambda sizes, first: screen.load_leave_out(hits.pos, hits.feats, hits.lig_ptr, sizes, first), sigmoid)
    column = checked_column('ligand_atom_masking', column, raw.shape[1])
    sweep.atom_masking_raw, out = split_scores(names, ns, raw, scored, column)
    if scores_file:
        _write_scores(sweep, scores_file, 'atom_masking', lambda: torch.cat([out[name] for name in names], 0),
                      ligand_atom_labels(names, ns))
    return out


def _pair_copies(sweep, hits, pairs, counts, ligand_atom, sigmoid):
    """Every hit's copies - the whole complex, then one per row of its pair table (pairs [K,2] int32 on the device:
    ligand atom inside the hit or -1, receptor atom; counts: the host's rows per hit) - streamed through the one
    struck LibraryScreen `sweep.struck` in dense batches (load_leave_out_pairs). Returns (raw [K + hits, C], the same
    with the sweep's sigmoid)."""
    dev = sweep.rec_pos.device
    screen = _copies_screen(sweep, hits, 'struck', struck=True)
    hits.pack(dev)
    pair_ptr = torch.tensor([0] + list(counts)).cumsum(0).to(device=dev, dtype=torch.int32)
    return _leave_out_stream(
        sweep, screen, leave_out_pair_plan(counts, hits.ns, sweep.b, ligand_atom=ligand_atom),
        sum(counts) + len(hits.ns),
        lambda batch, first: screen.load_leave_out_pairs(hits.pos, hits.feats, hits.lig_ptr, pairs, pair_ptr, *batch,
                                                         first), sigmoid)


def _hit_contacts(sweep, hits):
    """(pairs [K,2] int32 on the device, the host's pair counts per hit): PF.contact_pairs of the hits against the
    receptor at the sweep's edge radius; the whole pair_ptr comes back in the method's one copy to the host."""
    hits.pack(sweep.rec_pos.device)
    pairs, _, host_ptr = PF.contact_pairs(hits.pos, hits.lig_ptr, sweep.rec_pos.float().contiguous(),
                                          sweep.edge_radius, host_ptr=True)
    return pairs, [int(k) for k in (host_ptr[1:] - host_ptr[:-1]).tolist()]


def _hit_keep(sweep, hits):
    """PF.crop_keep of the hits at the sweep's crop radius: (keep masks [hits, words], kept_ptr, the host's kept_ptr)."""
    hits.pack(sweep.rec_pos.device)
    return PF.crop_keep(hits.pos, hits.lig_ptr, sweep.rec_pos.float().contiguous(), sweep.crop_radius, host_ptr=True)


@torch.no_grad()
def contact_masking(sweep, items, scores_file=None, sigmoid=None, column=None):
    hits = Hits(items, 'contact_masking')
    names = hits.names
    sweep.contact_masking_raw = {}
    if column is None and sweep.tasks == 'both':
        raise ValueError("contact_masking: with tasks='both' the column must be named (0: pose, 1..: affinity)")
    if not hits.items:
        return {}
    pairs, counts = _hit_contacts(sweep, hits)
    raw, scored = _pair_copies(sweep, hits, pairs, counts, True, sigmoid)
    if column is None:
        column = 1 if raw.shape[1] > 1 else 0
    column = checked_column('contact_masking', column, raw.shape[1])
    sweep.contact_masking_raw, scores = split_scores(names, counts, raw, scored, column)
    if scores_file:
        _write_scores(sweep, scores_file, 'atom_masking', lambda: torch.cat([scores[name] for name in names], 0),
                      contact_labels(names, counts, pairs.cpu().tolist() if sum(counts) else []))
    return _per_hit(names, counts, pairs, scores)


@torch.no_grad()
def receptor_atom_masking(sweep, items, atoms='contacts', scores_file=None, sigmoid=None, column=0):
    hits = Hits(items, 'receptor_atom_masking')
    names, n_hits = hits.names, len(hits.items)
    sweep.receptor_atom_masking_raw = {}
    if not n_hits:
        return {}
    dev, n_rec = sweep.rec_pos.device, int(sweep.rec_pos.shape[0])
    if isinstance(atoms, str) and atoms == 'contacts':
        pairs, counts = _hit_contacts(sweep, hits)
        hit = torch.repeat_interleave(torch.arange(n_hits, device=dev), torch.tensor(counts, device=dev))
        keys = torch.unique(hit * n_rec + pairs[:, 1].long())         # ascending: by hit, then by receptor atom
        which = (keys % n_rec).to(torch.int32)
        counts = torch.bincount(keys // n_rec, minlength=n_hits).tolist()
    elif isinstance(atoms, str) and atoms == 'all' and sweep.crop_radius is not None:
        # every atom of each hit's cropped complex: the builders' keep decision, counts from its one copy back
        keep, _, host_ptr = _hit_keep(sweep, hits)
        which = PF.kept_atoms(keep, n_rec)[1].to(torch.int32)
        counts = [int(k) for k in (host_ptr[1:] - host_ptr[:-1]).tolist()]
    elif isinstance(atoms, str) and atoms == 'all':
        which = torch.arange(n_rec, dtype=torch.int32, device=dev).repeat(n_hits)
        counts = [n_rec] * n_hits
    elif torch.is_tensor(atoms) and atoms.dim() == 1 and not atoms.is_floating_point():
        host = [int(r) for r in atoms.tolist()]
        if any(not 0 <= r < n_rec for r in host):
            raise ValueError(f'receptor_atom_masking: atoms must be receptor atoms 0..{n_rec - 1}')
        which = torch.tensor(host, dtype=torch.int32, device=dev).repeat(n_hits)
        counts = [len(host)] * n_hits
        if sweep.crop_radius is not None and host:
            # an atom a hit's crop does not keep is no atom of that hit's complex: the list intersected with the kept
            # atoms per hit, order kept
            keep = _hit_keep(sweep, hits)[0]
            at = which[:len(host)].long()
            on = ((keep[:, at >> 6] >> (at & 63)) & 1).bool()      # [hits, atoms]
            which = which[on.reshape(-1)]
            counts = [int(k) for k in on.sum(1).tolist()]
    else:
        raise ValueError(f"receptor_atom_masking: atoms={atoms!r}: 'contacts', 'all' or a 1-D index tensor")
    table = torch.stack([torch.full_like(which, -1), which], 1).contiguous()
    raw, scored = _pair_copies(sweep, hits, table, counts, False, sigmoid)
    column = checked_column('receptor_atom_masking', column, raw.shape[1])
    sweep.receptor_atom_masking_raw, scores = split_scores(names, counts, raw, scored, column)
    if scores_file:
        _write_scores(sweep, scores_file, 'atom_masking', lambda: torch.cat([scores[name] for name in names], 0),
                      receptor_atom_labels(names, counts, which.cpu().tolist() if sum(counts) else []))
    return _per_hit(names, counts, which, scores)


ATTRIBUTIONS = ('edge_attention', 'cam', 'atom_masking')


def _masking_rows(sweep, items, atoms, sigmoid, column):
    """attribution='atom_masking': the sweep's own receptor_atom_masking and ligand_atom_masking of the hits, the
    receptor scores laid out as NaN-filled rows. Returns (rows [hits, n_rec], {name: ligand scores [n]})."""
    dev, n_rec = sweep.rec_pos.device, int(sweep.rec_pos.shape[0])
    if torch.is_tensor(atoms) and atoms.dim() == 1 and not atoms.is_floating_point():
        listed = atoms.tolist()
        if len(set(listed)) != len(listed):
            raise ValueError('receptor_hotspots: atoms lists a receptor atom more than once '
                             f'({sorted({r for r in listed if listed.count(r) > 1})}): a hit has one score per atom')
    by_hit = sweep.receptor_atom_masking(items, atoms=atoms, sigmoid=sigmoid, column=column)
    ligand = sweep.ligand_atom_masking(items, sigmoid=sigmoid, column=column)
    rows = torch.full((len(items), n_rec), float('nan'), dtype=torch.float32, device=dev)
    counts = [int(by_hit[name][0].shape[0]) for name, _, _ in items]
    if sum(counts):
        # (one indexed write: a hit lists an atom once)
        hit = torch.repeat_interleave(torch.arange(len(items), device=dev), torch.tensor(counts, device=dev))
        which = torch.cat([by_hit[name][0] for name, _, _ in items], 0).long()
        rows[hit, which] = torch.cat([by_hit[name][1] for name, _, _ in items], 0).float()
    return rows, {name: ligand[name].float() for name, _, _ in items}


def _hotspot_order(out, use_rank, top):
    """The receptor atoms with count > 0, best first - by rank_mean ascending under use_rank, else by mean descending
    (the reference's final sort), ties to the lower atom - cut to the first `top` (its --cutoff)."""
    key = out['rank_mean'] if use_rank else -out['mean']
    have = torch.nonzero(out['count'] > 0).reshape(-1)
    order = have[torch.sort(key[have], stable=True).indices]       # (have ascends: a stable sort leaves ties to the lower atom)
    return order if top is None else order[:top]


@torch.no_grad()
def receptor_hotspots(sweep, items, gnn_layer=1, scores_file=None, per_hit=False, attribution='edge_attention',
                      column=None, ligand_scores_file=None, atoms='contacts', sigmoid=None, use_rank=False, top=None):
    if attribution not in ATTRIBUTIONS:
        raise ValueError(f"receptor_hotspots: attribution={attribution!r}: 'edge_attention', 'cam' or 'atom_masking'")
    by_cam, by_masking = attribution == 'cam', attribution == 'atom_masking'
    if column is not None and not (by_cam or by_masking):
        raise ValueError("receptor_hotspots: column selects a head output of attribution='cam' or 'atom_masking'")
    if not by_masking and (sigmoid is not None or not (isinstance(atoms, str) and atoms == 'contacts')):
        raise ValueError("receptor_hotspots: atoms and sigmoid belong to attribution='atom_masking'")
    if top is not None:
        top = int(top)
        if top < 0:
            raise ValueError(f'receptor_hotspots: top={top}: the number of atoms to keep in order, or None')
    hits = Hits(items, 'receptor_hotspots')            # (materialises `items`, once)
    names, ns = hits.names, hits.ns
    dev, n_rec = sweep.rec_pos.device, int(sweep.rec_pos.shape[0])
    ligand, hit_rows = {}, []
    # use_rank: the ranks of every batch's values (PF.hit_value_ranks, behind the step and outside its capture)
    # accumulate into a second triple; edge_attention ranks the receptor atoms alone, the other two the whole complex
    ranks = PF.new_contact_accumulators(n_rec, dev) if use_rank else None
    rank_rows, lig_ranks = [], []
    lig_key, slot_key = ('lig_val', 'slot_rec_val') if by_cam else ('lig_att', 'slot_rec_att')
    if by_masking:
        rows, ligand = _masking_rows(sweep, hits.items, atoms, sigmoid, 0 if column is None else column)
        rec_sum, count, high = PF.hit_rows_accumulate(rows, PF.new_contact_accumulators(n_rec, dev))
        if use_rank and hits.items:
            lig_ptr = torch.tensor([0] + ns).cumsum(0).to(device=dev, dtype=torch.int32)
            got = PF.hit_value_ranks(rows, torch.cat([ligand[name] for name in names], 0), lig_ptr, acc=ranks)
            rank_rows.append(got[0])
            lig_ranks.append(got[1])
        if per_hit:
            hit_rows.append(rows)
    elif hits.items:
        kw = dict(cam=True if column is None else int(column)) if by_cam else dict(contact_attention=gnn_layer)
        screen = _ready_screen(sweep, hits, 'cam_screen' if by_cam else 'hotspot', **kw)
        values = screen.cam if by_cam else screen.contact
        sweep._capture_if_wanted(screen)
        # (behind the sizing batch and the capture's warm-up steps)
        screen.reset_cam() if by_cam else screen.reset_contact_attention()
        hits.pack(dev, lig_ptr=False)
        batches =[ns[k:k + sweep.b] for k in range(0, len(ns), sweep.b)]
        ptrs_dev = slot_offsets(batches, sweep.b).to(dev)
        at, lig_rows = 0, []
        for k, batch_ns in enumerate(batches):
            total = sum(batch_ns)
            screen.load_packed(hits.pos[at:at + total], hits.feats[at:at + total], ptrs_dev[k], batch_ns)
            at += total
            sweep._library_step(screen)
            sweep.batches_run += 1
            lig_rows.append(values[lig_key][:total].clone())
            if per_hit:
                hit_rows.append(values[slot_key][:len(batch_ns)].clone())
            if use_rank:
                with_lig = (lig_rows[-1], ptrs_dev[k, :len(batch_ns) + 1]) if by_cam else ()
                got = PF.hit_value_ranks(values[slot_key][:len(batch_ns)], *with_lig, acc=ranks)
                if per_hit:
                    rank_rows.append(got[0])
                if by_cam:
                    lig_ranks.append(got[1])
        screen.check()
        rec_sum, count, high = (values[key].clone() for key in ('rec_sum', 'rec_count', 'rec_max'))
        lig_rows = torch.cat(lig_rows, 0)
        ligand = {name: lig_rows[lo:lo + n] for name, n, lo in zip(names, ns, _starts(ns))}
    else:
        rec_sum, count, high = PF.new_contact_accumulators(n_rec, dev)
    out = dict(mean=rec_sum / count, count=count, max=high, ligand=ligand)      # (0 / 0: NaN)
    if per_hit:
        out['per_hit'] = torch.cat(hit_rows, 0) if hit_rows else torch.empty((0, n_rec), dtype=torch.float32,
                                                                             device=dev)
    if use_rank:
        out['rank_mean'] = ranks[0] / ranks[1]
        if by_cam or by_masking:
            packed = torch.cat(lig_ranks, 0) if lig_ranks else torch.empty(0, dtype=torch.float32, device=dev)
            out['ligand_rank'] = {name: packed[lo:lo + n] for name, n, lo in zip(names, ns, _starts(ns))}
        if per_hit:
            out['per_hit_rank'] = torch.cat(rank_rows, 0) if rank_rows else torch.empty((0, n_rec), dtype=torch.float32,
                                                                                       device=dev)
    if use_rank or top is not None:
        out['order'] = _hotspot_order(out, use_rank, top)
    if scores_file:
        # the one copy to the host (under use_rank the file carries rank_mean)
        packed = torch.stack([out['rank_mean' if use_rank else 'mean'], count.double()], 1).cpu().numpy()
        atoms = [j for j in range(n_rec) if packed[j, 1] > 0]
        # (touch: no contact at all gives an empty file)
        _write_scores(sweep, scores_file, 'hotspot', packed[atoms], [f'atom{j}' for j in atoms], touch=True)
    if ligand_scores_file:
        _write_scores(sweep, ligand_scores_file, 'atom_masking', lambda: torch.cat([ligand[name] for name in names], 0),
                      ligand_atom_labels(names, ns), touch=True)
    return out
