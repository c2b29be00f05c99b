"""Cropped copies (PvsScreenCopiesJob / pvs_screen_copies_build, pvs_crop_keep, pvs_leave_out_parent_pack;
LibraryScreen(crop_parents=True), ScreeningSweep(cropped_attribution=True)), the host side (CPU): the ctypes struct against
the C compiler's layout, every refusal of csrc/screen_copies.h by its text (compiled alone with the host compiler), the
loaded library refusing by name before any launch, exports and prototype widths, the numpy references of
tests/_crop_copies_ref.py against scipy's cdist, and the Python keyword refusals that need no device."""
import ctypes as C
import inspect
import re
import subprocess

import numpy as np
import pytest

from tests import _crop_copies_ref as cref
from tests.test_screen_job_host import CC, CXX, INCLUDE, _compile

WHO = 'pvs_screen_copies_build'
SLOTS_WHO = 'pvs_screen_slots_build'
FIELDS = ['slots', 'crop_pos', 'crop_ptr', 'rec_drop', 'crop_cap']


def test_binding_layout_is_the_c_compilers(tmp_path):
    from pointvs_amd import _lib
    lines = ['#include "pvs_egnn.h"', '#include <stddef.h>', '#include <stdio.h>', 'int main(void) {',
             '    printf("sizeof %zu\\n", sizeof(PvsScreenCopiesJob));']
    lines += [f'    printf("{n} %zu %zu\\n", offsetof(PvsScreenCopiesJob, {n}), sizeof(((PvsScreenCopiesJob*)0)->{n}));'
              for n in FIELDS]
    exe = _compile(CC, ['-std=c11'], '\n'.join(lines + ['    return 0;', '}', '']), tmp_path / 'layout')
    want = [tuple(line.split()) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                           check=True).stdout.splitlines()]
    cls = _lib.PvsScreenCopiesJob
    assert [n for n, _ in cls._fields_] == FIELDS
    got = [('sizeof', str(C.sizeof(cls)))] + [(n, str(getattr(cls, n).offset), str(getattr(cls, n).size)) for n in FIELDS]
    assert got == want
    assert cls.slots.size == C.sizeof(_lib.PvsScreenSlotsJob) and cls.slots.offset == 0      # embedded by value, first


# argv: field=value settings on top of an acceptable job (a pointer field: 0 = NULL, else some address). Prints the
# refusal of the whole job and the refusal of its counts alone ("fine" for none).
PROGRAM = r'''
#include "screen_copies.h"
#include <stdlib.h>
#include <string>
static int32_t some[4];
static bool set(PvsScreenCopiesJob& j, const std::string& key, const char* val) {
    const long v = atol(val);
#define PTR(f) if (key == #f) { j.f = v ? (decltype(j.f))(void*)some : nullptr; return true; }
#define INT(f) if (key == #f) { j.f = (int32_t)v; return true; }
#define DBL(f) if (key == #f) { j.f = atof(val); return true; }
    PTR(crop_pos) PTR(crop_ptr) PTR(rec_drop) INT(crop_cap)
    INT(slots.layout) PTR(slots.lig_pos) PTR(slots.lig_ptr) PTR(slots.rec_drop) PTR(slots.rec_pos) PTR(slots.keep)
    PTR(slots.status) PTR(slots.full.rowptr) PTR(slots.lig.rowptr) INT(slots.n_slots) INT(slots.lig_cap)
    INT(slots.n_rec) INT(slots.slot_cap) DBL(slots.crop_radius) INT(slots.tables.n_feats) PTR(slots.tables.base_magg)
    return false;
}
int main(int argc, char** argv) {
    PvsScreenCopiesJob j = {};
    PvsScreenSlotsJob& s = j.slots;
    s.layout = PVS_SLOTS_CROPPED;
    s.lig_pos = (const float*)some; s.lig_ptr = some; s.rec_pos = (const float*)some; s.rr_rowptr = s.rr_col = some;
    s.full.rowptr = s.full.row = s.full.col = some; s.full.etype = (uint8_t*)some;
    s.inv_deg = (float*)some; s.node_ptr = s.node_graph = some; s.pos = (float*)some; s.keep = (uint64_t*)some;
    s.status = some;
    s.n_slots = 2; s.lig_cap = 64; s.n_rec = 65; s.slot_cap = 64; s.inter_radius = 4.0; s.intra_radius = 2.0;
    s.crop_radius = 6.0;
    j.crop_pos = (const float*)some; j.crop_ptr = some; j.crop_cap = 64;
    for (int i = 1; i < argc; ++i) {
        const std::string arg = argv[i];
        const size_t eq = arg.find('=');
        if (eq == std::string::npos || !set(j, arg.substr(0, eq), arg.c_str() + eq + 1)) return 2;
    }
    char why[256], why_counts[256];
    const char* full = pvs_screen_copies_refusal(j, false, why, sizeof(why));
    const char* counts = pvs_screen_copies_refusal(j, true, why_counts, sizeof(why_counts));
    printf("%s\n%s\n", full ? full : "fine", counts ? counts : "fine");
    return 0;
}
'''

# (settings, the refusal or None for an accepted job, whether the counts alone are accepted)
CASES = [
    ({}, None, True),
    ({'rec_drop': 1}, None, True),                                       # the copies' own rec_drop: optional
    ({'crop_pos': 0}, f'{WHO}: NULL crop_pos', True),
    ({'crop_ptr': 0}, f'{WHO}: NULL crop_ptr', True),
    ({'crop_cap': 0}, f'{WHO}: crop_cap must be 1..1024 * slots (got 0 for 2)', False),
    ({'crop_cap': -5}, f'{WHO}: crop_cap must be 1..1024 * slots (got -5 for 2)', False),
    ({'crop_cap': 1}, None, True),
    ({'crop_cap': 2048}, None, True),                                    # = 1024 * n_slots
    ({'crop_cap': 2049}, f'{WHO}: crop_cap must be 1..1024 * slots (got 2049 for 2)', False),
    ({'slots.layout': 0}, f'{WHO}: the embedded job must state PVS_SLOTS_CROPPED (layout 0)', False),
    ({'slots.layout': 1}, f'{WHO}: the embedded job must state PVS_SLOTS_CROPPED (layout 1)', False),
    ({'slots.layout': 3}, f'{WHO}: the embedded job must state PVS_SLOTS_CROPPED (layout 3)', False),
    ({'slots.rec_drop': 1}, f"{WHO}: slots.rec_drop must be NULL (the copies' rec_drop is the job's own)", True),
    # the embedded job's refusals, under its entry's name
    ({'slots.lig_pos': 0}, f'{SLOTS_WHO}: NULL lig_pos', True),
    ({'slots.keep': 0}, f'{SLOTS_WHO}: NULL keep', True),
    ({'slots.status': 0}, f'{SLOTS_WHO}: NULL status', True),
    ({'slots.full.rowptr': 0}, f'{SLOTS_WHO}: NULL full.rowptr', True),
    ({'slots.lig.rowptr': 0}, None, True),                               # (cropped: no ligand-touching CSR)
    ({'slots.slot_cap': 1025}, f'{SLOTS_WHO}: slot_cap must be 1..1024 (got 1025)', False),
    ({'slots.lig_cap': 129}, f'{SLOTS_WHO}: needs slots, 1..64 * slots packed ligand atoms (got 129 for 2) and a receptor',
     False),
    ({'slots.n_rec': 0}, f'{SLOTS_WHO}: needs slots, 1..64 * slots packed ligand atoms (got 64 for 2) and a receptor',
     False),
    ({'slots.crop_radius': 0}, f'{SLOTS_WHO}: crop_radius must be positive (got 0)', True),
    ({'slots.tables.n_feats': -1}, f'{SLOTS_WHO}: negative table width', True),
    ({'slots.tables.base_magg': 1}, None, True),                         # (cropped: base tables dropped, not checked)
]


@pytest.fixture(scope='module')
def refusal(tmp_path_factory):
    exe = _compile(CXX, ['-std=c++17', '-O1'], PROGRAM, tmp_path_factory.mktemp('screen_copies') / 'copies_probe')

    def run(settings):
        res = subprocess.run([str(exe)] + [f'{k}={v}' for k, v in settings.items()], capture_output=True, text=True)
        assert res.returncode == 0, (res.returncode, res.stderr)
        return res.stdout.splitlines()
    return run


def test_every_refusal_names_its_cause(refusal):
    from pointvs_amd import _lib
    lib = _lib.lib()
    for settings, want, counts_ok in CASES:
        full, counts = refusal(settings)
        assert full == ('fine' if want is None else want), settings
        assert (counts == 'fine') == counts_ok, settings
        if not counts_ok:
            assert counts == full, settings
        # the loaded library's state size: nonzero exactly where the counts are accepted, and then that of the embedded job
        job = _lib.PvsScreenCopiesJob(crop_cap=settings.get('crop_cap', 64))
        s = job.slots
        s.layout, s.n_slots, s.lig_cap, s.n_rec, s.slot_cap = (settings.get('slots.' + k, v) for k, v in (
            ('layout', 2), ('n_slots', 2), ('lig_cap', 64), ('n_rec', 65), ('slot_cap', 64)))
        n = lib.pvs_screen_copies_state_bytes(C.byref(job))
        assert (n != 0) == counts_ok, settings
        if counts_ok:
            assert n == lib.pvs_screen_slots_state_bytes(C.byref(job.slots))
    assert lib.pvs_screen_copies_state_bytes(None) == 0


def _fake_job(_lib, fake=4096):
    job = _lib.PvsScreenCopiesJob(crop_pos=fake, crop_ptr=fake, crop_cap=64)
    s = job.slots
    s.layout, s.n_slots, s.lig_cap, s.n_rec, s.slot_cap = _lib.SLOTS_CROPPED, 2, 64, 65, 64
    s.inter_radius, s.intra_radius, s.crop_radius = 4.0, 2.0, 6.0
    for name in ('lig_pos', 'lig_ptr', 'rec_pos', 'rr_rowptr', 'rr_col', 'inv_deg', 'node_ptr', 'node_graph', 'pos',
                 'keep', 'status'):
        setattr(s, name, fake)
    s.full.rowptr = s.full.row = s.full.col = s.full.etype = fake
    return job


def test_the_library_refuses_by_name_before_any_launch():
    """Host checks return before any launch, so this runs without a GPU: pvs_last_error() names entry and cause."""
    from pointvs_amd import _lib
    from pointvs_amd import functional as PF
    lib, fake = _lib.lib(), 4096
    build = lambda job: lib.pvs_screen_copies_build(C.byref(job), fake, 1 << 20, None)      # noqa: E731
    job = _fake_job(_lib)
    job.crop_pos = None
    assert build(job) != 0 and lib.pvs_last_error() == b'pvs_screen_copies_build: NULL crop_pos'
    job = _fake_job(_lib)
    job.crop_ptr = None
    assert build(job) != 0 and lib.pvs_last_error() == b'pvs_screen_copies_build: NULL crop_ptr'
    job = _fake_job(_lib)
    job.crop_cap = 2049
    assert build(job) != 0
    assert lib.pvs_last_error() == b'pvs_screen_copies_build: crop_cap must be 1..1024 * slots (got 2049 for 2)'
    assert lib.pvs_screen_copies_state_bytes(C.byref(job)) == 0
    with pytest.raises(ValueError, match='crop_cap'):
        PF.screen_copies_state_bytes(job)
    job = _fake_job(_lib)
    job.slots.layout = _lib.SLOTS_RAGGED
    assert build(job) != 0
    assert lib.pvs_last_error() == b'pvs_screen_copies_build: the embedded job must state PVS_SLOTS_CROPPED (layout 0)'
    job = _fake_job(_lib)
    job.slots.rec_drop = fake
    assert build(job) != 0
    assert lib.pvs_last_error() == b"pvs_screen_copies_build: slots.rec_drop must be NULL (the copies' rec_drop is the job's own)"
    job = _fake_job(_lib)
    job.slots.keep = None                                  # the embedded job's refusals are still reached
    assert build(job) != 0 and lib.pvs_last_error() == b'pvs_screen_slots_build: NULL keep'
    job = _fake_job(_lib)
    assert lib.pvs_screen_copies_build(C.byref(job), fake, 16, None) != 0
    assert lib.pvs_last_error().startswith(b'pvs_screen_copies_build: state too small (16 < ')
    assert lib.pvs_screen_copies_build(None, fake, 16, None) != 0
    assert lib.pvs_last_error() == b'pvs_screen_copies_build: NULL job'
    # pvs_crop_keep and pvs_leave_out_parent_pack
    assert lib.pvs_crop_keep(fake, fake, 2, 8, fake, 0, 6.0, fake, fake, None) != 0
    assert lib.pvs_last_error() == b'pvs_crop_keep: 2 hits, 8 rows, 0 receptor atoms'
    assert lib.pvs_crop_keep(fake, fake, 2, 8, fake, 65, 0.0, fake, fake, None) != 0
    assert lib.pvs_last_error() == b'pvs_crop_keep: crop_radius must be positive (got 0)'
    assert lib.pvs_crop_keep(fake, fake, 2, 8, fake, 65, 6.0, None, fake, None) != 0
    assert lib.pvs_last_error() == b'pvs_crop_keep: NULL argument'
    assert lib.pvs_leave_out_parent_pack(fake, fake, fake, 2, 8, fake, 4, 1025, fake, fake, fake, None) != 0
    assert lib.pvs_last_error() == b'leave_out_parent_pack: 4 slots of up to 1025 atoms (1..1024)'
    assert lib.pvs_leave_out_parent_pack(fake, fake, None, 2, 8, fake, 4, 64, fake, fake, fake, None) != 0
    assert lib.pvs_last_error() == b'leave_out_parent_pack: NULL argument'
    assert lib.pvs_leave_out_parent_pack(fake, fake, fake, -1, 8, fake, 4, 64, fake, fake, fake, None) != 0
    assert lib.pvs_last_error() == b'leave_out_parent_pack: -1 hits, 8 rows'


def test_exports_prototypes_and_version():
    from pointvs_amd import _lib
    from pointvs_amd import functional as PF
    header = (INCLUDE / 'pvs_egnn.h').read_text()
    for name, n_args in (('pvs_screen_copies_state_bytes', 1), ('pvs_screen_copies_build', 4), ('pvs_crop_keep', 10),
                         ('pvs_leave_out_parent_pack', 12)):
        assert re.search(r'\b' + name + r'\s*\(', header), name
        assert name in _lib.EXPORTED_SYMBOLS and len(_lib._PROTOTYPES[name][1]) == n_args and hasattr(_lib.lib(), name)
    assert 'typedef struct PvsScreenCopiesJob {' in header
    # the library that has these entries is the one the binding asks for
    assert _lib.lib().pvs_version() >= _lib.MIN_VERSION >= 113
    for fn in (PF.screen_copies_state_bytes, PF.screen_copies_build, PF.crop_keep, PF.leave_out_parent_pack,
               PF.kept_atoms):
        assert callable(fn)


def test_the_references_against_scipy_cdist():
    from scipy.spatial.distance import cdist
    rng = np.random.default_rng(11)
    rec = (rng.random((130, 3)) * 20).astype(np.float32)
    parent = (rng.random((9, 3)) * 20).astype(np.float32)
    parent[0] = rec[7]                                                     # coincident: kept
    rec[8] = np.float32([-30.0, 3.0, 4.0])                                  # (far from every other atom)
    parent[1] = np.float32([-26.0, 3.0, 4.0])                               # exactly at the radius: not kept
    parent[2] = np.float32([50.0, 50.0, 50.0])
    rec[9] = np.float32([50.0, 53.0, 50.0])                                 # kept by atom 2 and by no other atom
    d = cdist(parent.astype(np.float64), rec.astype(np.float64))
    want = (d < 4.0).any(0)
    assert want[7] and want[9] and d[1, 8] == 4.0 and not want[8]
    assert np.array_equal(cref.keep_mask(parent, rec, 4.0), want)
    assert not cref.keep_mask(parent[:0], rec, 4.0).any()                    # an empty crop set keeps nothing
    for drop in (0, 7, 63, 64, 129):
        got = cref.keep_mask(parent, rec, 4.0, drop)
        struck = want.copy()
        struck[drop] = False
        assert np.array_equal(got, struck), drop
    assert np.array_equal(cref.keep_mask(parent, rec, 4.0, -1), want)
    # the copy's complex: the ligand without `skip`, then the parent's kept atoms without rec_drop
    feats, rec_feats = rng.random((9, 4)).astype(np.float32), rng.random((130, 4)).astype(np.float32)
    x, pos, kept = cref.copy_complex(feats, parent, rec_feats, rec, 4.0, skip=2, rec_drop=7)
    rows = [0, 1, 3, 4, 5, 6, 7, 8]
    assert kept.tolist() == [j for j in np.flatnonzero(want) if j != 7]
    assert np.array_equal(pos, np.concatenate([parent[rows], rec[kept]])) and np.array_equal(
        x, np.concatenate([feats[rows], rec_feats[kept]]))
    again = cref.recropped_complex(feats, parent, rec_feats, rec, 4.0, skip=2, rec_drop=7)[2]
    assert again.tolist() == [j for j in np.flatnonzero((d[rows] < 4.0).any(0)) if j != 7]
    only_by_2 = want & ~(d[rows] < 4.0).any(0)
    assert only_by_2[9] and set(np.flatnonzero(only_by_2)) == set(kept) - set(again)
    # packed hits
    lig_ptr = [0, 3, 3, 9]
    words, ptr = cref.hits_keep(parent, lig_ptr, rec, 4.0)
    assert words.shape == (3, 3) and ptr.tolist() == [0] + np.cumsum(
        [(d[lo:hi] < 4.0).any(0).sum() if hi > lo else 0 for lo, hi in zip(lig_ptr, lig_ptr[1:])]).tolist()
    assert ptr[2] == ptr[1]


def test_the_parent_packers_layout():
    pos = np.arange(27, dtype=np.float32).reshape(9, 3)
    lig_ptr = [0, 2, 2, 5, 9]                              # hits of 2, 0, 3 and 4 atoms
    # ligand-atom copies (copy_ptr = lig_ptr): hit s owns n_s + 1 copies: 3, 1, 4, 5
    assert cref.copy_hits(lig_ptr, 0, 14) == [0] * 3 + [1] + [2] * 4 + [3] * 5 + [-1]
    out, ptr = cref.parent_pack(pos, lig_ptr, lig_ptr, 2, 4)               # starts mid-hit
    assert ptr.tolist() == [0, 2, 2, 5, 8] and np.array_equal(out, np.concatenate([pos[0:2], pos[2:5], pos[2:5]]))
    # pair copies (copy_ptr = pair_ptr): 1, 3, 1 and 2 copies
    pair_ptr = [0, 0, 2, 2, 3]
    assert cref.copy_hits(pair_ptr, 0, 8) == [0, 1, 1, 1, 2, 3, 3, -1]
    out, ptr = cref.parent_pack(pos, lig_ptr, pair_ptr, 5, 4)              # runs past the last copy
    assert ptr.tolist() == [0, 4, 8, 8, 8] and np.array_equal(out, np.concatenate([pos[5:9], pos[5:9]]))
    out, ptr = cref.parent_pack(pos, lig_ptr, pair_ptr, 40, 2)
    assert ptr.tolist() == [0, 0, 0] and out.shape == (0, 3)


def test_the_keywords_are_opt_in_and_refuse_without_a_device():
    import torch
    from pointvs_amd.screening import LibraryScreen, ScreeningSweep
    from tests.test_gpu_screen_crop import _model
    assert inspect.signature(LibraryScreen.__init__).parameters['crop_parents'].default is False
    assert inspect.signature(ScreeningSweep.__init__).parameters['cropped_attribution'].default is False
    rec, rec_feats = torch.zeros((5, 3)), torch.zeros((5, 12))
    with pytest.raises(ValueError, match=r'crop_parents=True\) needs crop_radius'):
        LibraryScreen(_model(), rec, rec_feats, 2, 8, 4.0, crop_parents=True)
    with pytest.raises(ValueError, match=r'cropped_attribution=True\) needs crop_radius'):
        ScreeningSweep(_model(), rec, rec_feats, edge_radius=4.0, cropped_attribution=True)
    with pytest.raises(ValueError, match='crop_radius 3 is below the edge radius 4'):
        ScreeningSweep(_model(), rec, rec_feats, edge_radius=4.0, crop_radius=3.0, cropped_attribution=True)
    sweep = ScreeningSweep(_model(), rec, rec_feats, edge_radius=4.0, crop_radius=4.0, cropped_attribution=True)
    with pytest.raises(NotImplementedError, match='crop'):
        sweep.receptor_hotspots([])
    # the keyword off: the four refusals of a cropped sweep stand, word for word
    sweep = ScreeningSweep(_model(), rec, rec_feats, edge_radius=4.0, crop_radius=4.0)
    for method in (sweep.ligand_atom_masking, sweep.contact_masking, sweep.receptor_atom_masking,
                   sweep.receptor_hotspots):
        with pytest.raises(NotImplementedError, match='WHOLE ligand, so a copy must not be cropped again'):
            method([])
