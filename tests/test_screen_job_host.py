"""The pose-batch slot builders' job (PvsScreenSlotsJob, pvs_screen_slots_build), the host side (CPU): the struct
layouts of the ctypes binding against the C compiler's, field by field and by name (the public header compiles as C11), and the
refusals (csrc/screen_job.h, compiled alone with the host compiler) one by one from an acceptable job of every layout -
with pvs_screen_slots_state_bytes of the loaded library nonzero exactly where the counts are accepted."""
import ctypes as C
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'pointvs_amd' / 'csrc'
INCLUDE = ROOT / 'include'
CC = shutil.which('cc') or shutil.which('gcc') or shutil.which('clang')
CXX = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
WHO = 'pvs_screen_slots_build'

# The fields as include/pvs_egnn.h declares them, in order.
FIELDS = {
    'PvsCsrOut': ['rowptr', 'row', 'col', 'etype', 'capacity'],
    'PvsRaggedNodeTables': ['n_feats', 'hidden', 'lig_feats', 'rec_feats', 'rec_magg', 'rec_xsum', 'rec_deg', 'feats',
                            'base_magg', 'base_xsum', 'base_deg'],
    'PvsScreenSlotsJob': ['layout', 'lig_pos', 'lig_ptr', 'rec_drop', 'rec_pos', 'rr_rowptr', 'rr_col', 'n_slots',
                          'lig_cap', 'n_rec', 'slot_cap', 'inter_radius', 'intra_radius', 'crop_radius', 'full', 'lig',
                          'inv_deg', 'node_ptr', 'node_graph', 'pos', 'keep', 'tables', 'status'],
}


def _compile(compiler, flags, source, exe):
    assert compiler is not None, 'the job struct is checked with the host compiler; none found'
    source_file = exe.with_suffix('.cpp' if compiler == CXX else '.c')
    source_file.write_text(source)
    out = subprocess.run([compiler] + flags + ['-Wall', '-Werror', '-I', str(CSRC), '-I', str(INCLUDE),
                          str(source_file), '-o', str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return exe


def test_binding_layouts_are_the_c_compilers(tmp_path):
    from pointvs_amd import _lib
    lines = ['#include "pvs_egnn.h"', '#include <stddef.h>', '#include <stdio.h>', 'int main(void) {']
    for struct, names in FIELDS.items():
        lines.append(f'    printf("{struct} sizeof %zu\\n", sizeof({struct}));')
        lines += [f'    printf("{struct} {n} %zu %zu\\n", offsetof({struct}, {n}), sizeof((({struct}*)0)->{n}));'
                  for n in names]
    exe = _compile(CC, ['-std=c11'], '\n'.join(lines + ['    return 0;', '}', '']), tmp_path / 'layout')
    want = [tuple(line.split()) for line in subprocess.run([str(exe)], capture_output=True, text=True,
                                                           check=True).stdout.splitlines()]
    got = []
    for struct, names in FIELDS.items():
        cls = getattr(_lib, struct)
        assert [n for n, _ in cls._fields_] == names, struct
        got.append((struct, 'sizeof', str(C.sizeof(cls))))
        got += [(struct, n, str(getattr(cls, n).offset), str(getattr(cls, n).size)) for n in names]
    assert got == want
    assert (_lib.SLOTS_RAGGED, _lib.SLOTS_STRUCK, _lib.SLOTS_CROPPED) == (0, 1, 2)
    header = (INCLUDE / 'pvs_egnn.h').read_text()
    assert 'enum { PVS_SLOTS_RAGGED = 0, PVS_SLOTS_STRUCK = 1, PVS_SLOTS_CROPPED = 2 };' in header


# argv: layout, then field=value settings on top of that layout's acceptable job (a pointer field: 0 = NULL, else some
# address). Prints the refusal of the whole job, the refusal of its counts alone ("fine" for none) and whether the
# tables that the kernels would get still have base rows.
PROGRAM = r'''
#include "screen_job.h"
#include <stdlib.h>
#include <string>
static int32_t some[4];
static bool set(PvsScreenSlotsJob& j, const std::string& key, const char* val) {
    const long v = atol(val);
#define PTR(f) if (key == #f) { j.f = v ? (decltype(j.f))(void*)some : nullptr; return true; }
#define INT(f) if (key == #f) { j.f = (int32_t)v; return true; }
#define DBL(f) if (key == #f) { j.f = atof(val); return true; }
    INT(layout) PTR(lig_pos) PTR(lig_ptr) PTR(rec_drop) PTR(rec_pos) PTR(rr_rowptr) PTR(rr_col)
    INT(n_slots) INT(lig_cap) INT(n_rec) INT(slot_cap) DBL(inter_radius) DBL(intra_radius) DBL(crop_radius)
    PTR(full.rowptr) PTR(full.row) PTR(full.col) PTR(full.etype) INT(full.capacity)
    PTR(lig.rowptr) PTR(lig.row) PTR(lig.col) PTR(lig.etype) INT(lig.capacity)
    PTR(inv_deg) PTR(node_ptr) PTR(node_graph) PTR(pos) PTR(keep) PTR(status)
    INT(tables.n_feats) INT(tables.hidden) PTR(tables.lig_feats) PTR(tables.rec_feats) PTR(tables.rec_magg)
    PTR(tables.rec_xsum) PTR(tables.rec_deg) PTR(tables.feats) PTR(tables.base_magg) PTR(tables.base_xsum)
    PTR(tables.base_deg)
    return false;
}
int main(int argc, char** argv) {
    PvsScreenSlotsJob j = {};
    j.layout = atoi(argv[1]);
    for (const char* f : {"lig_pos", "lig_ptr", "rec_pos", "rr_rowptr", "rr_col", "full.rowptr", "full.row", "full.col",
                          "full.etype", "inv_deg", "node_ptr", "node_graph", "pos", "status"}) set(j, f, "1");
    if (j.layout != PVS_SLOTS_CROPPED)
        for (const char* f : {"lig.rowptr", "lig.row", "lig.col", "lig.etype"}) set(j, f, "1");
    if (j.layout == PVS_SLOTS_STRUCK) set(j, "rec_drop", "1");
    if (j.layout == PVS_SLOTS_CROPPED) { set(j, "keep", "1"); j.crop_radius = 6.0; }
    j.n_slots = 2; j.lig_cap = 64; j.n_rec = 65; j.slot_cap = 64; j.inter_radius = 4.0; j.intra_radius = 2.0;
    for (int i = 2; i < argc; ++i) {
        const std::string arg = argv[i];
        const size_t eq = arg.find('=');
        if (eq == std::string::npos || !set(j, arg.substr(0, eq), arg.c_str() + eq + 1)) return 2;
    }
    char why[256], why_counts[256];
    const char* full = pvs_screen_job_refusal(j, false, why, sizeof(why));
    const char* counts = pvs_screen_job_refusal(j, true, why_counts, sizeof(why_counts));
    printf("%s\n%s\nbase %d\n", full ? full : "fine", counts ? counts : "fine",
           pvs_screen_job_tables(j).base_magg ? 1 : 0);
    return 0;
}
'''

RAGGED, STRUCK, CROPPED = 0, 1, 2
COMMON_POINTERS = ['lig_pos', 'lig_ptr', 'rec_pos', 'rr_rowptr', 'rr_col', 'full.rowptr', 'full.row', 'full.col',
                   'full.etype', 'inv_deg', 'node_ptr', 'node_graph', 'pos', 'status']
LIG_CSR = ['lig.rowptr', 'lig.row', 'lig.col', 'lig.etype']
REQUIRED = {RAGGED: COMMON_POINTERS + LIG_CSR, STRUCK: COMMON_POINTERS + LIG_CSR + ['rec_drop'],
            CROPPED: COMMON_POINTERS + ['keep']}
FEATS = {'tables.n_feats': 12, 'tables.lig_feats': 1, 'tables.rec_feats': 1, 'tables.feats': 1}
BASE = {'tables.hidden': 32, 'tables.rec_magg': 1, 'tables.rec_xsum': 1, 'tables.rec_deg': 1, 'tables.base_magg': 1,
        'tables.base_xsum': 1, 'tables.base_deg': 1}
SLOTS_NEEDED = 'needs slots, 1..{} * slots packed ligand atoms (got {} for {}) and a receptor'


def _cases():
    """(layout, settings, the refusal's text behind the entry's name or None for an accepted job, whether the counts
    alone are accepted)."""
    cases = [(layout, {}, None, True) for layout in REQUIRED]
    for layout, names in REQUIRED.items():
        cases += [(layout, {name: 0}, f'NULL {name}', True) for name in names]
    for layout in REQUIRED:
        cases += [
            (layout, dict(slot_cap=0), 'slot_cap must be 1..1024 (got 0)', False),
            (layout, dict(slot_cap=1, lig_cap=2), None, True),
            (layout, dict(slot_cap=1024), None, True),
            (layout, dict(slot_cap=1025), 'slot_cap must be 1..1024 (got 1025)', False),
            (layout, dict(lig_cap=128), None, True),                       # = slot_cap * n_slots
            (layout, dict(lig_cap=129), SLOTS_NEEDED.format(64, 129, 2), False),
            (layout, dict(lig_cap=0), SLOTS_NEEDED.format(64, 0, 2), False),
            (layout, dict(n_rec=0), SLOTS_NEEDED.format(64, 64, 2), False),
            (layout, dict(n_slots=0), SLOTS_NEEDED.format(64, 64, 0), False),
            # the node-count edge: 2 147 483 646 nodes are taken, 2 147 483 647 are not
            (layout, dict(n_slots=2, slot_cap=1024, n_rec=1073741311, lig_cap=1024), None, True),
            (layout, dict(n_slots=2, slot_cap=1024, n_rec=1073741311, lig_cap=1025), 'more than 2^31 nodes', False),
            # the table rules
            (layout, FEATS, None, True),
            (layout, {'tables.n_feats': -1}, 'negative table width', True),
            (layout, dict(FEATS, **{'tables.lig_feats': 0}), 'feature table without sources', True),
            (layout, dict(FEATS, **{'tables.rec_feats': 0}), 'feature table without sources', True),
            (layout, dict(FEATS, **{'tables.n_feats': 0}), 'feature table without sources', True),
        ]
    for layout in (RAGGED, STRUCK):
        cases += [(layout, BASE, None, True), (layout, dict(FEATS, **BASE), None, True),
                  (layout, {'tables.hidden': -1}, 'negative table width', True)]
        cases += [(layout, dict(BASE, **{name: 0}), 'receptor sums incomplete', True) for name in BASE
                  if name != 'tables.base_magg']
    # under CROPPED the base tables are dropped, not checked
    cases += [(CROPPED, dict(BASE, **{name: 0}), None, True) for name in BASE]
    cases += [(CROPPED, dict(BASE, **{'tables.hidden': -1}), None, True)]
    # the layout is stated, and what does not go with it is refused by name
    cases += [
        (CROPPED, dict(crop_radius=0), 'crop_radius must be positive (got 0)', True),
        (CROPPED, dict(crop_radius=-1), 'crop_radius must be positive (got -1)', True),
        (RAGGED, dict(rec_drop=1), 'rec_drop goes with PVS_SLOTS_STRUCK only (layout 0)', True),
        (CROPPED, dict(rec_drop=1), 'rec_drop goes with PVS_SLOTS_STRUCK only (layout 2)', True),
        (RAGGED, dict(crop_radius=6), 'crop_radius goes with PVS_SLOTS_CROPPED only (layout 0)', True),
        (STRUCK, dict(crop_radius=6), 'crop_radius goes with PVS_SLOTS_CROPPED only (layout 1)', True),
        (RAGGED, dict(keep=1), None, True),         # (an output that the layout does not write: ignored)
        (3, {}, 'unknown layout 3', False),
        (-1, {}, 'unknown layout -1', False),
    ]
    return cases


CASES = _cases()


@pytest.fixture(scope='module')
def refusal(tmp_path_factory):
    exe = _compile(CXX, ['-std=c++17', '-O1'], PROGRAM, tmp_path_factory.mktemp('screen_job') / 'screen_job_probe')

    def run(layout, settings):
        res = subprocess.run([str(exe), str(layout)] + [f'{k}={v}' for k, v in settings.items()], capture_output=True,
                             text=True)
        assert res.returncode == 0, (res.returncode, res.stderr)
        full, counts, base = res.stdout.splitlines()
        return full, counts, base == 'base 1'
    return run


def test_every_refusal_names_its_cause(refusal):
    from pointvs_amd import _lib
    lib = _lib.lib()
    assert len(CASES) == 138
    for layout, settings, want, counts_ok in CASES:
        what = (layout, settings)
        full, counts, base = refusal(layout, settings)
        assert full == ('fine' if want is None else f'{WHO}: {want}'), what
        assert (counts == 'fine') == counts_ok, what
        if not counts_ok:
            assert counts == full, what          # (the count part of the same function: the same words)
        # base rows reach the kernels only from an uncropped job that has them
        assert base == (layout != CROPPED and settings.get('tables.base_magg') == 1), what
        # the loaded library's state size: nonzero exactly where the counts are accepted (it reads no pointer)
        job = _lib.PvsScreenSlotsJob(layout=layout, n_slots=2, lig_cap=64, n_rec=65, slot_cap=64)
        for key in ('n_slots', 'lig_cap', 'n_rec', 'slot_cap'):
            setattr(job, key, settings.get(key, getattr(job, key)))
        assert (lib.pvs_screen_slots_state_bytes(C.byref(job)) != 0) == counts_ok, what
    assert lib.pvs_screen_slots_state_bytes(None) == 0
