"""Contact and receptor-atom masking through the library screen, the host side (CPU): the batches of the pair copies
(screening.leave_out_pair_plan), the copy enumeration the pair packer bisects (csrc/leave_out.h, compiled alone with
the host compiler) against the same enumeration written out in Python, the new exports and the version."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'pointvs_amd' / 'csrc'
CXX = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')


def test_plan_with_empty_tables_and_empty_hits():
    from pointvs_amd.screening import leave_out_pair_plan
    sizes, counts = [0, 3, 1, 5, 2], [0, 2, 0, 4, 1]
    # hit 0: the empty whole; 1: whole + 2 copies of 2 atoms; 2: whole alone; 3: whole + 4 of 4; 4: whole + 1 of 1
    plan = leave_out_pair_plan(counts, sizes, 4)
    assert plan == [([0, 3, 2, 2], 2), ([1, 5, 4, 4], 2), ([4, 4, 2, 1], 3)]
    # the last batch partly empty; totals
    plan = leave_out_pair_plan(counts, sizes, 5)
    assert plan == [([0, 3, 2, 2, 1], 2), ([5, 4, 4, 4, 4], 4), ([2, 1, 0, 0, 0], 1)]
    for b in (1, 3, 4, 5, 7, 64):
        plan = leave_out_pair_plan(counts, sizes, b)
        assert len(plan) == -(-(sum(counts) + len(sizes)) // b) and all(len(batch) == b for batch, _ in plan)
        assert sum(sum(batch) for batch, _ in plan) == sum(n + k * (n - 1) for n, k in zip(sizes, counts))
        assert sum(struck for _, struck in plan) == sum(counts)
    # receptor-atom copies keep the whole ligand, and a hit of 0 atoms may have them
    plan = leave_out_pair_plan([2, 1], [0, 3], 3, ligand_atom=False)
    assert plan == [([0, 0, 0], 2), ([3, 3, 0], 1)]
    # ligand-atom-only tables strike nothing
    assert leave_out_pair_plan([2], [3], 4, receptor_atom=False) == [([3, 2, 2, 0], 0)]
    assert leave_out_pair_plan([], [], 4) == [] and leave_out_pair_plan([0], [0], 2) == [([0, 0], 0)]
    with pytest.raises(ValueError):
        leave_out_pair_plan([1], [0], 4)            # a contact of a hit without atoms
    with pytest.raises(ValueError):
        leave_out_pair_plan([1, 2], [3], 4)
    with pytest.raises(ValueError):
        leave_out_pair_plan([1], [3], 0)
    with pytest.raises(ValueError):
        leave_out_pair_plan([-1], [3], 2)


def test_exports_and_version():
    from pointvs_amd import _lib
    header = (ROOT / 'include' / 'pvs_egnn.h').read_text()
    declared = set(re.findall(r'\b(pvs_[a-z0-9_]+)\s*\(', header))
    widths = {'pvs_contact_pairs_count': 9, 'pvs_contact_pairs_fill': 11, 'pvs_leave_out_pair_pack': 19}
    for name, n_args in widths.items():
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name), name
        assert len(_lib._PROTOTYPES[name][1]) == n_args, name
    # the slot builders of every layout (struck: the ragged one plus rec_drop) are one entry pair on one job struct
    # (its layout against the C compiler's: test_screen_job_host.py); the eight positional entries before it are gone
    for name in ('pvs_screen_slots_state_bytes', 'pvs_screen_slots_build'):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name), name
    for layout in ('ragged', 'ragged_cap', 'struck', 'cropped'):
        for name in (f'pvs_screen_graph_{layout}_state_bytes', f'pvs_screen_graph_build_{layout}'):
            assert name not in declared and name not in _lib.EXPORTED_SYMBOLS and not hasattr(_lib.lib(), name), name
    assert _lib.MIN_VERSION >= 113 and _lib.lib().pvs_version() >= 113


def test_the_library_refuses_a_job_by_name_before_any_launch():
    """Host checks return before any launch, so this runs without a GPU: pvs_last_error() names entry and cause."""
    import ctypes as C
    from pointvs_amd import _lib
    lib = _lib.lib()
    fake = 4096         # (an address that no refusal reads)
    job = _lib.PvsScreenSlotsJob(
        layout=_lib.SLOTS_STRUCK, n_slots=2, lig_cap=64, n_rec=65, slot_cap=64, inter_radius=4.0, intra_radius=2.0,
        **{name: fake for name in ('lig_pos', 'lig_ptr', 'rec_pos', 'rr_rowptr', 'rr_col', 'inv_deg', 'node_ptr',
                                   'node_graph', 'pos', 'status')})
    for csr in (job.full, job.lig):
        csr.rowptr = csr.row = csr.col = csr.etype = fake
    assert lib.pvs_screen_slots_build(C.byref(job), fake, 1 << 20, None) != 0
    assert lib.pvs_last_error() == b'pvs_screen_slots_build: NULL rec_drop'
    job.layout, job.slot_cap = _lib.SLOTS_RAGGED, 1025
    assert lib.pvs_screen_slots_build(C.byref(job), fake, 1 << 20, None) != 0
    assert lib.pvs_last_error() == b'pvs_screen_slots_build: slot_cap must be 1..1024 (got 1025)'
    assert lib.pvs_screen_slots_state_bytes(C.byref(job)) == 0


# argv: K n_rec pair_ptr[...]. Prints the verdict on the table, every copy ("c <copy> <hit> <pair>") and two outside it.
PROGRAM = r'''
#include "leave_out.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>
int main(int argc, char** argv) {
    const int K = atoi(argv[1]);
    std::vector<int32_t> ptr;
    for (int i = 2; i < argc; ++i) ptr.push_back(atoi(argv[i]));
    const int S = (int)ptr.size() - 1;
    int ok = 1;
    for (int t = 0; t <= S; ++t) ok &= pvs_pair_table_ok(ptr.data(), S, t, K) ? 1 : 0;
    printf("ok %d\n", ok);
    if (!ok) return 0;
    const long long total = (long long)ptr[S] + S;
    for (long long c = -2; c <= total + 2; ++c) {
        const PvsPairCopy v = pvs_pair_copy(ptr.data(), S, c);
        printf("c %lld %d %d\n", c, v.hit, v.pair);
    }
    const PvsPairCopy far = pvs_pair_copy(ptr.data(), S, 3000000000ll);
    printf("far %d %d\n", far.hit, far.pair);
    printf("pairs %d%d%d%d%d%d\n", (int)pvs_pair_ok(-1, -1, 0, 1), (int)pvs_pair_ok(4, 6, 5, 7), (int)pvs_pair_ok(5, 6, 5, 7),
           (int)pvs_pair_ok(4, 7, 5, 7), (int)pvs_pair_ok(-2, 0, 5, 7), (int)pvs_pair_ok(0, -2, 5, 7));
    return 0;
}
'''


# The same for the ligand-atom copies. argv: slot_cap n_rows lig_ptr[...]. Prints the verdict on the table and every copy
# ("c <copy> <first> <n> <skip>"), two on either side of them included.
LIGAND_PROGRAM = r'''
#include "leave_out.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>
int main(int argc, char** argv) {
    const int slot_cap = atoi(argv[1]), n_rows = atoi(argv[2]);
    std::vector<int32_t> ptr;
    for (int i = 3; i < argc; ++i) ptr.push_back(atoi(argv[i]));
    const int S = (int)ptr.size() - 1;
    int ok = 1;
    for (int t = 0; t <= S; ++t) ok &= pvs_leave_out_table_ok(ptr.data(), S, t, slot_cap, n_rows) ? 1 : 0;
    printf("ok %d\n", ok);
    if (!ok) return 0;
    const long long total = (long long)ptr[S] + S;
    for (long long c = -2; c <= total + 2; ++c) {
        const PvsLeaveOutCopy v = pvs_leave_out_copy(ptr.data(), S, c);
        printf("c %lld %d %d %d\n", c, v.first, v.n, v.skip);
    }
    return 0;
}
'''


def _compiled(tmp_path_factory, name, program):
    assert CXX is not None, 'the copy enumeration is checked with the host C++ compiler; none found'
    d = tmp_path_factory.mktemp(name)
    (d / 'main.cpp').write_text(program)
    exe = d / f'{name}_probe'
    out = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', str(CSRC), str(d / 'main.cpp'), '-o', str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]

    def run(*args):
        res = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        return res.stdout.splitlines()
    return run


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    run = _compiled(tmp_path_factory, 'pair_copy', PROGRAM)
    return lambda n_pairs, ptr: run(n_pairs, *ptr)


@pytest.fixture(scope='module')
def ligand_probe(tmp_path_factory):
    run = _compiled(tmp_path_factory, 'ligand_copy', LIGAND_PROGRAM)
    return lambda slot_cap, n_rows, ptr: run(slot_cap, n_rows, *ptr)


def _ptr(counts):
    ptr = [0]
    for n in counts:
        ptr.append(ptr[-1] + n)
    return ptr


@pytest.mark.parametrize('counts', [[0, 2, 0, 4, 1], [0, 0, 0], [3], [0], [], [85], list(range(30))])
def test_pair_copy_enumeration_matches_the_python_one(probe, counts):
    ptr = _ptr(counts)
    lines = probe(ptr[-1], ptr)
    assert lines[0] == 'ok 1'
    want = [(s, -1 if j == 0 else ptr[s] + j - 1) for s, k in enumerate(counts) for j in range(k + 1)]
    got = {int(f[1]): tuple(map(int, f[2:])) for f in (line.split() for line in lines) if f[0] == 'c'}
    assert len(want) == sum(counts) + len(counts)
    for c, w in enumerate(want):
        assert got[c] == w, (c, got[c], w)
    assert sorted(w[1] for w in want if w[1] >= 0) == list(range(ptr[-1]))       # every row of the table, once
    for c in (-1, len(want), len(want) + 1):         # outside the copies: nothing
        assert got[c] == (-1, -1), c
    assert lines[-2] == 'far -1 -1' and lines[-1] == 'pairs 110000'


def test_pair_table_verdicts(probe):
    assert probe(7, [0, 2, 2, 6, 7])[0] == 'ok 1'
    assert probe(8, [0, 2, 2, 6, 7])[0] == 'ok 1'               # (a table may use fewer rows than there are)
    assert probe(6, [0, 2, 2, 6, 7])[0] == 'ok 0'               # ends outside the rows
    assert probe(9, [0, 5, 3, 9])[0] == 'ok 0'                  # descending
    assert probe(9, [1, 5, 9])[0] == 'ok 0'                     # does not start at 0
    assert probe(0, [0])[0] == 'ok 1' and probe(0, [0, 0])[0] == 'ok 1'


@pytest.mark.parametrize('n_hits', [257, 513])
def test_both_enumerations_over_257_and_513_hits(probe, ligand_probe, n_hits):
    """The tables the packer tests of tests/test_gpu_many_slots.py use - empty hits at both ends, at 255 / 256 and every
    50th, hits without pairs - bisected over 9 and 10 levels: every copy number in [-2, total + 2] of both numberings."""
    from tests import _many_slots_cases as mc
    sizes = mc.hit_sizes(n_hits)
    counts = [len(hit) for hit in mc.hit_pairs(sizes, mc.N_REC)]
    assert sizes[0] == sizes[255] == sizes[256] == sizes[-1] == sizes[100] == 0 and counts[0] == counts[-1] == 0
    cases = [(probe(sum(counts), _ptr(counts)), counts,
              [(s, -1 if j == 0 else _ptr(counts)[s] + j - 1) for s, k in enumerate(counts) for j in range(k + 1)], (-1, -1)),
             (ligand_probe(9, sum(sizes), _ptr(sizes)), sizes,
              [(_ptr(sizes)[s], n, -1) if j == 0 else (_ptr(sizes)[s], n - 1, j - 1)
               for s, n in enumerate(sizes) for j in range(n + 1)], (0, 0, -1))]
    for lines, table, want, nothing in cases:
        assert lines[0] == 'ok 1'
        got = {int(f[1]): tuple(map(int, f[2:])) for f in (line.split() for line in lines) if f[0] == 'c'}
        total = sum(table) + n_hits
        assert len(want) == total and sorted(got) == list(range(-2, total + 3))
        for c in range(-2, total + 3):
            assert got[c] == (want[c] if 0 <= c < total else nothing), (c, got[c])
    assert ligand_probe(8, sum(sizes), _ptr(sizes))[0] == 'ok 0'            # (the 9-atom hit is wider than 8)
    late = _ptr(sizes)
    late[n_hits - 2] = late[n_hits - 3] - 1                                 # one descending pair, two entries from the end
    assert ligand_probe(9, sum(sizes), late)[0] == 'ok 0'
