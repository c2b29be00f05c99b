"""Ligand-atom masking through the library screen, the host side (CPU): the slot sizes of the leave-one-atom-out batches
(screening.leave_out_plan), the copy enumeration the packer kernel bisects (csrc/leave_out.h, compiled alone with the host
compiler) against the same enumeration written out in Python, the new export and the scores-line format."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'pointvs_amd' / 'csrc'
CXX = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
SIZES = [0, 1, 2, 5, 64, 65, 130]


def test_plan_sizes_0_1_2_5_batch_3():
    from pointvs_amd.screening import leave_out_plan
    plan = leave_out_plan([0, 1, 2, 5], 3)
    # ligand 0: one empty copy; 1: whole + 1 copy of 0 atoms; 2: whole + 2 of 1; 5: whole + 5 of 4
    assert plan == [[0, 1, 0], [2, 1, 1], [5, 4, 4], [4, 4, 4]]
    assert sum(len(b) for b in plan) == sum([0, 1, 2, 5]) + 4 == 12         # every copy, no empty slot: 12 = 4 * 3
    assert leave_out_plan([0, 1, 2, 5], 5) == [[0, 1, 0, 2, 1], [1, 5, 4, 4, 4], [4, 4, 0, 0, 0]]      # empty trailing slots
    assert leave_out_plan([0, 1, 2, 5], 16) == [[0, 1, 0, 2, 1, 1, 5, 4, 4, 4, 4, 4, 0, 0, 0, 0]]
    assert leave_out_plan([], 4) == [] and leave_out_plan([0], 2) == [[0, 0]]
    assert leave_out_plan([3], 1) == [[3], [2], [2], [2]]
    for sizes, b in (([0, 1, 2, 5], 3), (SIZES, 7), ([7] * 9, 32)):
        plan = leave_out_plan(sizes, b)
        assert len(plan) == -(-(sum(sizes) + len(sizes)) // b) and all(len(batch) == b for batch in plan)
        assert sum(map(sum, plan)) == sum(n + n * (n - 1) for n in sizes)
    with pytest.raises(ValueError):
        leave_out_plan([1, 2], 0)
    with pytest.raises(ValueError):
        leave_out_plan([1, -2], 3)


def test_export_version_and_line_format():
    from pointvs_amd import _lib
    from pointvs_amd.predictions import format_lines
    header = (ROOT / 'include' / 'pvs_egnn.h').read_text()
    declared = set(re.findall(r'\b(pvs_[a-z0-9_]+)\s*\(', header))
    name = 'pvs_leave_out_ligand_pack'
    assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
    assert len(_lib._PROTOTYPES[name][1]) == 14
    assert _lib.MIN_VERSION >= 107 and _lib.lib().pvs_version() >= 107
    assert format_lines('atom_masking', [0.25, -1e-7], None, ['rec', 'rec'], ['lig_atom0', 'lig_atom1']) == \
        ['0.250000 | rec lig_atom0', '-0.000000 | rec lig_atom1']


# Prints every copy of the table given on the command line ("c <copy> <first> <n> <skip>"), two copy numbers outside it
# and the verdict on every entry of the table.
PROGRAM = r'''
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
    for (long long c = -1; c <= total + 1; ++c) {
        const PvsLeaveOutCopy v = pvs_leave_out_copy(ptr.data(), S, c);
        printf("c %lld %d %d %d\n", c, v.first, v.n, v.skip);
    }
    const PvsLeaveOutCopy far = pvs_leave_out_copy(ptr.data(), S, 3000000000ll);
    printf("far %d %d %d\n", far.first, far.n, far.skip);
    return 0;
}
'''


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    assert CXX is not None, 'the copy enumeration is checked with the host C++ compiler; none found'
    d = tmp_path_factory.mktemp('leave_out')
    (d / 'main.cpp').write_text(PROGRAM)
    exe = d / 'leave_out_probe'
    out = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', str(CSRC), str(d / 'main.cpp'), '-o', str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]

    def run(slot_cap, n_rows, ptr):
        res = subprocess.run([str(exe), str(slot_cap), str(n_rows)] + [str(p) for p in ptr], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        return res.stdout.splitlines()
    return run


def _ptr(sizes):
    ptr = [0]
    for n in sizes:
        ptr.append(ptr[-1] + n)
    return ptr


@pytest.mark.parametrize('sizes', [SIZES, [0, 0, 0], [3], [0], [], [1, 0, 1, 0, 0, 2], list(range(40))])
def test_copy_enumeration_matches_the_python_one(probe, sizes):
    from pointvs_amd.screening import leave_out_plan
    ptr = _ptr(sizes)
    lines = probe(1024, ptr[-1], ptr)
    assert lines[0] == 'ok 1'
    want = [(ptr[s], n, -1) if j == 0 else (ptr[s], n - 1, j - 1) for s, n in enumerate(sizes) for j in range(n + 1)]
    got = {int(f[1]): tuple(map(int, f[2:])) for f in (line.split() for line in lines) if f[0] == 'c'}
    assert len(want) == sum(sizes) + len(sizes)
    for c, w in enumerate(want):
        assert got[c] == w, (c, got[c], w)
    for c in (-1, len(want), len(want) + 1):         # outside the copies: nothing
        assert got[c] == (0, 0, -1), c
    assert lines[-1] == 'far 0 0 -1'
    flat = [n for batch in leave_out_plan(sizes, 7) for n in batch]       # the plan is these copies' sizes
    assert flat[:len(want)] == [w[1] for w in want] and not any(flat[len(want):])


def test_table_verdicts(probe):
    assert probe(130, 267, _ptr(SIZES))[0] == 'ok 1'
    assert probe(129, 267, _ptr(SIZES))[0] == 'ok 0'            # a ligand of slot_cap + 1 atoms
    assert probe(130, 266, _ptr(SIZES))[0] == 'ok 0'            # the table ends outside the rows
    assert probe(1024, 100, [0, 5, 3, 9])[0] == 'ok 0'          # descending
    assert probe(1024, 100, [1, 5, 9])[0] == 'ok 0'             # does not start at 0
    assert probe(1024, 100, [-2, 5, 9])[0] == 'ok 0'
    assert probe(1024, 0, [0])[0] == 'ok 1' and probe(1, 0, [0, 0])[0] == 'ok 1'
