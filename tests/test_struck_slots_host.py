"""The struck slot layout of the pose-batch builder (csrc/screen_slots.h: PvsStruckSlots and its helpers), compiled
alone with the host compiler (CPU): a slot whose receptor lacks one atom owns one row less, so the layout must agree
with a Python walk over the slots, must equal the ragged layout row for row when no slot is struck, and the helpers
(receptor numbering of a struck slot, membership in an ascending template row, the validity of a rec_drop entry)
must agree with their plain restatements here."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'pointvs_amd' / 'csrc'
CXX = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
BAD_TABLE = 8

# atoms: "a q valid a0 n_lig"; rows: "r g valid slot a0 n_lig node0 local drop"
PROGRAM = r'''
#include "screen_slots.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
template <class Slots>
static void dump(const Slots& L) {
    for (int q = 0; q < L.atoms(); ++q) {
        const PvsSlotAtom a = L.atom(q);
        printf("a %d %d %d %d\n", q, (int)a.valid, a.a0, a.n_lig);
    }
    for (int g = 0; g < L.rows(); ++g) {
        const PvsSlotRow r = L.row(g);
        printf("r %d %d %d %d %d %d %d %d\n", g, (int)r.valid, r.slot, r.a0, r.n_lig, r.node0, r.local, r.drop);
    }
}
int main(int argc, char** argv) {
    std::vector<int32_t> v;
    for (int i = 2; i < argc; ++i) v.push_back((int32_t)atoi(argv[i]));
    if (!strcmp(argv[1], "struck") || !strcmp(argv[1], "ragged")) {
        // B L_cap n_rec status lig_ptr[B+1] node_ptr[B+1] slot_of[L_cap] (struck: rec_drop[B])
        const int B = v[0], L_cap = v[1];
        const bool struck = argv[1][0] == 's';
        if ((int)v.size() != 4 + 2 * (B + 1) + L_cap + (struck ? B : 0)) return 2;
        const int32_t status = v[3];
        const int32_t* lig_ptr = v.data() + 4;
        const int32_t* slot_of = lig_ptr + 2 * (B + 1);
        if (struck) dump(PvsStruckSlots{lig_ptr, lig_ptr + B + 1, slot_of, &status, slot_of + L_cap, B, L_cap, v[2]});
        else dump(PvsRaggedSlots{lig_ptr, lig_ptr + B + 1, slot_of, &status, B, L_cap, v[2]});
    } else if (!strcmp(argv[1], "helpers")) {           // n_rec drop: "k receptor(k)" then "i row(i)", and drop_ok
        const int n_rec = v[0], drop = v[1];
        printf("%d\n", (int)pvs_rec_drop_ok(drop, n_rec));
        for (int k = 0; k < n_rec - (drop >= 0); ++k) printf("%d\n", pvs_struck_receptor(k, drop));
        for (int i = 0; i < n_rec; ++i) printf("%d\n", i == drop ? -1 : pvs_struck_row(i, drop));
    } else {                                            // find v_end row[...]: where 0 .. v_end-1 stand in the row
        for (int x = 0; x < v[0]; ++x) printf("%d\n", pvs_find_ascending(v.data() + 1, (int)v.size() - 1, x));
    }
    return 0;
}
'''


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    if CXX is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('struck_slots')
    (d / 'main.cpp').write_text(PROGRAM)
    exe = d / 'struck_slots_probe'
    out = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', str(CSRC), str(d / 'main.cpp'), '-o', str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]

    def run(*args):
        text = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, check=True).stdout
        return [tuple(line.split()[:1]) + tuple(map(int, line.split()[1:])) if line[0] in 'ar' else int(line)
                for line in text.splitlines()]
    return run


def tables(sizes, n_rec, rec_drop):
    """lig_ptr, node_ptr (a struck slot has one receptor row less) and the atom -> slot table."""
    lig_ptr, node_ptr = [0], [0]
    for n, r in zip(sizes, rec_drop):
        lig_ptr.append(lig_ptr[-1] + n)
        node_ptr.append(node_ptr[-1] + n + n_rec - (r >= 0))
    slot_of = [p for p, n in enumerate(sizes) for _ in range(n)]
    return lig_ptr, node_ptr, slot_of


def args(kind, sizes, n_rec, l_cap, rec_drop, status=0):
    lig_ptr, node_ptr, slot_of = tables(sizes, n_rec, rec_drop)
    tail = list(rec_drop) if kind == 'struck' else []
    return (kind, len(sizes), l_cap, n_rec, status, *lig_ptr, *node_ptr, *slot_of, *([-1] * (l_cap - len(slot_of))), *tail)


SIZES, N_REC, L_CAP = [0, 2, 1, 0, 3], 3, 8


def test_struck_layout_agrees_with_a_walk_over_the_slots(program):
    rec_drop = [-1, 0, 2, 1, -1]
    lig_ptr, node_ptr, _ = tables(SIZES, N_REC, rec_drop)
    # node_ptr[p] = lig_ptr[p] + p * n_rec - (struck slots before p)
    assert node_ptr == [lig_ptr[p] + p * N_REC - sum(r >= 0 for r in rec_drop[:p]) for p in range(len(SIZES) + 1)]
    n_cap = L_CAP + len(SIZES) * N_REC
    want = []
    for p, n in enumerate(SIZES):
        want += [('a', lig_ptr[p] + k, 1, lig_ptr[p], n) for k in range(n)]
    want += [('a', q, 0, 0, 0) for q in range(lig_ptr[-1], L_CAP)]
    for p, (n, r) in enumerate(zip(SIZES, rec_drop)):
        rows = n + N_REC - (r >= 0)
        want += [('r', node_ptr[p] + k, 1, p, lig_ptr[p], n, node_ptr[p], k, r) for k in range(rows)]
    want += [('r', g, 0, -1, 0, 0, 0, 0, -1) for g in range(node_ptr[-1], n_cap)]
    assert node_ptr[-1] == sum(SIZES) + len(SIZES) * N_REC - 3 and len(want) == L_CAP + n_cap
    assert program(*args('struck', SIZES, N_REC, L_CAP, rec_drop)) == want


def test_unstruck_table_equals_the_ragged_layout_row_for_row(program):
    rec_drop = [-1] * len(SIZES)
    struck = program(*args('struck', SIZES, N_REC, L_CAP, rec_drop))
    ragged = program(*args('ragged', SIZES, N_REC, L_CAP, rec_drop))
    assert struck == ragged and all(line[-1] == -1 for line in struck if line[0] == 'r')
    assert sum(1 for line in struck if line[0] == 'r' and line[2]) == sum(SIZES) + len(SIZES) * N_REC


def test_bad_table_makes_nothing_valid(program):
    """What the builder's first kernel finds (an entry of rec_drop outside -1..n_rec-1, or a bad lig_ptr) is the status
    word's bit 3: no atom and no row is valid then, whatever the tables hold."""
    assert program('helpers', N_REC, N_REC)[0] == 0 and program('helpers', N_REC, -2)[0] == 0
    n_cap = L_CAP + len(SIZES) * N_REC
    for status in (BAD_TABLE, BAD_TABLE | 4):
        got = program(*args('struck', SIZES, N_REC, L_CAP, [-1, 0, N_REC, 1, -2], status))
        assert got == [('a', q, 0, 0, 0) for q in range(L_CAP)] + [('r', g, 0, -1, 0, 0, 0, 0, -1) for g in range(n_cap)]


@pytest.mark.parametrize('n_rec,drop', [(3, -1), (3, 0), (3, 2), (130, 64), (1, 0)])
def test_receptor_numbering_of_a_struck_slot(program, n_rec, drop):
    got = program('helpers', n_rec, drop)
    kept = [i for i in range(n_rec) if i != drop]
    assert got[0] == 1
    assert got[1:1 + len(kept)] == kept                                          # row k of the slot -> receptor atom
    assert got[1 + len(kept):] == [kept.index(i) if i != drop else -1 for i in range(n_rec)]    # and back


@pytest.mark.parametrize('row', [[], [4], [0, 1, 2, 3], [1, 5, 6, 64, 65, 129], [2, 9]])
def test_membership_in_an_ascending_row(program, row):
    assert program('find', 131, *row) == [row.index(x) if x in row else -1 for x in range(131)]
