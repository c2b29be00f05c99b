"""The slot layouts of the pose-batch builders and the shared table bisection (csrc/screen_slots.h), compiled alone
with the host compiler (CPU). The uniform layout (B poses of one ligand, by arithmetic) and the ragged layout (device
tables) must answer alike wherever both apply, the ragged layout must agree with a walk over the slots, and the one
bisection must agree with a linear scan and with the two formulations the kernels carried inline before they shared
it, restated here in Python from that source."""
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'pointvs_amd' / 'csrc'
CXX = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
BAD_TABLE = 8

# atoms: "a q valid a0 n_lig"; rows: "r g valid slot a0 n_lig node0 local"
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
        printf("r %d %d %d %d %d %d %d\n", g, (int)r.valid, r.slot, r.a0, r.n_lig, r.node0, r.local);
    }
}
int main(int argc, char** argv) {
    std::vector<int32_t> v;
    for (int i = 2; i < argc; ++i) v.push_back((int32_t)atoi(argv[i]));
    if (!strcmp(argv[1], "uniform")) {                  // B n_lig n_rec
        dump(PvsUniformSlots{v[0], v[1], v[2]});
    } else if (!strcmp(argv[1], "ragged")) {            // B L_cap n_rec status lig_ptr[B+1] node_ptr[B+1] slot_of[L_cap]
        const int B = v[0], L_cap = v[1];
        if ((int)v.size() != 4 + 2 * (B + 1) + L_cap) return 2;
        const int32_t status = v[3];
        const int32_t* lig_ptr = v.data() + 4;
        dump(PvsRaggedSlots{lig_ptr, lig_ptr + B + 1, lig_ptr + 2 * (B + 1), &status, B, L_cap, v[2]});
    } else {                                            // bisect n i_end table[...]
        for (int i = 0; i < v[1]; ++i) printf("%d\n", pvs_last_le(v.data() + 2, v[0], i));
    }
    return 0;
}
'''


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    if CXX is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('screen_slots')
    (d / 'main.cpp').write_text(PROGRAM)
    exe = d / 'screen_slots_probe'
    out = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', str(CSRC), str(d / 'main.cpp'), '-o', str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]

    def run(*args):
        text = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, check=True).stdout
        return [tuple(line.split()[:1]) + tuple(map(int, line.split()[1:])) if line[0] in 'ar' else int(line)
                for line in text.splitlines()]
    return run


def tables(sizes, n_rec):
    """lig_ptr, node_ptr and the atom -> slot table of a batch of slots with `sizes` ligand atoms."""
    lig_ptr = [0]
    for n in sizes:
        lig_ptr.append(lig_ptr[-1] + n)
    node_ptr = [a + p * n_rec for p, a in enumerate(lig_ptr)]
    slot_of = [p for p, n in enumerate(sizes) for _ in range(n)]
    return lig_ptr, node_ptr, slot_of


def ragged_args(sizes, n_rec, l_cap, status=0):
    lig_ptr, node_ptr, slot_of = tables(sizes, n_rec)
    return ('ragged', len(sizes), l_cap, n_rec, status, *lig_ptr, *node_ptr, *slot_of, *([-1] * (l_cap - len(slot_of))))


@pytest.mark.parametrize('shape', [(2, 1, 64), (2, 64, 65), (6, 17, 130)])
def test_ragged_layout_on_uniform_tables_answers_like_the_uniform_layout(program, shape):
    b, n_lig, n_rec = shape
    uniform = program('uniform', b, n_lig, n_rec)
    assert len(uniform) == b * n_lig + b * (n_lig + n_rec)
    assert uniform == program(*ragged_args([n_lig] * b, n_rec, b * n_lig))
    n = n_lig + n_rec                                  # and both say what the uniform builder computed inline
    want = [('a', q, 1, q // n_lig * n_lig, n_lig) for q in range(b * n_lig)]
    want += [('r', g, 1, g // n, g // n * n_lig, n_lig, g // n * n, g % n) for g in range(b * n)]
    assert uniform == want


@pytest.mark.parametrize('sizes', [(64, 0, 1, 64), (0, 0, 5, 0)])
def test_ragged_layout_agrees_with_a_walk_over_the_slots(program, sizes):
    n_rec, l_cap = 65, 64 * len(sizes)
    n_cap = l_cap + len(sizes) * n_rec
    lig_ptr, node_ptr, _ = tables(sizes, n_rec)
    invalid_atom, invalid_row = (0, 0, 0), (0, -1, 0, 0, 0, 0)
    want = []
    for p, n in enumerate(sizes):
        want += [('a', lig_ptr[p] + k, 1, lig_ptr[p], n) for k in range(n)]
    want += [('a', q) + invalid_atom for q in range(lig_ptr[-1], l_cap)]             # atoms from lig_ptr[B]: padding
    for p, n in enumerate(sizes):
        want += [('r', node_ptr[p] + k, 1, p, lig_ptr[p], n, node_ptr[p], k) for k in range(n + n_rec)]
    want += [('r', g) + invalid_row for g in range(node_ptr[-1], n_cap)]             # rows from node_ptr[B]: padding
    assert len(want) == l_cap + n_cap
    assert program(*ragged_args(sizes, n_rec, l_cap)) == want
    # the builder found lig_ptr to be no table: nothing is valid
    for status in (BAD_TABLE, BAD_TABLE | 4):
        got = program(*ragged_args(sizes, n_rec, l_cap, status))
        assert got == [('a', q) + invalid_atom for q in range(l_cap)] + [('r', g) + invalid_row for g in range(n_cap)]
    assert program(*ragged_args(sizes, n_rec, l_cap, 4)) == want                     # (the overflow bit alone is not it)


def slot_of_node_formerly(table, n, i):
    """screen_graph.hip's slot_of_node: closed interval [0, n - 1], upper middle."""
    lo, hi = 0, n - 1
    while lo < hi:
        mid = (lo + hi + 1) >> 1
        if table[mid] <= i:
            lo = mid
        else:
            hi = mid - 1
    return lo


def graph_of_row_formerly(table, n, i):
    """k_radius_fill's and k_complex_edges' search: half-open interval [0, n)."""
    lo, hi = 0, n
    while hi - lo > 1:
        mid = (lo + hi) >> 1
        if table[mid] <= i:
            lo = mid
        else:
            hi = mid
    return lo


@pytest.mark.parametrize('table', [
    tables((64, 0, 1, 64), 65)[1], tables((0, 0, 5, 0), 65)[1],          # node_ptr with empty slots (65 rows each)
    tables((1, 0, 2, 63, 64, 65, 128, 129, 0), 0)[0],                    # a graph_ptr with empty graphs, the last one too
    tables((0, 0, 3), 0)[0], tables((4,), 0)[0], tables((0, 1), 0)[0],
])
def test_bisection_agrees_with_a_linear_scan_and_both_former_searches(program, table):
    n, end = len(table) - 1, table[-1]
    got = program('bisect', n, end, *table)
    assert len(got) == end
    for i in range(end):
        linear = max(k for k in range(n) if table[k] <= i)
        assert table[linear] <= i < table[linear + 1]                    # (the last of equal entries: a non-empty owner)
        assert got[i] == linear == slot_of_node_formerly(table, n, i) == graph_of_row_formerly(table, n, i), i
