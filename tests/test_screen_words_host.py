"""The word / bit arithmetic of the pose-batch builders' ligand-side masks (csrc/screen_slots.h: pvs_slot_words,
pvs_slot_word, pvs_slot_bit, pvs_mask_rank, the layouts' words()), compiled alone with the host compiler (CPU) and
compared with a Python restatement on big integers. A ligand atom's contacts with the up to 1,024 atoms of its slot are
ceil(cap / 64) words; pvs_mask_rank is the offset k_fill writes an entry at. The layouts built the way they were before
slots could be wider than one word (no slot_cap given) must answer exactly as they did."""
import random
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'pointvs_amd' / 'csrc'
CXX = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
CAPS = (1, 63, 64, 65, 128, 129, 1024)

PROGRAM = r'''
#include "screen_slots.h"
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
template <class Slots>
static void dump(const Slots& L) {
    printf("w %d\n", L.words());
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
    if (argc < 2) return 2;
    if (!strcmp(argv[1], "cap")) {                      // cap: words, then word and bit of every atom of the slot
        const int cap = atoi(argv[2]);
        printf("%d\n", pvs_slot_words(cap));
        for (int k = 0; k < cap; ++k) printf("%d %d\n", pvs_slot_word(k), pvs_slot_bit(k));
    } else if (!strcmp(argv[1], "rank")) {              // hex words: "word bit rank" of every set bit, ascending
        std::vector<unsigned long long> m;
        for (int i = 2; i < argc; ++i) m.push_back(strtoull(argv[i], nullptr, 16));
        for (int w = 0; w < (int)m.size(); ++w)
            for (int b = 0; b < 64; ++b)
                if ((m[w] >> b) & 1ull) printf("%d %d %d\n", w, b, pvs_mask_rank(m.data(), w, b));
    } else if (!strcmp(argv[1], "limits")) {
        printf("%d %d\n", kPvsMaxSlotCap, kPvsBadTable);
    } else if (!strcmp(argv[1], "uniform")) {           // B n_lig n_rec
        dump(PvsUniformSlots{atoi(argv[2]), atoi(argv[3]), atoi(argv[4])});
    } else {                                            // ragged[_cap] B L_cap n_rec cap status lig_ptr node_ptr slot_of
        std::vector<int32_t> v;
        for (int i = 2; i < argc; ++i) v.push_back((int32_t)atoi(argv[i]));
        const int B = v[0], L_cap = v[1];
        if ((int)v.size() != 5 + 2 * (B + 1) + L_cap) return 2;
        const int32_t status = v[4];
        const int32_t* lig_ptr = v.data() + 5;
        if (!strcmp(argv[1], "ragged"))                 // the seven members of before: slots of one word
            dump(PvsRaggedSlots{lig_ptr, lig_ptr + B + 1, lig_ptr + 2 * (B + 1), &status, B, L_cap, v[2]});
        else
            dump(PvsRaggedSlots{lig_ptr, lig_ptr + B + 1, lig_ptr + 2 * (B + 1), &status, B, L_cap, v[2], v[3]});
    }
    return 0;
}
'''


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    if CXX is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('screen_words')
    (d / 'main.cpp').write_text(PROGRAM)
    exe = d / 'screen_words_probe'
    out = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', str(CSRC), str(d / 'main.cpp'), '-o', str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]

    def run(*args):
        text = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, check=True).stdout
        return [tuple(int(t) if t.lstrip('-').isdigit() else t for t in line.split()) for line in text.splitlines()]
    return run


def test_limits(program):
    from pointvs_amd.screening import MAX_SCREEN_LIGAND_ATOMS
    from pointvs_amd.parquet_data import MAX_LIGAND_ATOMS
    assert program('limits') == [(MAX_SCREEN_LIGAND_ATOMS, 8)]
    assert MAX_SCREEN_LIGAND_ATOMS == MAX_LIGAND_ATOMS == 1024


@pytest.mark.parametrize('cap', CAPS)
def test_words_per_cap_and_the_place_of_every_atom(program, cap):
    got = program('cap', cap)
    assert got[0] == (-(-cap // 64),)
    assert got[1:] == [divmod(k, 64) for k in range(cap)]
    # one bit per atom, none shared, all inside the cap's words
    assert len({64 * w + b for w, b in got[1:]}) == cap and max(w for w, _ in got[1:]) == got[0][0] - 1


def _masks(n_words):
    """Masks of n_words words: no bit; every bit; a lone bit at position 0 and at position 63 of each word; each word
    all ones between all-zero words; both end bits of every word; seeded random words with all-zero words between."""
    ones = (1 << 64) - 1
    masks = [[0] * n_words, [ones] * n_words]
    for w in range(n_words):
        for bit in (0, 63):
            masks.append([(1 << bit) if k == w else 0 for k in range(n_words)])
        masks.append([ones if k == w else 0 for k in range(n_words)])
    masks.append([(1 << 63) | 1] * n_words)
    rng = random.Random(64 * n_words)
    masks.append([rng.getrandbits(64) if k % 2 == 0 else 0 for k in range(n_words)])
    masks.append([rng.getrandbits(64) if k % 2 == 1 else ones for k in range(n_words)])
    return masks


@pytest.mark.parametrize('n_words', sorted({-(-cap // 64) for cap in CAPS}))
def test_rank_of_every_set_bit(program, n_words):
    for mask in _masks(n_words):
        whole = sum(word << (64 * w) for w, word in enumerate(mask))
        want = [(p // 64, p % 64, bin(whole & ((1 << p) - 1)).count('1')) for p in range(64 * n_words) if (whole >> p) & 1]
        assert [rank for _, _, rank in want] == list(range(len(want)))       # ascending by column, dense
        assert program('rank', *(f'{word:x}' for word in mask)) == want, [f'{word:x}' for word in mask]


def _tables(sizes, n_rec):
    lig_ptr = [0]
    for n in sizes:
        lig_ptr.append(lig_ptr[-1] + n)
    node_ptr = [a + p * n_rec for p, a in enumerate(lig_ptr)]
    slot_of = [p for p, n in enumerate(sizes) for _ in range(n)]
    return lig_ptr, node_ptr, slot_of


def _walk(sizes, n_rec, l_cap):
    """What the ragged layout says about every packed atom and every row, from a walk over the slots."""
    lig_ptr, node_ptr, _ = _tables(sizes, n_rec)
    want = []
    for p, n in enumerate(sizes):
        want += [('a', lig_ptr[p] + k, 1, lig_ptr[p], n) for k in range(n)]
    want += [('a', q, 0, 0, 0) for q in range(lig_ptr[-1], l_cap)]
    for p, n in enumerate(sizes):
        want += [('r', node_ptr[p] + k, 1, p, lig_ptr[p], n, node_ptr[p], k) for k in range(n + n_rec)]
    want += [('r', g, 0, -1, 0, 0, 0, 0) for g in range(node_ptr[-1], l_cap + len(sizes) * n_rec)]
    return want


def _ragged_args(kind, sizes, n_rec, l_cap, cap, status=0):
    lig_ptr, node_ptr, slot_of = _tables(sizes, n_rec)
    return (kind, len(sizes), l_cap, n_rec, cap, status, *lig_ptr, *node_ptr, *slot_of, *([-1] * (l_cap - len(slot_of))))


@pytest.mark.parametrize('shape', [(2, 1, 64), (2, 64, 65), (6, 17, 130)])
def test_layouts_without_a_slot_cap_answer_as_before(program, shape):
    """PvsUniformSlots{B, n_lig, n_rec} and the seven-member PvsRaggedSlots: one word, and atom() / row() as the
    builders computed them when one word was all there was."""
    b, n_lig, n_rec = shape
    n = n_lig + n_rec
    want = [('a', q, 1, q // n_lig * n_lig, n_lig) for q in range(b * n_lig)]
    want += [('r', g, 1, g // n, g // n * n_lig, n_lig, g // n * n, g % n) for g in range(b * n)]
    assert program('uniform', b, n_lig, n_rec) == [('w', 1)] + want
    assert program(*_ragged_args('ragged', [n_lig] * b, n_rec, b * n_lig, 0)) == [('w', 1)] + want
    sizes = (64, 0, 1, 64)
    assert program(*_ragged_args('ragged', sizes, n_rec, 256, 0)) == [('w', 1)] + _walk(sizes, n_rec, 256)


@pytest.mark.parametrize('cap', CAPS)
def test_wide_slots_change_the_word_count_and_nothing_else(program, cap):
    sizes = (cap, 0, 1, max(cap - 1, 1))
    n_rec, l_cap = 3, 4 * cap
    words = -(-cap // 64)
    assert program(*_ragged_args('ragged_cap', sizes, n_rec, l_cap, cap)) == [('w', words)] + _walk(sizes, n_rec, l_cap)
    got = program('uniform', 2, cap, n_rec)
    assert got[0] == ('w', words)
    n = cap + n_rec
    assert got[1:] == ([('a', q, 1, q // cap * cap, cap) for q in range(2 * cap)] +
                       [('r', g, 1, g // n, g // n * cap, cap, g // n * n, g % n) for g in range(2 * n)])
