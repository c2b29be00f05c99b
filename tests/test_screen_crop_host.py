"""The cropped slot layout (csrc/screen_slots.h: PvsCroppedSlots, pvs_select64), compiled alone with the host compiler
(CPU): select, rank, kept and row() against numpy on the masks where the word arithmetic can go wrong, and the numpy
reference of the crop (tests/_crop_ref.py) pinned against scipy's cdist."""
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import _crop_ref as ref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'pointvs_amd' / 'csrc'
CXX = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')

# args: B L_cap n_rec status lig_ptr[B+1] node_ptr[B+1] slot_of[L_cap] keep[B*W] keep_rank[B*(W+1)]
# out: "k p j kept rank" per slot and atom; "s p k atom" per slot and receptor row; "a q valid a0 n_lig";
#      "r g valid slot a0 n_lig node0 local"; "n rows words rec_words"; "c p kept_count"
PROGRAM = r'''
#include "screen_slots.h"
#include <stdio.h>
#include <stdlib.h>
#include <vector>
int main(int argc, char** argv) {
    std::vector<unsigned long long> v;
    for (int i = 1; i < argc; ++i) v.push_back(strtoull(argv[i], nullptr, 10));
    const int B = (int)v[0], L_cap = (int)v[1], n_rec = (int)v[2], W = pvs_rec_words(n_rec);
    if ((int)v.size() != 4 + 2 * (B + 1) + L_cap + B * W + B * (W + 1)) return 2;
    const int32_t status = (int32_t)v[3];
    std::vector<int32_t> t;
    for (int i = 0; i < 2 * (B + 1) + L_cap; ++i) t.push_back((int32_t)(long long)v[4 + i]);
    const unsigned long long* keep = v.data() + 4 + 2 * (B + 1) + L_cap;
    std::vector<int32_t> rank;
    for (int i = 0; i < B * (W + 1); ++i) rank.push_back((int32_t)keep[B * W + i]);
    const PvsCroppedSlots L{t.data(), t.data() + B + 1, t.data() + 2 * (B + 1), &status, keep, rank.data(), B, L_cap,
                            n_rec};
    printf("n %d %d %d\n", L.rows(), L.words(), L.rec_words());
    for (int p = 0; p < B; ++p) {
        printf("c %d %d\n", p, L.kept_count(p));
        for (int j = 0; j < n_rec; ++j) printf("k %d %d %d %d\n", p, j, (int)L.kept(p, j), L.receptor_row(p, j));
        for (int k = 0; k < L.kept_count(p); ++k) printf("s %d %d %d\n", p, k, L.receptor(p, k));
    }
    for (int q = 0; q < L.atoms(); ++q) {
        const PvsSlotAtom a = L.atom(q);
        printf("a %d %d %d %d\n", q, (int)a.valid, a.a0, a.n_lig);
    }
    for (int g = 0; g < L.rows(); ++g) {
        const PvsSlotRow r = L.row(g);
        printf("r %d %d %d %d %d %d %d\n", g, (int)r.valid, r.slot, r.a0, r.n_lig, r.node0, r.local);
    }
    for (int n = 0; n < 64; ++n) {                    // pvs_select64 on its own: one bit, all bits, every other bit
        const unsigned long long odd = 0xAAAAAAAAAAAAAAAAull;
        printf("b %d %d %d %d\n", n, pvs_select64(1ull << n, 0), pvs_select64(~0ull, n), n < 32 ? pvs_select64(odd, n) : -1);
    }
    return 0;
}
'''


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    if CXX is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('screen_crop')
    (d / 'main.cpp').write_text(PROGRAM)
    exe = d / 'screen_crop_probe'
    out = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', str(CSRC), str(d / 'main.cpp'), '-o',
                          str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]

    def run(sizes, masks, l_cap, status=0):
        """The layout of slots with `sizes` ligand atoms and keep `masks` ([B, n_rec] bool), as the builder lays it out."""
        masks = np.asarray(masks, dtype=bool)
        b, n_rec = masks.shape
        lig_ptr = np.concatenate([[0], np.cumsum(sizes)])
        node_ptr = lig_ptr + np.concatenate([[0], np.cumsum(masks.sum(axis=1))])
        slot_of = [p for p, n in enumerate(sizes) for _ in range(n)]
        slot_of += [0] * (l_cap - len(slot_of))
        args = [b, l_cap, n_rec, status, *lig_ptr, *node_ptr, *slot_of]
        args += [int(w) for m in masks for w in ref.mask_words(m)]
        args += [int(r) for m in masks for r in ref.rank_table(m)]
        text = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, check=True).stdout
        out = {}
        for line in text.splitlines():
            out.setdefault(line[0], []).append(tuple(map(int, line.split()[1:])))
        return out, lig_ptr, node_ptr
    return run


def _masks(n_rec):
    """The masks of the issue's list on n_rec atoms: random ones, all, none, and kept counts 1, 63, 64, 65 placed at
    random and as runs that cross word borders."""
    rng = np.random.default_rng(n_rec)
    masks = [rng.random(n_rec) < p for p in (0.5, 0.1, 0.9)]
    masks += [np.ones(n_rec, dtype=bool), np.zeros(n_rec, dtype=bool)]
    for count in (1, 63, 64, 65):
        if count > n_rec:
            continue
        m = np.zeros(n_rec, dtype=bool)
        m[rng.choice(n_rec, count, replace=False)] = True
        masks.append(m)
        run = np.zeros(n_rec, dtype=bool)                  # a run that ends at the last atom
        run[n_rec - count:] = True
        masks.append(run)
    last = np.zeros(n_rec, dtype=bool)                     # only the last atom: the partial word's last valid bit
    last[-1] = True
    masks.append(last)
    return masks


@pytest.mark.parametrize('n_rec', [130, 64, 65, 1, 200])
def test_select_rank_and_rows_agree_with_numpy(program, n_rec):
    """n_rec = 130: three words with two bits in the last. Every mask is a slot of one batch, with ligand sizes that
    include 0, so that slots without any row (no ligand atom, nothing kept) stand between others."""
    masks = _masks(n_rec)
    sizes = [(3, 0, 1, 7, 0)[k % 5] for k in range(len(masks))]
    sizes[4] = 0                                           # the none-kept mask without ligand atoms: a slot of no rows
    l_cap = sum(sizes) + 5
    out, lig_ptr, node_ptr = program(sizes, masks, l_cap)
    n_words = (n_rec + 63) // 64
    assert out['n'] == [(l_cap + len(masks) * n_rec, 1, n_words)]
    assert out['c'] == [(p, int(m.sum())) for p, m in enumerate(masks)]
    want_k, want_s = [], []
    for p, m in enumerate(masks):
        before = np.concatenate([[0], np.cumsum(m)])[:-1]      # kept atoms before j: the rank (for a dropped atom too)
        want_k += [(p, j, int(m[j]), int(before[j])) for j in range(n_rec)]
        want_s += [(p, k, int(j)) for k, j in enumerate(np.flatnonzero(m))]
    assert out['k'] == want_k
    assert out.get('s', []) == want_s
    want_a = [(q, 1, int(lig_ptr[p]), n) for p, n in enumerate(sizes) for q in range(lig_ptr[p], lig_ptr[p + 1])]
    want_a += [(q, 0, 0, 0) for q in range(lig_ptr[-1], l_cap)]
    assert out['a'] == want_a
    want_r = []
    for p, (n, m) in enumerate(zip(sizes, masks)):
        want_r += [(node_ptr[p] + k, 1, p, lig_ptr[p], n, node_ptr[p], k) for k in range(n + int(m.sum()))]
    assert len(want_r) == node_ptr[-1]
    want_r += [(g, 0, -1, 0, 0, 0, 0) for g in range(node_ptr[-1], l_cap + len(masks) * n_rec)]
    assert out['r'] == want_r
    # select and rank are inverse on the kept atoms
    rank_of = {(p, j): r for p, j, kept, r in out['k'] if kept}
    assert all(rank_of[(p, j)] == k for p, k, j in out.get('s', []))
    # a table that the builder found bad: nothing is valid
    bad, _, _ = program(sizes, masks, l_cap, status=8)
    assert all(a[1:] == (0, 0, 0) for a in bad['a']) and all(r[1:] == (0, -1, 0, 0, 0, 0) for r in bad['r'])


def test_select_in_a_word(program):
    out, _, _ = program([1], [np.ones(64, dtype=bool)], 1)
    assert out['b'] == [(n, n, n, 2 * n + 1 if n < 32 else -1) for n in range(64)]


@pytest.mark.parametrize('radius', [2.5, 6.0, 10.0])
def test_numpy_reference_is_scipys_cdist_decision(radius):
    """keep_mask == (cdist(ligand, receptor) < R).any(0) on fp32 coordinates widened to fp64, with pairs placed at
    exactly R (not kept), just inside it, and on top of each other (kept)."""
    from scipy.spatial.distance import cdist
    rng = np.random.default_rng(int(radius * 10))
    rec = (rng.random((400, 3)) * 30).astype(np.float32)
    lig = (rng.random((9, 3)) * 6 + 12).astype(np.float32)
    rec[0] = lig[0]                                         # coincident: kept
    rec[1] = lig[1] + np.array([radius, 0, 0], dtype=np.float32)
    lig[2] = (4.0, 4.0, 4.0)
    rec[2] = (4.0 + radius, 4.0, 4.0)                       # exactly representable, exactly R away: not kept
    rec[3] = (4.0, 4.0 - radius + 0.25, 4.0)                # exactly R - 0.25 away: kept
    want = (cdist(lig.astype(np.float64), rec.astype(np.float64)) < radius).any(axis=0)
    got = ref.keep_mask(lig, rec, radius)
    assert np.array_equal(got, want)
    assert got[0] and got[3] and 0 < got.sum() < len(rec)
    far = rec + np.float32(1000.0)
    assert not ref.keep_mask(lig, far, radius).any() and not ref.keep_mask(lig[:0], rec, radius).any()
    assert not (cdist(lig[2:3].astype(np.float64), rec[2:3].astype(np.float64)) < radius).any()
    # the words, backwards and forwards, and the cropped complex
    assert np.array_equal(ref.words_mask(ref.mask_words(got), len(rec)), got)
    assert ref.rank_table(got)[-1] == got.sum()
    feats_l, feats_r = rng.random((9, 4)).astype(np.float32), rng.random((400, 4)).astype(np.float32)
    x, pos, kept = ref.cropped_complex(feats_l, lig, feats_r, rec, radius)
    assert np.array_equal(kept, np.flatnonzero(want))
    assert np.array_equal(pos, np.concatenate([lig, rec[want]])) and np.array_equal(x, np.concatenate([feats_l, feats_r[want]]))
