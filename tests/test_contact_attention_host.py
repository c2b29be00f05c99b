"""Contact attention, the host side (CPU): the two new exports and the library version, the numpy restatement of the
reduction (tests/_contact_ref.py) on three rows written out by hand, the order relation and the slot check of
csrc/contact_attention.h compiled alone with the host compiler, the layer index of `contact_attention=` and the
hotspot line format."""
import itertools
import re
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

from tests import _contact_ref as ref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'pointvs_amd' / 'csrc'
CXX = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
NAN = float('nan')


def test_exports_and_version():
    from pointvs_amd import _lib
    header = (ROOT / 'include' / 'pvs_egnn.h').read_text()
    declared = set(re.findall(r'\b(pvs_[a-z0-9_]+)\s*\(', header))
    for name, n_args in (('pvs_egnn_layer_fwd_partial_att', 16), ('pvs_contact_attention', 15)):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
        assert len(_lib._PROTOTYPES[name][1]) == n_args
    # the entry it extends: the same arguments less att_out
    assert len(_lib._PROTOTYPES['pvs_egnn_layer_fwd_partial'][1]) == 15
    assert _lib.MIN_VERSION >= 108 and _lib.lib().pvs_version() >= 108


def test_restatement_on_three_hand_written_rows():
    """One slot of one ligand atom and two receptor atoms. Row 0 (the ligand atom): class-1 edges interleaved with
    other classes and last, the largest value of the row on a class-0 edge -> 7. Row 1 (receptor atom 0): one NaN among
    its class-1 values -> 4. Row 2 (receptor atom 1): a class-1 edge with NaN only and a class-2 edge -> NaN, nothing
    accumulated."""
    rowptr = np.array([0, 5, 8, 10], dtype=np.int32)
    etype = np.array([0, 1, 2, 1, 1, 1, 1, 0, 1, 2], dtype=np.uint8)
    att = np.array([9, 3, 8, 7, 5, NAN, 4, 6, NAN, 2], dtype=np.float32)
    node_ptr, lig_ptr = np.array([0, 3], dtype=np.int32), np.array([0, 1], dtype=np.int32)
    lig_att, slot_rec, rec_sum, rec_count, rec_max = ref.contact_attention(
        rowptr, etype, att, node_ptr, lig_ptr, 2, *ref.fresh_accumulators(2), np.full(3, -7.0, dtype=np.float32))
    assert lig_att[0] == 7 and lig_att[1] == -7 and lig_att[2] == -7              # (rows beyond the ligand atoms stay)
    assert slot_rec[0, 0] == 4 and np.isnan(slot_rec[0, 1])
    assert rec_sum.tolist() == [4.0, 0.0] and rec_count.tolist() == [1, 0]
    assert rec_max[0] == 4 and np.isnan(rec_max[1])
    # a second call on the accumulators, with receptor atom 0's values raised: sum and count grow, the maximum too
    att2 = att.copy()
    att2[6] = 11
    _, slot_rec2, rec_sum2, rec_count2, rec_max2 = ref.contact_attention(
        rowptr, etype, att2, node_ptr, lig_ptr, 2, rec_sum, rec_count, rec_max, lig_att)
    assert slot_rec2[0, 0] == 11 and rec_sum2.tolist() == [15.0, 0.0] and rec_count2.tolist() == [2, 0]
    assert rec_max2[0] == 11 and np.isnan(rec_max2[1])
    assert rec_sum.tolist() == [4.0, 0.0]                                          # (the inputs are not written)
    # an empty slot in front: nothing from it
    out = ref.contact_attention(np.array([0, 0, 0, 5, 8, 10], dtype=np.int32), etype, att,
                                np.array([0, 2, 5], dtype=np.int32), np.array([0, 0, 1], dtype=np.int32), 2,
                                *ref.fresh_accumulators(2), np.full(1, -7.0, dtype=np.float32))
    assert out[0].tolist() == [7.0] and np.isnan(out[1][0]).all() and out[1][1, 0] == 4
    assert out[3].tolist() == [1, 0]
    assert np.signbit(ref.row_max(np.array([-0.0, -0.0], dtype=np.float32), [1, 1], 0, 2))
    assert not np.signbit(ref.row_max(np.array([-0.0, 0.0, -0.0], dtype=np.float32), [1, 1, 1], 0, 3))


# Folds the values given on the command line (nan, -0, numbers) with pvs_contact_max from NaN and prints the result's
# bits; "slot": prints the verdict on every slot of the tables n_slots n_rec n_nodes node_ptr.. lig_ptr..
PROGRAM = r'''
#include "contact_attention.h"
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "slot")) {
        const int n_slots = atoi(argv[2]), n_rec = atoi(argv[3]), n_nodes = atoi(argv[4]);
        std::vector<int32_t> node_ptr, lig_ptr;
        for (int i = 0; i <= n_slots; ++i) node_ptr.push_back(atoi(argv[5 + i]));
        for (int i = 0; i <= n_slots; ++i) lig_ptr.push_back(atoi(argv[6 + n_slots + i]));
        for (int p = 0; p < n_slots; ++p) {
            const PvsContactSlot s = pvs_contact_slot(node_ptr.data(), lig_ptr.data(), p, n_slots, n_rec, n_nodes);
            printf("%d %d %d\n", s.a0, s.n, s.node0);
        }
        return 0;
    }
    float cur = NAN;
    for (int i = 1; i < argc; ++i) cur = pvs_contact_max(cur, strcmp(argv[i], "nan") ? (float)atof(argv[i]) : NAN);
    uint32_t bits;
    memcpy(&bits, &cur, 4);
    printf("%08x\n", bits);
    return 0;
}
'''


@pytest.fixture(scope='module')
def probe(tmp_path_factory):
    assert CXX is not None, 'the order relation is checked with the host C++ compiler; none found'
    d = tmp_path_factory.mktemp('contact')
    (d / 'main.cpp').write_text(PROGRAM)
    exe = d / 'contact_probe'
    out = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', str(CSRC), str(d / 'main.cpp'), '-o', str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]

    def run(*args):
        res = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True)
        assert res.returncode == 0, res.stderr
        return res.stdout.splitlines()
    return run


def _bits(v):
    return '%08x' % np.array([v], dtype=np.float32).view(np.uint32)[0]


def test_the_maximum_does_not_depend_on_the_order(probe):
    for values, want in ((['nan', '-2', '7.5', '7.5'], 7.5), (['-0', '0', '-0'], 0.0), (['-0', '-0'], -0.0),
                         (['nan', '-inf', 'nan'], -np.inf), (['-1', '-0'], -0.0), (['1e-45', '0'], 1e-45)):
        got = {probe(*perm)[0] for perm in itertools.permutations(values)}
        assert got == {_bits(want)}, (values, got)
    assert probe('nan', 'nan')[0] == _bits(np.nan) and probe()[0] == _bits(np.nan)


def test_slot_verdicts(probe):
    # slots of 0, 2 and 1 ligand atoms, 3 receptor atoms, in 13 rows (one row of padding)
    node_ptr, lig_ptr = [0, 3, 8, 12], [0, 0, 2, 3]
    assert probe('slot', 3, 3, 13, *node_ptr, *lig_ptr) == ['0 0 0', '0 2 3', '2 1 8']
    assert probe('slot', 3, 3, 12, *node_ptr, *lig_ptr) == ['0 0 0', '0 2 3', '2 1 8']
    assert probe('slot', 3, 3, 11, *node_ptr, *lig_ptr)[2] == '0 -1 0'              # the last slot's rows do not fit
    assert probe('slot', 3, 3, 13, 0, 3, 9, 12, *lig_ptr)[1:] == ['0 -1 0', '0 -1 0']      # the tables disagree
    assert probe('slot', 3, 3, 13, *node_ptr, 0, 2, 0, 3)[:2] == ['0 -1 0', '0 -1 0']      # descending
    assert probe('slot', 1, 2, 2000, 0, 1027, 0, 1025) == ['0 -1 0']                # 1,025 ligand atoms
    assert probe('slot', 1, 2, 2000, 0, 1026, 0, 1024) == ['0 1024 0']


def test_layer_index_of_contact_attention():
    from pointvs_amd.screening import resolve_attention_layer
    embed = SimpleNamespace()
    model = SimpleNamespace(layers=[embed] + [SimpleNamespace(edge_attention=on) for on in (True, False, True)])
    assert resolve_attention_layer(model, None) is None
    assert resolve_attention_layer(model, 1) == 1 and resolve_attention_layer(model, 3) == 3
    assert resolve_attention_layer(model, -1) == 3 and resolve_attention_layer(model, -3) == 1
    for bad in (0, 2, -2, 4, -4, -5):
        with pytest.raises(ValueError, match=r'no edge attention \(the layers that have it: \[1, 3\], of 4\)'):
            resolve_attention_layer(model, bad)


def test_hotspot_line_format():
    from pointvs_amd.predictions import format_lines
    assert format_lines('hotspot', np.array([[0.25, 3.0], [1e-7, 1.0]]), None, ['rec', 'rec'], ['atom4', 'atom17']) == \
        ['0.250000 3 | rec atom4', '0.000000 1 | rec atom17']
