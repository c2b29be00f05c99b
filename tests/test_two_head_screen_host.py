"""Screening two-headed models, the host side (CPU): the two new exports, the best-pose relation
(csrc/pose_select.h, compiled alone with the host compiler), which heads a screen evaluates (_resolve_tasks), the
hits-line format and the names of the two predictions files."""
import itertools
import re
import shutil
import subprocess
import types
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'pointvs_amd' / 'csrc'
CXX = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
NEW_SYMBOLS = ('pvs_pool_heads_fwd', 'pvs_segment_argmax')


def test_new_symbols_are_declared_bound_and_exported():
    from pointvs_amd import _lib
    header = (ROOT / 'include' / 'pvs_egnn.h').read_text()
    declared = set(re.findall(r'\b(pvs_[a-z0-9_]+)\s*\(', header))
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and name in _lib._PROTOTYPES, name
        assert hasattr(_lib.lib(), name), name
    assert 'PvsHead' in header and 'PVS_HEAD_SOFTPLUS' in header
    assert _lib.MIN_VERSION >= 106 and _lib.lib().pvs_version() >= 106
    # the ctypes struct is the header's: two pointers, three int32, padded to the pointer's alignment
    assert [name for name, _ in _lib.PvsHead._fields_] == ['w', 'b', 'n_out', 'act', 'col']
    assert re.search(r'const float\* w;\s*const float\* b;\s*int32_t n_out;\s*int32_t act;[^\n]*\n\s*int32_t col;', header)
    import ctypes
    assert ctypes.sizeof(_lib.PvsHead) == 32


# Prints, for the candidate table below (value, row): every pairwise merge, and every triple merged both ways round.
PROGRAM = r'''
#include "pose_select.h"
#include <stdio.h>
#include <string.h>
#include <vector>
static unsigned bits(float v) { unsigned u; memcpy(&u, &v, 4); return u; }
static bool same(PvsPosePick a, PvsPosePick b) {
    if (a.index != b.index) return false;
    return a.index < 0 || bits(a.value) == bits(b.value);
}
int main() {
    const float inf = INFINITY, nan = NAN;
    std::vector<PvsPosePick> t = {{1.5f, 0}, {1.5f, 1}, {-2.f, 2}, {inf, 3}, {inf, 4}, {-inf, 5}, {-inf, 6}, {nan, 7},
                                  {-nan, 8}, {0.f, 9}, {-0.f, 10}, {0.f, 11}, {3.25f, 12}, {3.25f, 76}, {nan, -1},
                                  {7.f, -1}, {-1e-45f, 13}};
    const int n = (int)t.size();
    int bad = 0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const PvsPosePick ab = pvs_pose_merge(t[i], t[j]), ba = pvs_pose_merge(t[j], t[i]);
            if (!same(ab, ba)) { printf("not commutative %d %d\n", i, j); ++bad; }
            if (pvs_pose_better(t[i], t[j]) && pvs_pose_better(t[j], t[i])) { printf("both better %d %d\n", i, j); ++bad; }
            printf("m %d %d %d\n", i, j, ab.index);
            for (int k = 0; k < n; ++k) {
                const PvsPosePick l = pvs_pose_merge(ab, t[k]), r = pvs_pose_merge(t[i], pvs_pose_merge(t[j], t[k]));
                if (!same(l, r)) { printf("not associative %d %d %d\n", i, j, k); ++bad; }
            }
        }
    const PvsPosePick none = pvs_pose_none();
    printf("none %d %d\n", none.index, (int)(none.value != none.value));
    return bad ? 1 : 0;
}
'''
# the same table for the Python restatement: (value, row); row < 0 = no row
INF, NAN = float('inf'), float('nan')
TABLE = [(1.5, 0), (1.5, 1), (-2.0, 2), (INF, 3), (INF, 4), (-INF, 5), (-INF, 6), (NAN, 7), (NAN, 8), (0.0, 9),
         (-0.0, 10), (0.0, 11), (3.25, 12), (3.25, 76), (NAN, -1), (7.0, -1), (-1e-45, 13)]


def _usable(p):
    return p[1] >= 0 and p[0] == p[0]


def _winner(a, b):
    """The issue's rules restated: the larger value, equal values to the lower row, a NaN (or no row) never wins."""
    both = [p for p in (a, b) if _usable(p)]
    if not both:
        return -1
    return min(both, key=lambda p: (-p[0], p[1]))[1]


@pytest.fixture(scope='module')
def relation(tmp_path_factory):
    assert CXX is not None, 'the tie and NaN rules are checked with the host C++ compiler; none found'
    d = tmp_path_factory.mktemp('pose_select')
    (d / 'main.cpp').write_text(PROGRAM)
    exe = d / 'pose_select_probe'
    out = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', str(CSRC), str(d / 'main.cpp'), '-o', str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_relation_is_commutative_and_associative(relation):
    complaints = [line for line in relation.stdout.splitlines() if line.startswith(('not ', 'both '))]
    assert relation.returncode == 0 and not complaints, complaints[:10]
    assert 'none -1 1' in relation.stdout.splitlines()


def test_relation_follows_the_rules(relation):
    merged = {}
    for line in relation.stdout.splitlines():
        if line.startswith('m '):
            i, j, index = map(int, line.split()[1:])
            merged[i, j] = index
    assert len(merged) == len(TABLE) ** 2
    for i, j in itertools.product(range(len(TABLE)), repeat=2):
        assert merged[i, j] == _winner(TABLE[i], TABLE[j]), (TABLE[i], TABLE[j])
    assert merged[0, 1] == merged[1, 0] == 0                 # ties go to the lower row ...
    assert merged[12, 13] == 12 and merged[9, 10] == merged[10, 9] == 9 and merged[11, 10] == 10     # ... -0.0 and +0.0 are a tie
    assert merged[7, 5] == merged[5, 7] == 5                 # a NaN loses to -inf
    assert merged[5, 6] == 5 and merged[3, 12] == 3          # -inf and +inf are scores
    assert merged[7, 8] == merged[14, 15] == merged[7, 14] == -1             # nothing usable: none


def _stub(two_headed, model_task='classification'):
    stub = types.SimpleNamespace(model_task=model_task)
    if two_headed:
        stub.feats_linear_layers_pose = stub.feats_linear_layers_affinity = object()
    else:
        stub.feats_linear_layers = object()
    return stub


def test_resolve_tasks_every_legal_combination():
    from pointvs_amd.screening import _resolve_tasks
    for task in ('classification', 'regression', 'multi_regression'):
        assert _resolve_tasks(_stub(False, task), None) is None
    assert _resolve_tasks(_stub(True, 'classification'), None) == 'pose'
    assert _resolve_tasks(_stub(True, 'regression'), None) == 'affinity'
    assert _resolve_tasks(_stub(True, 'multi_regression'), None) == 'affinity'      # (as the model's forward decides)
    for model_task in ('classification', 'regression'):
        for tasks in ('pose', 'affinity', 'both'):
            stub = _stub(True, model_task)
            assert _resolve_tasks(stub, tasks) == tasks
            assert stub.model_task == model_task


def test_resolve_tasks_on_constructed_models(tmp_path):
    from pointvs_amd.egnn_multitask import MultitaskSatorrasEGNN
    from pointvs_amd.egnn_satorras import SartorrasEGNN
    from pointvs_amd.screening import _resolve_tasks
    kw = dict(dim_input=12, k=16, dim_output=3, num_layers=1, graphnorm=False, model_task='regression')
    two = MultitaskSatorrasEGNN(tmp_path / 'two', 1e-3, 0.0, silent=True, **kw)
    one = SartorrasEGNN(tmp_path / 'one', 1e-3, 0.0, silent=True, **kw)
    assert _resolve_tasks(two, None) == 'affinity' and _resolve_tasks(two, 'both') == 'both'
    assert _resolve_tasks(one, None) is None
    pose, affinity = two.feats_linear_layers_pose, two.feats_linear_layers_affinity
    assert two.task_heads('pose') == [pose] and two.task_heads('affinity') == [affinity]
    assert two.task_heads('both') == [pose, affinity]
    assert one.task_heads(None) == [one.feats_linear_layers]
    for model, tasks in ((two, None), (two, 'classification'), (one, 'pose')):
        with pytest.raises(ValueError, match='tasks='):
            model.task_heads(tasks)
    assert two.model_task == 'regression'


def test_resolve_tasks_refusals():
    from pointvs_amd.screening import _resolve_tasks
    for tasks in ('pose', 'affinity', 'both', 'classification'):
        with pytest.raises(ValueError, match='has one head'):
            _resolve_tasks(_stub(False), tasks)
    for tasks in ('classification', 'regression', 'Pose', '', ('pose', 'affinity'), 0):
        with pytest.raises(ValueError, match="one of 'pose', 'affinity', 'both' or None"):
            _resolve_tasks(_stub(True), tasks)


def test_hit_lines_for_one_two_and_four_columns():
    from pointvs_amd.predictions import format_hit_lines
    names = ['ligA', 'ligB', 'ligC']
    nan = float('nan')
    assert format_hit_lines([2, -1, 0], [[0.12345], [nan], [-1.0]], 'rec', names) == [
        '0.123 | rec ligA_pose2', '-1.000 | rec ligC_pose0']
    assert format_hit_lines([0, 11, -1], [[0.5, 6.25], [0.9996, 0.0], [nan, nan]], 'rec', names) == [
        '0.500 6.250 | rec ligA_pose0', '1.000 0.000 | rec ligB_pose11']
    assert format_hit_lines([1, 0, 3], [[0.25, 1, 2, 3], [0.75, 4, 5, 6.0004], [1, 7, 8, 9]], '1abc', names) == [
        '0.250 1.000 2.000 3.000 | 1abc ligA_pose1', '0.750 4.000 5.000 6.000 | 1abc ligB_pose0',
        '1.000 7.000 8.000 9.000 | 1abc ligC_pose3']
    assert format_hit_lines([], [], 'rec', []) == []


def test_predictions_file_names(tmp_path):
    from pointvs_amd.predictions import task_files
    path = tmp_path / 'out' / 'library.txt'
    assert task_files(path, 'both') == {'pose': tmp_path / 'out' / 'pose_library.txt',
                                        'affinity': tmp_path / 'out' / 'affinity_library.txt'}
    assert list(task_files(path, 'both')) == ['pose', 'affinity']
    for tasks in (None, 'pose', 'affinity'):
        assert task_files(str(path), tasks) == {tasks: path}
