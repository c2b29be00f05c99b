"""Class-activation maps of hits, the host side (CPU): the two new exports and the library version, the numpy
restatement of the slot operator (tests/_cam_ref.py) pinned on hand-made numbers, the compiler's resource report of the
two new kernels, the LDS row stride of the per-node heads in the lane-group model, what `cam=` selects, and that the
inputs of the sweep test (tests/test_gpu_cam.py) discriminate - shown on the oracle alone."""
import importlib.util
import re
import shutil
import subprocess
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest
from torch import nn

from tests import _cam_ref as ref

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'pointvs_amd' / 'csrc'
CXX = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
NAN = float('nan')


def test_exports_and_version():
    from pointvs_amd import _lib
    header = (ROOT / 'include' / 'pvs_egnn.h').read_text()
    declared = set(re.findall(r'\b(pvs_[a-z0-9_]+)\s*\(', header))
    for name, n_args in (('pvs_node_heads_fwd', 8), ('pvs_slot_node_values', 15)):
        assert name in declared and name in _lib.EXPORTED_SYMBOLS and hasattr(_lib.lib(), name)
        assert len(_lib._PROTOTYPES[name][1]) == n_args
    assert _lib.MIN_VERSION >= 109 and _lib.lib().pvs_version() >= 109
    from pointvs_amd import functional as PF
    assert callable(PF.node_heads) and callable(PF.slot_node_values)


def test_restatement_on_hand_made_numbers():
    """Two slots of two receptor atoms: slot 0 has one ligand atom (rows 0 | 1, 2), slot 1 none (rows 3, 4); row 5 is
    padding. Row 0's three columns are (1e8, 1, -1e8): in the stated order (1e8 + 1) rounds to 1e8 and the mean is 0,
    in any other it is 1 / 3."""
    y = np.array([[1e8, 1, -1e8], [3, 6, 12], [NAN, 5, 7], [9, 9, 9], [8, 8, 8], [4, 4, 4]], dtype=np.float32)
    node_ptr, lig_ptr = np.array([0, 3, 5], dtype=np.int32), np.array([0, 1, 1], dtype=np.int32)
    start = ref.fresh_accumulators(2) + (np.full(2, -7.0, dtype=np.float32),)
    lig, slot, rec_sum, rec_count, rec_max = ref.slot_node_values(y, 1, 1, node_ptr, lig_ptr, 2, *start)
    assert lig.tolist() == [1.0, -7.0]                                   # (the entry past the ligand atoms stays)
    assert slot[0].tolist() == [6.0, 5.0] and np.isnan(slot[1]).all()     # the empty slot: NaN, nothing accumulated
    assert rec_sum.tolist() == [6.0, 5.0] and rec_count.tolist() == [1, 1] and rec_max.tolist() == [6.0, 5.0]
    lig3, slot3, sum3, count3, max3 = ref.slot_node_values(y, 0, 3, node_ptr, lig_ptr, 2, *start)
    assert lig3[0] == 0.0 and slot3[0, 0] == 7.0 and np.isnan(slot3[0, 1])      # a NaN column: a NaN value, skipped
    assert sum3.tolist() == [7.0, 0.0] and count3.tolist() == [1, 0] and max3[0] == 7.0 and np.isnan(max3[1])
    assert ref.node_value(np.array([[1, 1, 2]], dtype=np.float32), 0, 0, 3) == np.float32(np.float32(4.0) / np.float32(3.0))
    # a second call accumulates; the inputs are not written
    again = ref.slot_node_values(y, 1, 1, node_ptr, lig_ptr, 2, rec_sum, rec_count, rec_max, lig)
    assert again[2].tolist() == [12.0, 10.0] and again[3].tolist() == [2, 2] and rec_sum.tolist() == [6.0, 5.0]
    # a broken node_ptr entry spoils the two slots that share it, and only them
    y3 = np.concatenate([y[:5], y[:3], y[5:]])                            # a third slot like the first; padding last
    node3, lig_ptr3 = np.array([0, 3, 5, 8], dtype=np.int32), np.array([0, 1, 1, 2], dtype=np.int32)
    good = ref.slot_node_values(y3, 1, 1, node3, lig_ptr3, 2, *ref.fresh_accumulators(2), np.full(3, -7.0, dtype=np.float32))
    assert good[0].tolist() == [1.0, 1.0, -7.0] and good[3].tolist() == [2, 2]
    node3[1] = 4
    bad = ref.slot_node_values(y3, 1, 1, node3, lig_ptr3, 2, *ref.fresh_accumulators(2), np.full(3, -7.0, dtype=np.float32))
    assert bad[0].tolist() == [-7.0, 1.0, -7.0] and np.isnan(bad[1][:2]).all() and bad[3].tolist() == [1, 1]


KERNELS = (('node_heads.hip', 'k_node_heads_fwdILb1E'), ('node_heads.hip', 'k_node_heads_fwdILb0E'),
           ('contact_attention.hip', 'k_slot_node_values'), ('contact_attention.hip', 'k_contact_accumulate'))


@pytest.mark.parametrize('src', sorted({src for src, _ in KERNELS}))
def test_new_kernels_use_no_scratch_and_spill_nothing(src):
    """From the compiler's resource report, as tests/test_kernel_resources.py reads it."""
    from tests.test_kernel_resources import HIPCC, _report
    assert Path(HIPCC).exists(), 'the resource report needs hipcc'
    kernels = _report(src, [])
    for frag in (frag for s, frag in KERNELS if s == src):
        hits = [v for k, v in kernels.items() if frag in k]
        assert len(hits) == 1, (frag, list(kernels))
        r = hits[0]
        print(frag, r)
        assert r['ScratchSize [bytes/lane]'] == 0 and r['VGPRs Spill'] == 0 and r['SGPRs Spill'] == 0, (frag, r)
        # (four waves per SIMD: more never fit beside the LDS tiles - 18 KB a workgroup of two waves at width 32)
        assert r['VGPRs'] <= 128, (frag, r)


# Prints "width stride tile_rows" of csrc/node_heads.h for the widths on the command line (16-byte path where it applies).
PROGRAM = r'''
#include "node_heads.h"
#include <stdio.h>
#include <stdlib.h>
int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        const int w = atoi(argv[i]), s = pvs_node_heads_stride(w, w % 4 == 0);
        printf("%d %d %d\n", w, s, pvs_node_heads_tile_rows(s));
    }
    return 0;
}
'''


def test_row_stride_is_conflict_free_in_the_lane_group_model(tmp_path):
    """The stride the library uses (csrc/node_heads.h, compiled alone with the host compiler) against the bank rules in
    tools/lds_conflicts.py: no conflict cycle at any width, where the unpadded stride has them at 32, 64 and 128; width
    64 gets the issue's width + 4; the tile fits its LDS budget and never has more rows than the block has lanes."""
    assert CXX is not None, 'the stride is read from the header with the host C++ compiler; none found'
    (tmp_path / 'main.cpp').write_text(PROGRAM)
    exe = tmp_path / 'stride_probe'
    out = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', str(CSRC), str(tmp_path / 'main.cpp'), '-o', str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    widths = sorted(set(range(1, 130)) | {252, 256, 512, 1000, 1023, 1024})
    res = subprocess.run([str(exe)] + [str(w) for w in widths], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    table = {w: (s, r) for w, s, r in (map(int, line.split()) for line in res.stdout.splitlines())}
    assert table[64] == (68, 128) and table[32] == (36, 128) and table[20][0] == 20 and table[128] == (132, 64)
    spec = importlib.util.spec_from_file_location('lds_conflicts', ROOT / 'tools' / 'lds_conflicts.py')
    lds = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(lds)
    for w in widths:
        stride, rows = table[w]
        assert stride == lds.node_heads_stride(w) and stride >= w
        assert 1 <= rows <= 128 and rows & (rows - 1) == 0 and rows * stride * 4 <= 40960
        assert rows == 128 or 2 * rows * stride * 4 > 40960
        assert lds.node_heads(w, stride, rows, quiet=True)[1] == 0, (w, stride)
    for w in (32, 64, 128):
        assert lds.node_heads(w, w, quiet=True)[1] > 0


def test_what_cam_selects():
    from pointvs_amd.screening import resolve_cam
    one = SimpleNamespace(feats_linear_layers=nn.Sequential(nn.Linear(8, 1)))
    three = SimpleNamespace(feats_linear_layers=nn.Sequential(nn.Linear(8, 16), nn.SiLU(), nn.Linear(16, 3), nn.Softplus()))
    two = SimpleNamespace(feats_linear_layers=nn.Sequential(nn.Linear(8, 2)))
    assert resolve_cam(one, None, None, None) is None
    assert resolve_cam(one, None, None, True)[1:] == ([1], 0, 1)
    assert resolve_cam(three, None, None, True)[1:] == ([3], 0, 3)
    assert resolve_cam(three, None, None, 2)[1:] == ([3], 2, 1)
    pose, aff = nn.Sequential(nn.Linear(8, 1)), nn.Sequential(nn.Linear(8, 3), nn.ReLU())
    assert resolve_cam(None, [pose, aff], 'both', 1)[1:] == ([1, 3], 1, 1)
    assert resolve_cam(None, [aff], 'affinity', True)[1:] == ([3], 0, 3)
    with pytest.raises(ValueError, match='name a column'):
        resolve_cam(None, [pose, aff], 'both', True)
    with pytest.raises(ValueError, match='name a column'):
        resolve_cam(two, None, None, True)
    for bad in (3, -1):
        with pytest.raises(ValueError, match=r'column -?\d of 3 outputs'):
            resolve_cam(three, None, None, bad)
    for bad in (False, 1.0, 'pose'):
        with pytest.raises(ValueError, match='None, True or a column'):
            resolve_cam(one, None, None, bad)
    with pytest.raises(ValueError, match='no head'):
        resolve_cam(SimpleNamespace(feats_linear_layers=None), None, None, True)


def test_the_sweep_tests_inputs_discriminate_on_the_oracle_alone():
    """The hits of tests/test_gpu_contact_attention.py under the fp64 and the one-thread fp32 oracle: no atom pair within
    1e-4 of the radius; every receptor atom has a value in every hit; across the hits an atom's values spread, and its
    mean differs from its max, by more than 10 x the bound; and the mean of a hit's CAM values over its complex is the
    hit's score (the head is linear and the pooling a mean)."""
    from tests import _contact_ref
    y = ref.sweep_yardstick()
    a, bound = y['y64'], y['bound']
    gap = _contact_ref.radius_gap(y['items'], y['rec'], y['radius'])
    spread = a['per_hit'].max(0) - a['per_hit'].min(0)
    mean_max = float(np.abs(a['mean'] - a['max']).max())
    print(f"nearest pair to the radius {gap:.3e}; max|cam64| {y['scale']:.4f} noise32 {y['noise32']:.3e} bound "
          f"{bound:.3e}; largest spread across hits {float(spread.max()):.3f}; mean against max {mean_max:.3f}")
    assert gap > 1e-4
    assert y['noise32'] > 0 and bound < 1e-3 * y['scale']
    assert not np.isnan(a['per_hit']).any() and (a['count'] == len(y['items'])).all()
    assert float(spread.max()) > 10 * bound and mean_max > 10 * bound
    for name, _, pose in y['items']:
        values = np.concatenate([a['ligand'][name], a['per_hit'][[n for n, _, _ in y['items']].index(name)]])
        score = float(a['score'][name][0])
        print(f'{name}: mean CAM {values.mean():.15f} score {score:.15f}')
        assert abs(values.mean() - score) <= 1e-13 * max(1.0, abs(score)) * len(values)
    # the ligand atoms' values differ from one another too (a map that repeated one value would pass nothing here)
    assert float(np.ptp(a['ligand']['hitC'])) > 10 * bound
