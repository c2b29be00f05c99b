"""Which backward calls take the first-layer pair (csrc/edge_dispatch.h pvs_first_layer_bwd), on the host (CPU).

The header is compiled alone with the host compiler, as tests/test_edge_dispatch.py compiles it, and prints the decision
for every combination of hidden size {16, 32, 64}, class count {0, 3, 4}, the four edge-residual kinds, edge attention,
coordinate update (the flag and a live g_x_out), a caller that wants g_x, and the switch PVS_EGNN_FIRST_LAYER_BWD. Only
one cell of that table selects the pair: H = 32 in the split family with at most 3 classes, no edge residual, no edge
attention, coordinates updated with a live g_x_out, no g_x asked for, the switch not '0'.
"""
import itertools
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'pointvs_amd' / 'csrc'
CXX = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')

PROGRAM = r'''
#include "edge_dispatch.h"
#include <stdio.h>
int main() {
    const int Hs[] = {16, 32, 64}, As[] = {0, 3, 4};
    // none, sum, rezero, gated (pvs_edge_residual_kind): the kind needs the flag AND a previous message
    const uint32_t kinds[] = {0u, PVS_EDGE_RESIDUAL, PVS_EDGE_RESIDUAL | PVS_REZERO, PVS_EDGE_RESIDUAL | PVS_GATED_RESIDUAL};
    for (int H : Hs)
        for (int A : As)
            for (int kind = 0; kind < 4; ++kind)
                for (int att = 0; att < 2; ++att)
                    for (int upd = 0; upd < 2; ++upd)
                        for (int gxo = 0; gxo < 2; ++gxo)
                            for (int gx = 0; gx < 2; ++gx) {
                                const uint32_t f = kinds[kind] | (att ? PVS_EDGE_ATTENTION : 0u) | (upd ? PVS_UPDATE_COORDS : 0u);
                                printf("%d %d %d %d %d %d %d %d\n", H, A, kind, att, upd, gxo, gx,
                                       (int)pvs_first_layer_bwd(H, f, A, kind != 0, gxo != 0, gx != 0));
                            }
    // a residual flag without a previous message is no residual (kind 0)
    printf("nomprev %d\n", (int)pvs_first_layer_bwd(32, PVS_EDGE_RESIDUAL | PVS_UPDATE_COORDS, 3, false, true, false));
    // read at every call
    setenv("PVS_EGNN_FIRST_LAYER_BWD", "0", 1);
    printf("reread %d", (int)pvs_first_layer_bwd(32, PVS_UPDATE_COORDS, 3, false, true, false));
    unsetenv("PVS_EGNN_FIRST_LAYER_BWD");
    printf(" %d\n", (int)pvs_first_layer_bwd(32, PVS_UPDATE_COORDS, 3, false, true, false));
    return 0;
}
'''


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    if CXX is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('first_layer_bwd')
    (d / 'main.cpp').write_text(PROGRAM)
    exe = d / 'first_layer_bwd_probe'
    out = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', str(CSRC), str(d / 'main.cpp'), '-o', str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]

    def run(env=None):
        clean = {k: v for k, v in os.environ.items() if not k.startswith('PVS_')}
        clean.update(env or {})
        return subprocess.run([str(exe)], capture_output=True, text=True, check=True, env=clean).stdout
    return run


def _table(text):
    rows = [tuple(map(int, line.split())) for line in text.splitlines() if line[0].isdigit()]
    assert len(rows) == 3 * 3 * 4 * 2 * 2 * 2 * 2
    assert {r[:7] for r in rows} == set(itertools.product((16, 32, 64), (0, 3, 4), range(4), (0, 1), (0, 1), (0, 1), (0, 1)))
    return rows


@pytest.mark.parametrize('switch', [None, '1', '', 'on'])
def test_only_the_plain_h32_layer_without_g_x_takes_the_pair(program, switch):
    env = {} if switch is None else {'PVS_EGNN_FIRST_LAYER_BWD': switch}
    out = program(env)
    for H, A, kind, att, upd, gxo, gx, taken in _table(out):
        want = H == 32 and A <= 3 and kind == 0 and not att and upd and gxo and not gx
        assert bool(taken) == bool(want), (H, A, kind, att, upd, gxo, gx)
    assert 'nomprev 1' in out and 'reread 0 1' in out


def test_the_switch_turns_the_pair_off_everywhere(program):
    out = program({'PVS_EGNN_FIRST_LAYER_BWD': '0'})
    assert not any(r[7] for r in _table(out))
    assert 'nomprev 0' in out


@pytest.mark.parametrize('env', [{'PVS_EGNN_KERNELS': 'generic'}, {'PVS_EGNN_BF16X3': '0'}])
def test_other_kernel_families_never_take_the_pair(program, env):
    """The pair belongs to the split family: the generic and the exact kernels keep the general pair."""
    assert not any(r[7] for r in _table(program(env)))
