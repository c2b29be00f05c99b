"""Host-side dispatch of the edge kernels (csrc/edge_dispatch.h), compiled alone with the host compiler (CPU).

The header is the one place that decides which kernel family runs a layer, on what grid and as which edge-residual
kind. These tests compare it with the rules the launchers carried inline before they shared it, restated here in Python
from that source: the same (blocks, n_chunks) for every launcher's parameter set, the same family for every
(H, n_attr, direction, environment), the same residual kind for every flag combination. The last part checks the two
grid overrides (PVS_CHUNK_EDGES, PVS_EDGES_PER_WAVE: read at every call, reaching every launcher) and the grids they give
under the work partitions of tests/test_gpu_edge_partitions.py."""
import itertools
import os
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / 'pointvs_amd' / 'csrc'
CXX = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')

# The launchers' calls of pvs_edge_grid, restated (edge_mfma_fwd.hip, edge_bwd_f16.hip, edge_bwd_h64.hip,
# edge_bwd_wide.hip, edge_mfma.hip): name, waves (teams) per block, block cap, edges-per-wave floor, chunk size.
PROGRAM = r'''
#include "edge_dispatch.h"
#include <stdio.h>
#include <string.h>
struct Site { const char* name; int nw, cap; long long min_edges, chunk; };
int main(int argc, char** argv) {
    if (argc > 1 && !strcmp(argv[1], "grid")) {
        const Site sites[] = {
            {"fwd_256", 4, kPvsFwdMaxBlocks, pvs_edges_per_wave(), pvs_chunk_edges()},
            {"fwd_512", 8, kPvsFwdLargeMaxBlocks, pvs_edges_per_wave(), pvs_chunk_edges()},
            {"fwd_768", 12, kPvsFwdLargeMaxBlocks, pvs_edges_per_wave(), pvs_chunk_edges()},
            {"fwd_wide", 4, kPvsFwdLargeMaxBlocks, pvs_edges_per_wave(), pvs_chunk_edges()},
            {"bwd_f16", 8, kPvsBwdF16MaxBlocks, pvs_edges_per_wave(), pvs_chunk_edges(8192)},
            {"bwd_h64", 4, kPvsBwdH64MaxBlocks, pvs_edges_per_wave(), 4096},
            {"bwd_wide", 1, kPvsBwdWideMaxBlocks, 512, 4096},
            {"exact_wide", 1, kPvsBwdExactWideMaxBlocks, 512, 4096},
            {"exact_h32", 4, kPvsBwdExactMaxBlocks, pvs_edges_per_wave(), 4096},
            {"exact_h64", 1, kPvsBwdExactMaxBlocks, 512, 4096},
        };
        for (const Site& s : sites)
            for (int i = 2; i < argc; ++i) {
                const long long E = atoll(argv[i]);
                const PvsEdgeGrid g = pvs_edge_grid(E, s.nw, s.cap, s.min_edges, s.chunk);
                printf("%s %lld %d %d\n", s.name, E, g.blocks, g.n_chunks);
            }
        printf("cap bwd_f16 %d\ncap bwd_h64 %d\ncap bwd_wide %d\ncap exact_h32_h64 %d\ncap exact_wide %d\ncap generic %d\n",
               kPvsBwdF16MaxBlocks, kPvsBwdH64MaxBlocks, kPvsBwdWideMaxBlocks, kPvsBwdExactMaxBlocks,
               kPvsBwdExactWideMaxBlocks, kPvsBwdGenericMaxBlocks);
        printf("capacity %d\n", kPvsEdgeSlabCapacity);
    } else if (argc > 1 && !strcmp(argv[1], "launchers")) {
        // the calls as the launchers make them: every chunk size through pvs_chunk_edges(its default), the floor
        // through pvs_edges_per_wave() except in the team kernels
        const Site sites[] = {
            {"fwd_256", 4, kPvsFwdMaxBlocks, pvs_edges_per_wave(), pvs_chunk_edges()},
            {"fwd_512", 8, kPvsFwdLargeMaxBlocks, pvs_edges_per_wave(), pvs_chunk_edges()},
            {"fwd_768", 12, kPvsFwdLargeMaxBlocks, pvs_edges_per_wave(), pvs_chunk_edges()},
            {"fwd_wide", 4, kPvsFwdLargeMaxBlocks, pvs_edges_per_wave(), pvs_chunk_edges()},
            {"bwd_f16", 8, kPvsBwdF16MaxBlocks, pvs_edges_per_wave(), pvs_chunk_edges(8192)},
            {"bwd_h64", 4, kPvsBwdH64MaxBlocks, pvs_edges_per_wave(), pvs_chunk_edges(4096)},
            {"bwd_wide", 1, kPvsBwdWideMaxBlocks, 512, pvs_chunk_edges(4096)},
            {"exact_wide", 1, kPvsBwdExactWideMaxBlocks, 512, pvs_chunk_edges(4096)},
            {"exact_h32", 4, kPvsBwdExactMaxBlocks, pvs_edges_per_wave(), pvs_chunk_edges(4096)},
            {"exact_h64", 1, kPvsBwdExactMaxBlocks, 512, pvs_chunk_edges(4096)},
        };
        for (const Site& s : sites)
            for (int i = 2; i < argc; ++i) {
                const long long E = atoll(argv[i]);
                const PvsEdgeGrid g = pvs_edge_grid(E, s.nw, s.cap, s.min_edges, s.chunk);
                printf("%s %lld %d %d\n", s.name, E, g.blocks, g.n_chunks);
            }
    } else if (argc > 1 && !strcmp(argv[1], "reread")) {
        // both overrides inside ONE process: set, set to values that count as unset, removed
        const char* steps[] = {nullptr, "16", "0", "-3", "48", nullptr};
        const char* vars[] = {"PVS_CHUNK_EDGES", "PVS_EDGES_PER_WAVE"};
        for (int i = 0; i < 6; ++i) {
            for (const char* name : vars) {
                if (steps[i]) setenv(name, steps[i], 1); else unsetenv(name);
            }
            printf("%s %lld %lld %d\n", steps[i] ? steps[i] : "unset", pvs_chunk_edges(), pvs_chunk_edges(8192),
                   pvs_edges_per_wave());
        }
    } else if (argc > 1 && !strcmp(argv[1], "family")) {
        static const char* names[] = {"generic", "split", "exact", "wide"};
        const int Hs[] = {16, 32, 48, 64, 128};
        for (int H : Hs)
            for (int A = 0; A <= 8; ++A)
                for (int dir = 0; dir < 2; ++dir)
                    printf("%d %d %s %s\n", H, A, dir ? "bwd" : "fwd",
                           names[pvs_edge_family(H, 0u, A, dir ? PVS_EDGE_BWD : PVS_EDGE_FWD)]);
    } else {
        const uint32_t bits[] = {0u, PVS_EDGE_RESIDUAL, PVS_REZERO, PVS_GATED_RESIDUAL, PVS_EDGE_ATTENTION};
        for (int m = 0; m < 32; ++m) {
            uint32_t f = 0;
            for (int b = 0; b < 5; ++b) if (m & (1 << b)) f |= bits[b];
            for (int has = 0; has < 2; ++has)
                printf("%d %d %d %d %d\n", (f & PVS_EDGE_RESIDUAL) != 0, (f & PVS_REZERO) != 0,
                       (f & PVS_GATED_RESIDUAL) != 0, has, (int)pvs_edge_residual_kind(f, has != 0));
        }
    }
    return 0;
}
'''

# name -> (waves or teams per block, block cap, edges-per-wave floor, chunk size) as the launchers had them inline
SITES = {
    'fwd_256': (4, 1024, 64, 4096),      # pick_grid(E, nw = kWaves, max_blocks = 1024)
    'fwd_512': (8, 256, 64, 4096),       # pick_grid(E, nw, nw >= 8 ? 256 : 1024), H = 64 with > 3 edge classes
    'fwd_768': (12, 256, 64, 4096),      # the same, <= 3 edge classes
    'fwd_wide': (4, 256, 64, 4096),      # pick_grid(E, kWaves, 256)
    'bwd_f16': (8, 256, 64, 8192),       # b > 256; pvs_chunk_edges(8192)
    'bwd_h64': (4, 256, 64, 4096),       # b > 256; literal 4096
    'bwd_wide': (1, 256, 512, 4096),     # (E + 511) / 512; b > 256 * per_cu with per_cu = 160 KB / 141,904 B = 1
    'exact_wide': (1, 256, 512, 4096),   # (E + 511) / 512; b > 256
    'exact_h32': (4, 512, 64, 4096),     # pvs_edge_bwd_mfma_max_blocks() = 512; literal 4096
    'exact_h64': (1, 512, 512, 4096),    # kTeams = 1; (E + 511) / 512; b > 512
}
PARENT_CAPS = {'bwd_f16': 256, 'bwd_h64': 256, 'bwd_wide': 256, 'exact_h32_h64': 512, 'exact_wide': 256, 'generic': 512}


def parent_grid(E, nw, cap, per, ce):
    """pick_grid and its six inline copies: fill the chip, cap the blocks, the same number of chunks per wave."""
    b = (E + nw * per - 1) // (nw * per)
    b = min(max(b, 1), cap)
    waves = b * nw
    per_wave = max((E + waves * ce - 1) // (waves * ce), 1)
    return b, waves * per_wave


def edge_counts():
    vals = {1, 63, 64, 65, 176_000, 10_189_512, 81_500_000, 2 ** 31 - 1}
    for nw, cap, per, _ in SITES.values():
        for centre in (nw * 64, nw * per, cap * nw * 64, cap * nw * per, cap * nw * 4096, cap * nw * 8192):
            vals.update((centre - 1, centre, centre + 1))
    return sorted(v for v in vals if 0 < v < 2 ** 31)


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    if CXX is None:
        pytest.skip('no host C++ compiler')
    d = tmp_path_factory.mktemp('edge_dispatch')
    (d / 'main.cpp').write_text(PROGRAM)
    exe = d / 'edge_dispatch_probe'
    out = subprocess.run([CXX, '-std=c++17', '-O1', '-Wall', '-Werror', '-I', str(CSRC), str(d / 'main.cpp'), '-o', str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]

    def run(*args, env=None):
        clean = {k: v for k, v in os.environ.items() if not k.startswith('PVS_')}
        clean.update(env or {})
        return subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, check=True, env=clean).stdout
    return run


def test_grid_plan_matches_the_launchers_former_formulas(program):
    lines = program('grid', *edge_counts()).splitlines()
    seen = set()
    caps = {}
    capacity = None
    for line in lines:
        f = line.split()
        if f[0] == 'cap':
            caps[f[1]] = int(f[2])
        elif f[0] == 'capacity':
            capacity = int(f[1])
        else:
            name, E, blocks, n_chunks = f[0], int(f[1]), int(f[2]), int(f[3])
            assert (blocks, n_chunks) == parent_grid(E, *SITES[name]), (name, E)
            assert n_chunks % (blocks * SITES[name][0]) == 0      # every wave the same number of chunks
            seen.add((name, E))
    assert seen == set(itertools.product(SITES, edge_counts()))
    # one weight-gradient slab per backward workgroup: every family's cap fits the workspace's slab count, which is
    # what it was (512)
    assert caps == PARENT_CAPS and capacity == 512
    assert all(c <= capacity for c in caps.values())


def parent_family(H, A, direction, env):
    """pvs_use_mfma, pvs_edge_mfma_supported, pvs_edge_bwd_mfma_supported and the launchers' own getenv calls."""
    if env.get('PVS_EGNN_KERNELS', '')[:1] == 'g' or H not in (32, 64, 128):
        return 'generic'
    if direction == 'bwd' and A > 3:
        return 'generic'
    bf0 = env.get('PVS_EGNN_BF16X3', '')[:1] == '0'
    bf64_0 = env.get('PVS_EGNN_BF16X3_H64', '')[:1] == '0'
    if H == 128:       # forward: always the two-launch f16x2 form; backward: the fp32 team kernel with PVS_EGNN_BF16X3=0
        return 'exact' if direction == 'bwd' and bf0 else 'wide'
    f16x2 = not bf0 and (H == 32 or not bf64_0)
    return 'split' if f16x2 else 'exact'


@pytest.mark.parametrize('kernels', [None, 'generic', 'mfma'])
@pytest.mark.parametrize('bf', [None, '0', '1'])
@pytest.mark.parametrize('bf64', [None, '0', '1'])
def test_family_matches_the_former_selection(program, kernels, bf, bf64):
    env = {k: v for k, v in (('PVS_EGNN_KERNELS', kernels), ('PVS_EGNN_BF16X3', bf), ('PVS_EGNN_BF16X3_H64', bf64))
           if v is not None}
    rows = [line.split() for line in program('family', env=env).splitlines()]
    assert len(rows) == 5 * 9 * 2
    for H, A, direction, fam in rows:
        assert fam == parent_family(int(H), int(A), direction, env), (H, A, direction, env)


def test_residual_kind_orders_rezero_before_gated(program):
    rows = [tuple(map(int, line.split())) for line in program('residual').splitlines()]
    assert len(rows) == 64
    for eres, rezero, gated, has_m_prev, kind in rows:
        want = 0 if not (eres and has_m_prev) else 2 if rezero else 3 if gated else 1
        assert kind == want, (eres, rezero, gated, has_m_prev)


# ---- the work partitions of tests/test_gpu_edge_partitions.py ------------------------------------------------------------
def _site_lines(text):
    return [line for line in text.splitlines() if line.split()[0] in SITES]


def test_launchers_plan_as_before_when_nothing_is_set(program):
    """The calls as the launchers make them now (every chunk size through pvs_chunk_edges) give the grids of the
    SITES table when no override is set, and when one is set to a value that counts as unset."""
    want = _site_lines(program('grid', *edge_counts()))
    assert len(want) == len(SITES) * len(edge_counts())
    assert _site_lines(program('launchers', *edge_counts())) == want
    for value in ('0', '-7', ''):
        env = {'PVS_CHUNK_EDGES': value, 'PVS_EDGES_PER_WAVE': value}
        assert _site_lines(program('launchers', *edge_counts(), env=env)) == want, value


def test_overrides_are_read_at_every_call(program):
    rows = [line.split() for line in program('reread').splitlines()]
    assert rows == [['unset', '4096', '8192', '64'], ['16', '16', '16', '16'], ['0', '4096', '8192', '64'],
                    ['-3', '4096', '8192', '64'], ['48', '48', '48', '48'], ['unset', '4096', '8192', '64']]


def test_no_launcher_passes_a_literal_chunk_size():
    """PVS_CHUNK_EDGES reaches every MFMA edge launcher: no call of pvs_edge_grid ends in a literal."""
    import re
    calls = []
    for path in sorted(CSRC.glob('*.hip')):
        calls += re.findall(r'pvs_edge_grid\((?:[^()]|\([^()]*\))*\)', path.read_text())
    assert len(calls) == 8, calls        # forward 2 (its three block sizes share one), split 2, wide 1, exact 3
    for call in calls:
        assert not re.search(r',\s*\d+\s*\)$', call), call


@pytest.mark.parametrize('partition', ['many_chunks', 'one_block', 'fine'])
def test_partitions_of_the_gpu_tests_reach_every_site(program, partition):
    """(blocks, n_chunks) of every launch site under each partition of tests/_edge_partition_cases.py, at the edge
    count of its graphs: the overridden chunk size, the overridden floor where the site honours it and 512 for the
    team sites - and what keeps the GPU tests from being vacuous: two or more chunks per wave (team), a single
    workgroup, a grid at its cap."""
    from tests import _edge_partition_cases as epc
    E = epc.N_EDGES
    rows = [line.split() for line in _site_lines(program('launchers', E, env=epc.PARTITIONS[partition]))]
    assert [r[0] for r in rows] == list(SITES) == list(epc.SITES)
    for name, e, blocks, n_chunks in rows:
        blocks, n_chunks = int(blocks), int(n_chunks)
        nw, cap, floor, chunk = epc.site_parameters(name, partition)
        team = SITES[name][2] == 512
        assert team == (not epc.SITES[name][2]) and (nw, cap) == SITES[name][:2] and epc.SITES[name][3] == SITES[name][3]
        assert floor == (512 if team else int(epc.PARTITIONS[partition].get('PVS_EDGES_PER_WAVE', SITES[name][2])))
        assert int(e) == E and (blocks, n_chunks) == parent_grid(E, nw, cap, floor, chunk), name
        assert n_chunks % (blocks * nw) == 0 and blocks <= cap
        if partition in ('many_chunks', 'one_block'):
            assert n_chunks // (blocks * nw) >= 2, name
        if partition == 'one_block' and not team:
            assert blocks == 1, name
        # (the team sites keep 512 edges per team, so a floor of one edge never drives them to their cap)
        if partition == 'fine' and cap <= E // (nw * floor):
            assert blocks == cap, name
    if partition == 'fine':
        at_cap = {r[0] for r in rows if int(r[2]) == SITES[r[0]][1]}
        assert at_cap == {'fwd_512', 'fwd_768', 'fwd_wide', 'bwd_f16', 'bwd_h64', 'exact_h32'}
        assert dict((r[0], int(r[2])) for r in rows)['exact_h32'] == 512      # every slab of the workspace
