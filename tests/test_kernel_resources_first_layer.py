"""Register budget of the first-layer form of the H = 32 edge backward, from the compiler's own report (CPU).

k_edge_bwd_f16_nogx (csrc/edge_bwd_f16.hip) shares its text with the BASELINE kernel k_edge_bwd_f16<0, false> and must
stay within that kernel's own budget - 256 VGPRs, no AGPRs, at most 2 spilled VGPRs and 4 spilled SGPRs: the
two-waves-per-SIMD step of tests/test_kernel_resources.py. The bound is the shipped general kernel's, not a target. The
report parsing is that test's.
"""
from pathlib import Path

import pytest

from tests.test_kernel_resources import CASES, HIPCC, SGPR_SPILL_OK, _report

BASELINE = 'k_edge_bwd_f16ILi0ELb0E'
FIRST_LAYER = 'k_edge_bwd_f16_nogx'


@pytest.mark.skipif(not Path(HIPCC).exists(), reason='hipcc not installed')
def test_first_layer_backward_fits_the_baseline_kernels_budget():
    src, flags, _, max_v, max_a, max_spill = next(c for c in CASES if c[2] == BASELINE)
    assert (max_v, max_a, max_spill, SGPR_SPILL_OK[BASELINE]) == (256, 0, 2, 4)
    kernels = _report(src, flags)
    hits = [v for k, v in kernels.items() if FIRST_LAYER in k]
    assert len(hits) == 1, list(kernels)
    r = hits[0]
    print(FIRST_LAYER, r)
    assert r['VGPRs'] <= max_v and r['AGPRs'] <= max_a, r
    assert r['VGPRs Spill'] <= max_spill and r['SGPRs Spill'] <= SGPR_SPILL_OK[BASELINE], r
    # the general kernels are found by their names as before: the new kernel's name extends none of their fragments
    assert len([k for k in kernels if BASELINE in k]) == 1 and len([k for k in kernels if 'k_edge_bwd_f16I' in k]) == 8
