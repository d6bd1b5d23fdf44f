"""The register budget of the lean flow-MH forms (csrc/flow_b_lean.hip), read from the built library's kernel metadata
(tools/kernel_resources.py: resource counts of the code objects' notes, no instruction text).  No GPU.

A SIMD has 512 VGPRs per lane, allocated in granules of 8.  The jump of one part of a split run is to sit beside the
inner kernel's waves of the other part:

    budget = floor((512 - w * alloc_inner) / k)

with w the inner kernel's waves per SIMD for one part, alloc_inner its allocation and k >= 2 the jump waves wanted
beside them.

C3 (jump_mala, 65536 x 64, two parts): one part's mala_kernel<8, 8, ..., LEAN> launch is 1024 workgroups of 4 waves on
1024 SIMDs, w = 4, at 76 VGPRs = 80 allocated; k = 2 gives (512 - 320) / 2 = 96.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIMD_VGPRS = 512


@pytest.fixture(scope='module')
def kernels():
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    try:
        import kernel_resources
    finally:
        sys.path.pop(0)
    lib = os.path.join(ROOT, 'nfmc_amd', 'libnfmc_hip.so')
    assert os.path.exists(lib), 'build() leaves the library in the tree'
    return kernel_resources, kernel_resources.kernel_resources(lib)


def _one(res, fragment):
    hits = [k for k in res if fragment in k]
    assert len(hits) == 1, (fragment, hits)
    return res[hits[0]]


# mangled template arguments: <CPL, LPC, HP, QuadraticPot, FAST = true, DIAG = false, RR, NB = 0, WPE>
C3_LEAN = 'flow_mh_b_kernelILi8ELi8ELi4ENS_12QuadraticPotELb1ELb0ELi%dELi0ELi5EEE'
C3_RICH = 'flow_mh_b_kernelILi8ELi8ELi4ENS_12QuadraticPotELb1ELb0ELi10ELi0ELi1EEE'
C3_INNER = 'mala_kernelILi8ELi8ENS_12QuadraticPotELb1ELi0ELi10ELb1ELb0EEE'


def test_c3_lean_jump_fits_twice_beside_one_parts_mala_waves(kernels):
    kr, res = kernels
    inner = _one(res, C3_INNER)
    w, k = 4, 2
    budget = (SIMD_VGPRS - w * kr.alloc_vgprs(inner)) // k
    assert budget == 96                       # the figure the form was built for: the inner kernel still allocates 80
    lean = _one(res, C3_LEAN % 10)
    assert kr.alloc_vgprs(lean) <= budget
    assert lean['.private_segment_fixed_size'] == 0
    assert w * kr.alloc_vgprs(inner) + k * kr.alloc_vgprs(lean) <= SIMD_VGPRS
    # the kernel of a call without a part is not this one: it keeps its schedule, and only one of its waves fits
    rich = _one(res, C3_RICH)
    assert rich['.private_segment_fixed_size'] == 0
    assert (SIMD_VGPRS - w * kr.alloc_vgprs(inner)) // kr.alloc_vgprs(rich) == 1


def test_lean_forms_have_no_scratch_at_either_round_count(kernels):
    _kr, res = kernels
    for rounds in (10, 7):
        assert _one(res, C3_LEAN % rounds)['.private_segment_fixed_size'] == 0
