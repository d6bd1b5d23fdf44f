"""CPU: which headers each translation unit of the library reaches (nfmc_amd/csrc, DESIGN.md "Header layout of the
potential kinds").  The closure is the one the build hashes (build._unit_headers), so what these tests assert is what an
edit to a header recompiles.  No compiler runs here."""
import os
import shutil

from nfmc_amd import build

# the own_units kinds (NFMC_FOR_OWN_UNIT_POT, pot_kinds.hpp) by the name of their header pot_<kind>.hpp and of their units
OWN_KINDS = ['fullrank', 'rosenbrock', 'sv', 'slr', 'phi4', 'irt', 'vfx', 'particles', 'lgm', 'gmrf', 'diffusion']
KIND_HEADERS = {'pot_%s.hpp' % k for k in OWN_KINDS}


def own_units(kind):
    return ['sampler_%s_mala.hip' % kind, 'sampler_%s_hmc.hip' % kind, 'flow_b_%s.hip' % kind, 'flow_b_%s_rqs.hip' % kind]


# the dispatching units and the units of kinds 0 to 3: the own-unit classes are forward declarations there
GENERAL_UNITS = ['sampler_kernels.hip', 'flow_b_kernels.hip', 'flow_b_lean.hip', 'flow_kernels.hip', 'imh_parallel.hip',
                 'imh_parallel_rqs.hip'] + ['sampler_%s_j%d.hip' % (a, j) for a in ('mala', 'hmc') for j in (0, 4, 8)]
# the VALU NeuTra kernels dispatch over every neutra_valu kind (adjusted_potential_grad_row)
NEUTRA_UNITS = ['neutra_kernels.hip', 'neutra_kernels_r16.hip', 'neutra_kernels_r32.hip', 'neutra_kernels_r64.hip',
                'dlmc_kernels.hip']
# fit and matrix-core units: kinds 0 and 1 only, through potential_value_grad_row (flow_device.hpp), or no potential
FIT_AND_MFMA_UNITS = ['fit_kernels.hip', 'fit_mfma.hip', 'fit_rqs.hip', 'fit_rows_h4.hip', 'fit_rows_h8.hip',
                      'fit_support.hip', 'flow_mfma.hip', 'mfma_wide.hip', 'neutra_mfma.hip', 'misc_kernels.hip']


def pot_headers(unit, **roots):
    """Base names of the pot_*.hpp a unit (or header) of csrc reaches."""
    return {os.path.basename(p) for p in build._unit_headers(unit, **roots) if os.path.basename(p).startswith('pot_')}


def test_the_table_names_every_unit():
    units = [u for k in OWN_KINDS for u in own_units(k)] + GENERAL_UNITS + NEUTRA_UNITS + FIT_AND_MFMA_UNITS
    assert len(units) == len(set(units))
    assert sorted(units) == sorted(build.sources())
    assert KIND_HEADERS <= set(os.listdir(build.CSRC))


def test_own_units_reach_their_kind_only():
    for kind in OWN_KINDS:
        for unit in own_units(kind):
            assert pot_headers(unit) & KIND_HEADERS == {'pot_%s.hpp' % kind}, unit
            # and beside it the host's view and the shared helpers: not the classes of kinds 0 to 3
            assert pot_headers(unit) - KIND_HEADERS == {'pot_kinds.hpp', 'pot_shared.hpp'}, unit


def test_general_units_reach_the_basic_kinds_at_most():
    for unit in GENERAL_UNITS:
        assert pot_headers(unit) <= {'pot_kinds.hpp', 'pot_shared.hpp', 'pot_basic.hpp'}, unit
        assert 'pot_kinds.hpp' in pot_headers(unit), unit


def test_neutra_units_reach_every_kind():
    for unit in NEUTRA_UNITS:
        assert pot_headers(unit) == KIND_HEADERS | {'pot_kinds.hpp', 'pot_shared.hpp'}, unit


def test_fit_and_matrix_core_units_reach_no_potential_header():
    for unit in FIT_AND_MFMA_UNITS:
        assert pot_headers(unit) == set(), unit


def test_the_shared_headers_reach_no_kind():
    assert pot_headers('pot_kinds.hpp') == set()
    assert pot_headers('pot_shared.hpp') == {'pot_kinds.hpp'}
    assert pot_headers('pot_basic.hpp') == {'pot_kinds.hpp', 'pot_shared.hpp'}
    assert {os.path.basename(p) for p in build._unit_headers('common.hpp')} == {'nfmc_hip.h'}


def test_an_edit_to_one_kinds_header_invalidates_nine_units(tmp_path):
    roots = {'csrc': str(tmp_path / 'csrc'), 'include': str(tmp_path / 'include')}
    os.makedirs(roots['csrc'])
    for f in os.listdir(build.CSRC):   # the sources only: not build/
        if f.endswith(('.hip', '.hpp')):
            shutil.copy(os.path.join(build.CSRC, f), roots['csrc'])
    shutil.copytree(build.INCLUDE, roots['include'])
    units = build.sources()
    before = {u: build._unit_digest(u, **roots) for u in units}
    with open(os.path.join(roots['csrc'], 'pot_diffusion.hpp'), 'a') as fh:
        fh.write('// edited\n')
    changed = [u for u in units if build._unit_digest(u, **roots) != before[u]]
    assert sorted(changed) == sorted(own_units('diffusion') + NEUTRA_UNITS)
    assert len(changed) == 9
