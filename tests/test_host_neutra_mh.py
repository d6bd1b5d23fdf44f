"""CPU: the surface of nfmc_neutra_mh_steps_f32 (NeuTra-MH on a fused kernel): its export, and the routing decision of
NeuTra.sample for an MH inner sampler, which is a function of the potential, the flow and the Philox rounds alone
(NeuTra._mh_on_kernel).  tests/test_gpu_neutra_mh.py runs the kernel."""
import os

import pytest
import torch

import neutra_mh_cases as cases
import target_harness as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_declares_the_symbol_once_and_the_table_names_it():
    """Header and table are held together in tests/test_host_abi.py; here, the library's export."""
    from nfmc_amd import hip
    assert 'nfmc_neutra_mh_steps_f32' in {s[0] for s in hip.SYMBOLS} and hasattr(hip.lib(), 'nfmc_neutra_mh_steps_f32')
    assert hip.NFMC_ABI_VERSION == 4 == hip.limits().abi_version


@pytest.mark.parametrize('case', cases.ROUTES, ids=lambda c: c.name)
def test_the_route_of_an_mh_inner_sampler(case):
    """The seven cases of the GPU file's tests 1 and 7: a closed-form potential on a narrow flow is fused, everything else
    keeps the split path.  No GPU: the decision reads the potential, the flow's shape and the rounds."""
    s = case.sampler(T=1)
    rounds = int(getattr(s, 'rng_rounds', 10) or 10)
    pot = s._closed_form()
    assert (pot is not None) == case.closed_form
    assert s._mh_on_kernel(pot, rounds) == case.fused


@pytest.mark.parametrize('kind', sorted(cases.OWN_KINDS))
def test_the_route_of_the_own_unit_kinds(kind):
    """Every one is a closed-form potential of the NeuTra family; the kernel takes those measured no slower there."""
    pot, _ref, z0, nh = cases.OWN_KINDS[kind]()
    d = z0.shape[1]
    s = cases.sampler(d, pot, H.flow_pair(d, 9, n_hidden=nh, init_seed=1000 + d)[0], 1)
    assert s._closed_form() is pot
    assert s._mh_on_kernel(pot, 10) == cases.ON_KERNEL[kind]
    s.mh_kernel_kinds = (type(pot),)                  # what tools/probe_neutra_mh.py does to time a kind on the kernel
    assert s._mh_on_kernel(pot, 10)


def test_the_kinds_kept_on_the_split_path():
    from nfmc_amd import potentials as P
    from nfmc_amd.samplers import neutra
    on_kernel = set(neutra.MH_KERNEL_KINDS)
    assert on_kernel == {P.QuadraticPotential, P.Funnel, P.FullRankGaussian, P.Rosenbrock, P.StochasticVolatility,
                         P.LatticePhi4, P.VaryingEffectsRegression, P.ParticleSystem, P.DiffusionBridge}
    for cls in (P.SparseLogisticRegression, P.ItemResponseTheory, P.LatentGaussianModel, P.LatentGMRF, P.GaussianMixture,
                P.BayesianLogisticRegression):
        assert not issubclass(cls, tuple(on_kernel)), cls


def test_the_rows_per_wave_rule_is_the_kernels():
    """cases.rows_per_wave restates neutra_rows_per_wave and tile_stride; the source text it restates is matched here, as
    tests/test_host_dlmc.py does, so that a change of the formula, or of the MH entry point's tile count, fails.  Its
    switches: 148 | 149 and 300 | 301 with the kernel's four tiles, 196 | 197 and 396 | 397 with three."""
    def src(name):
        with open(os.path.join(ROOT, 'nfmc_amd', 'csrc', name)) as fh:
            return ' '.join(fh.read().split())
    nk, fd, entry = src('neutra_kernels.hpp'), src('flow_device.hpp'), src('neutra_kernels.hip')
    assert ('for (int rpw = 64; rpw >= 16; rpw >>= 1) if ((size_t)tiles_of_d * rpw * tile_stride(d) * sizeof(float) '
            '<= 150 * 1024) return rpw;') in nk
    assert 'int s = (d + 3) & ~3; if (((s >> 2) & 1) == 0) s += 4; return s;' in fd
    mh = entry[entry.index('int nfmc_neutra_mh_steps_f32('):]
    assert 'const int rpw = neutra_rows_per_wave(d, 4);' in mh
    assert 'const size_t lds = (size_t)4 * rpw * tile_stride(d) * sizeof(float);' in mh
    assert 'const int grid = (int)(tiles < kMaxGrid ? tiles : kMaxGrid);' in mh
    assert cases.MH_TILES == 4 and cases.LDS_BUDGET == 150 * 1024
    r = cases.rows_per_wave
    assert [r(d) for d in (2, 148, 149, 300, 301, 512)] == [64, 64, 32, 32, 16, 16]
    assert [r(d, 3) for d in (196, 197, 396, 397, 512)] == [64, 32, 32, 16, 16]
