"""CPU: the surface of the mclmc sampler (nfmc_mclmc_steps_f32): its export and its state size, the
controller recurrence (tuning.MicrocanonicalAdaptation) against hand-computed updates, two properties of the fp64 step of
tests/mclmc_fp64.py, and the plumbing of create_sampler.  tests/test_gpu_mclmc.py runs the kernels."""
import ctypes as C
import math

import pytest
import torch

import mclmc_fp64 as M

LN2 = math.log(2.0)


def test_the_header_declares_the_symbol_once_and_the_table_names_it():
    """Header and table are held together in tests/test_host_abi.py; here, the library's export."""
    from nfmc_amd import hip
    assert 'nfmc_mclmc_steps_f32' in {s[0] for s in hip.SYMBOLS} and hasattr(hip.lib(), 'nfmc_mclmc_steps_f32')
    assert hip.NFMC_ABI_VERSION == 4 == hip.limits().abi_version


def test_the_state_words_mirror_the_header():
    """Word by word they are held against the header in tests/test_host_abi.py; here, what the library makes of them."""
    from nfmc_amd import hip
    assert hip.MCLMC_WORDS == hip.TUNE_WORDS   # StatShift finds the shift words where the mala / hmc state keeps them
    lib = hip.lib()
    assert lib.nfmc_mclmc_state_doubles(10, 3) == lib.nfmc_tune_state_doubles(10) + 3 * hip.MCLMC_ROW_WORDS
    assert lib.nfmc_mclmc_state_doubles(0, 3) == 0 and lib.nfmc_mclmc_state_doubles(10, -1) == 0


# ---- the controller, against updates computed by hand
def test_an_update_moves_log_eps_by_a_sixth_of_the_log_error_ratio():
    from nfmc_amd.tuning import MicrocanonicalAdaptation
    d, count = 4, 100.0
    c = MicrocanonicalAdaptation(0.5, 2.0, torch.ones(d), d, target=5e-4)
    V = 1e-3                                        # twice the target: eps shrinks by 2^(1/6)
    c.step(V * count * d, count, None)
    assert c.step_size == pytest.approx(0.5 * 2.0 ** (-1.0 / 6.0), rel=1e-14)
    assert c.decoherence_length == 2.0 and c.energy_variance == pytest.approx(V, rel=1e-14)
    assert c.history == [[0.5, 2.0, c.energy_variance, count, c.step_size, 2.0]]


@pytest.mark.parametrize('V,factor', [(5e-4 * 1e9, 0.5), (5e-4 * 1e-9, 2.0), (0.0, 2.0)])
def test_both_clamps(V, factor):
    from nfmc_amd.tuning import MicrocanonicalAdaptation
    c = MicrocanonicalAdaptation(0.3, 1.0, torch.ones(3), 3)
    c.step(V * 30.0, 10.0, None)
    assert c.step_size == pytest.approx(0.3 * factor, rel=1e-14)


@pytest.mark.parametrize('e2,count', [(1.0, 0.0), (math.inf, 5.0), (math.nan, 5.0)])
def test_an_update_without_finite_steps_halves_eps_and_moves_nothing_else(e2, count):
    from nfmc_amd.tuning import MicrocanonicalAdaptation
    s = torch.tensor([1.0, 2.0, 3.0])
    c = MicrocanonicalAdaptation(0.3, 1.5, s, 3, tune_inv_mass_diag=True)
    c.step(e2, count, torch.tensor([9.0, 9.0, 9.0], dtype=torch.float64))
    assert c.step_size == 0.15 and c.decoherence_length == 1.5 and torch.equal(c.inv_mass_diag, s)


def test_the_scales_and_the_length_follow_the_variance():
    from nfmc_amd.tuning import MicrocanonicalAdaptation
    d = 3
    s0, v = torch.tensor([1.0, 2.0, 4.0]), torch.tensor([4.0, 2.0, 1.0], dtype=torch.float64)
    c = MicrocanonicalAdaptation(0.3, 1.5, s0, d, imd_adjustment=0.25, decoherence_factor=2.0, tune_inv_mass_diag=True)
    c.step(5e-4 * 10 * d, 10.0, v)                  # V on target: eps stays
    s1 = torch.tensor([0.75 * 1 + 0.25 * 4, 0.75 * 2 + 0.25 * 2, 0.75 * 4 + 0.25 * 1])
    assert c.step_size == pytest.approx(0.3, rel=1e-14)
    assert torch.allclose(c.inv_mass_diag, s1, rtol=0, atol=1e-7)
    assert c.decoherence_length == pytest.approx(2.0 * math.sqrt(4 / 1.75 + 2 / 2.0 + 1 / 3.25), rel=1e-7)
    # the tuners off: with the scales held, L takes them as they are; with L held, nothing but eps moves
    c = MicrocanonicalAdaptation(0.3, 1.5, s0, d, tune_inv_mass_diag=False)
    c.step(5e-4 * 10 * d, 10.0, v)
    assert torch.equal(c.inv_mass_diag, s0) and c.decoherence_length == pytest.approx(math.sqrt(4 + 1 + 0.25), rel=1e-12)
    c = MicrocanonicalAdaptation(0.3, 1.5, s0, d, tune_decoherence_length=False, tune_step_size=False)
    c.step(1.0, 10.0, v)
    assert (c.step_size, c.decoherence_length) == (0.3, 1.5)


# ---- the fp64 step
def _gauss_inputs(n, d, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.randn(n, d, generator=g, dtype=torch.float64)
    return x0, M.initial_velocity(n, d, seed, 0)


def test_the_fp64_step_conserves_the_unit_velocity():
    x0, u0 = _gauss_inputs(32, 7, 3)
    assert torch.allclose(u0.norm(dim=1), torch.ones(32, dtype=torch.float64), atol=1e-14)
    imd = torch.linspace(0.5, 2.0, 7)
    _, us, _, ok = M.steps(M.quadratic(torch.linspace(0.3, 2.0, 7), 0.1), x0, u0, 0.4, 2.0, imd, 3, 0, 16)
    assert ok.all()
    assert torch.allclose(us.norm(dim=2), torch.ones(16, 32, dtype=torch.float64), atol=1e-13)


def test_the_fp64_energy_error_is_of_third_order_in_eps():
    """dE of one step on a standard Gaussian between eps and eps / 2: the root mean square falls by 2^3."""
    n, d = 4096, 16
    x0, u0 = _gauss_inputs(n, d, 5)
    target = M.quadratic(0.5, 0.0)
    rms = []
    for eps in (0.25, 0.125):
        de = M.steps(target, x0, u0, eps, 1e6, None, 5, 0, 1)[2]
        rms.append(float((de ** 2).mean().sqrt()))
    assert 6.0 <= rms[0] / rms[1] <= 10.0, rms


def test_a_zero_force_leaves_the_velocity_and_the_kinetic_energy_alone():
    u = M.initial_velocity(4, 5, 1, 0)
    un, dk = M.kick(u, torch.zeros(4, 5, dtype=torch.float64), torch.ones(1, 5, dtype=torch.float64), 0.3, 5)
    assert torch.equal(un, u) and torch.equal(dk, torch.zeros(4, dtype=torch.float64))


def test_the_package_step_is_the_reference_step():
    """samplers.mcmc.mclmc_kick (the torch path of targets with no closed form) against the restatement here, in fp64"""
    from nfmc_amd.samplers.mcmc import mclmc_kick
    x0, u0 = _gauss_inputs(16, 6, 9)
    sigma = torch.linspace(0.5, 1.5, 6, dtype=torch.float64)[None]
    a, b = mclmc_kick(u0, x0, sigma, 0.2, 6), M.kick(u0, x0, sigma, 0.2, 6)
    assert torch.allclose(a[0], b[0], atol=1e-14) and torch.allclose(a[1], b[1], atol=1e-13)


# ---- plumbing
def test_create_sampler_builds_an_mclmc_sampler_with_the_documented_defaults():
    from nfmc_amd import create_sampler
    from nfmc_amd.potentials import SumOfSquares
    from nfmc_amd.samplers.mcmc import MCLMC, MCLMCKernel, MCLMCParameters
    s = create_sampler(SumOfSquares((16,)), strategy='mclmc', flow=None, param_kwargs={'n_iterations': 7, 'tune_every': 4},
                       kernel_kwargs={'decoherence_length': 3.0})
    assert isinstance(s, MCLMC) and isinstance(s.kernel, MCLMCKernel) and isinstance(s.params, MCLMCParameters)
    assert s.kernel.step_size == pytest.approx(0.25 * 4.0) and s.kernel.decoherence_length == 3.0
    assert torch.equal(s.kernel.inv_mass_diag, torch.ones(16))
    p = MCLMCParameters()
    assert (p.tune_step_size, p.tune_decoherence_length, p.tune_inv_mass_diag) == (True, True, False)
    assert (p.imd_adjustment, p.energy_variance_target, p.decoherence_factor, p.tune_every) == (0.25, 5e-4, 1.0, 8)
    assert MCLMCKernel(event_size=9).decoherence_length == pytest.approx(3.0)
    assert 'log step' in repr(s.kernel)


def test_an_event_size_of_one_is_a_value_error():
    from nfmc_amd import create_sampler
    from nfmc_amd.potentials import SumOfSquares
    with pytest.raises(ValueError, match='at least 2'):
        create_sampler(SumOfSquares((1,)), strategy='mclmc', flow=None)


def test_mclmc_is_a_supported_strategy_and_the_others_stay_out():
    from nfmc_amd import create_sampler
    from nfmc_amd.potentials import SumOfSquares
    from nfmc_amd.util import get_supported_mcmc_samplers, get_supported_samplers
    assert 'mclmc' in get_supported_samplers() and 'mclmc' in get_supported_mcmc_samplers()
    for strategy in ('ess', 'jump_ess', 'tess', 'nuts'):
        with pytest.raises(ValueError, match='Unsupported sampling strategy'):
            create_sampler(SumOfSquares((4,)), strategy=strategy, flow=None)


def test_the_entry_point_refuses_with_the_codes_of_the_hmc_entry_point():
    """Every refusal is decided before the first launch, from host values alone: no device is needed to ask."""
    from nfmc_amd import hip

    def rc(**kw):
        a = hip.NfmcMclmcArgs()
        a.x, a.velocity, a.n, a.d, a.n_steps, a.step_size, a.decoherence_length = 4096, 8192, 8, 4, 2, 0.1, 2.0
        a.pot = hip.NfmcPotential(hip.POT_QUADRATIC, 0, None, None, 1.0, 0.0)
        a.rng = hip.make_rng(1, 0, 0)
        a.stats = hip.null_stats()
        a.samples = hip.dense_store(None)
        for k, v in kw.items():
            obj, name = a, k
            while '.' in name:
                head, name = name.split('.', 1)
                obj = getattr(obj, head)
            setattr(obj, name, v)
        return hip.lib().nfmc_mclmc_steps_f32(C.byref(a), None)

    assert hip.lib().nfmc_mclmc_steps_f32(None, None) == hip.EINVAL
    assert rc(x=None) == hip.EINVAL and rc(velocity=None) == hip.EINVAL
    assert rc(d=1) == hip.EINVAL and rc(d=0) == hip.EINVAL and rc(n=0) == hip.EINVAL and rc(n_steps=0) == hip.EINVAL
    assert rc(n_steps=hip.MAX_STEPS_PER_CALL + 1) == hip.ESHAPE and rc(d=1025) == hip.ESHAPE
    assert rc(step_size=0.0) == hip.EINVAL and rc(decoherence_length=0.0) == hip.EINVAL
    assert rc(**{'pot.kind': 99}) == hip.EUNSUPPORTED
    assert rc(x=4098) == hip.EALIGN and rc(velocity=8194) == hip.EALIGN
    assert rc(**{'rng.rounds': 7}) == hip.EUNSUPPORTED and rc(**{'rng.rounds': 3}) == hip.EINVAL
    assert rc(**{'samples.base': 4096, 'samples.stride': 0}) == hip.EINVAL
    assert rc(**{'stats.sum_x': 4096}) == hip.EINVAL                      # statistics without their other buffers
    assert rc(energy_sums=4096) == hip.EINVAL                             # the energy sums travel through the statistics
    assert rc(**{'tune.state': 4096}) == hip.EINVAL
    full = {'stats.sum_x': 4096, 'stats.sum_x2': 4096, 'stats.counters': 4096, 'stats.scratch': 4096}
    assert rc(**full, **{'stats.defer': 1, 'stats.scratch_bytes': 1 << 30}) == hip.EINVAL
    assert rc(**full, **{'stats.scratch_bytes': 8}) == hip.ESCRATCH
    assert rc(**full, **{'stats.scratch_bytes': 1 << 30, 'tune.state': 4096, 'tune.tune_inv_mass_diag': 1}) == hip.EINVAL


@pytest.mark.parametrize('entry', ['nfmc_mala_steps_f32', 'nfmc_hmc_steps_f32'])
def test_the_mala_and_hmc_entry_points_refuse_the_same_single_faults_with_the_same_codes(entry):
    """The faults of the test above that the mala and hmc structs can carry, one at a time: the three entry points share
    these checks, and a fault has one code whichever of them meets it."""
    from nfmc_amd import hip
    EINVAL, ESHAPE, EALIGN, EUNSUPPORTED, ESCRATCH = -1, -2, -3, -4, -5
    assert (hip.OK, hip.EINVAL, hip.ESHAPE, hip.EALIGN, hip.EUNSUPPORTED, hip.ESCRATCH) == (0, -1, -2, -3, -4, -5)
    hmc = entry == 'nfmc_hmc_steps_f32'
    fn = getattr(hip.lib(), entry)

    def rc(**kw):
        a = (hip.NfmcHmcArgs if hmc else hip.NfmcMalaArgs)()
        a.x, a.n, a.d, a.n_steps, a.step_size, a.adjust = 4096, 8, 4, 2, 0.1, 1
        if hmc:
            a.n_leapfrog = 3
        a.pot = hip.NfmcPotential(hip.POT_QUADRATIC, 0, None, None, 1.0, 0.0)
        a.rng = hip.make_rng(1, 0, 0)
        a.stats = hip.null_stats()
        a.samples = hip.dense_store(None)
        for k, v in kw.items():
            obj, name = a, k
            while '.' in name:
                head, name = name.split('.', 1)
                obj = getattr(obj, head)
            setattr(obj, name, v)
        return fn(C.byref(a), None)

    assert fn(None, None) == EINVAL and rc(x=None) == EINVAL
    assert rc(n=0) == EINVAL and rc(d=0) == EINVAL and rc(n_steps=0) == EINVAL
    assert rc(n_steps=513) == ESHAPE and rc(d=1025) == ESHAPE
    assert rc(step_size=0.0) == EINVAL
    assert rc(**{'pot.kind': 99}) == EUNSUPPORTED
    assert rc(x=4098) == EALIGN
    assert rc(**{'rng.rounds': 3}) == EINVAL
    assert rc(**{'samples.base': 4096, 'samples.stride': 0}) == EINVAL
    assert rc(**{'stats.sum_x': 4096}) == EINVAL                          # statistics without their other buffers
    full = {'stats.sum_x': 4096, 'stats.sum_x2': 4096, 'stats.counters': 4096, 'stats.scratch': 4096}
    assert rc(**full, **{'stats.scratch_bytes': 8}) == ESCRATCH
    assert rc(**{'tune.state': 4096}) == EINVAL                           # the controller rides on the statistics fold
    if hmc:
        assert rc(n_leapfrog=0) == EINVAL
