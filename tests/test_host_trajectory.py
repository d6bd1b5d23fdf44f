"""CPU: the host side of the trajectory-length adaptation (tuning.TrajectoryAdaptation, radical_inverse, leapfrog_count),
its refusals, the ABI of the trajectory block, and the fp64 reference of the behaviour tests (tests/chees_fp64.py)."""
import math
import types

import numpy as np
import pytest
import torch

import chees_fp64 as CH
from nfmc_amd.tuning import (TrajectoryAdaptation, TrajectoryAdaptationParams, leapfrog_count, radical_inverse)


def test_radical_inverse_known_answers():
    half = 2.0 ** -33                                     # the half-ulp offset of the 32-bit grid
    want = [1 / 2, 1 / 4, 3 / 4, 1 / 8, 5 / 8, 3 / 8, 7 / 8, 1 / 16, 9 / 16]
    assert [radical_inverse(k) for k in range(len(want))] == [w + half for w in want]
    assert radical_inverse(2 ** 32 - 1) == half           # k + 1 wraps to 0
    assert radical_inverse(2 ** 32 - 2) == (2 ** 32 - 1 + 0.5) * 2.0 ** -32 < 1.0
    assert radical_inverse((1 << 31) - 1) == 2.0 ** -32 + half   # k + 1 = 2^31: the lowest bit of the reversed word
    assert all(0.0 < radical_inverse(k) < 1.0 for k in (0, 1, 12345, 1 << 31, 2 ** 32 - 1))


def test_leapfrog_count_clamps_and_ceiling():
    # k = 0: u = 1/2 + 2^-33
    assert leapfrog_count(0, 1.0, 0.25) == 3              # ceil(2 + 2^-31) = 3: the offset keeps u T / h off the integer
    assert leapfrog_count(1, 1.0, 0.25) == 2              # u = 1/4 + 2^-33: ceil(1 + 2^-31)
    assert leapfrog_count(2 ** 32 - 1, 1.0, 0.25) == 1    # u = 2^-33: lower clamp (ceil gives 1 already)
    assert leapfrog_count(0, 1e-9, 0.25) == 1
    assert leapfrog_count(0, 1000.0, 0.25) == 128         # upper clamp at the default L_max
    assert leapfrog_count(0, 1000.0, 0.25, 7) == 7
    assert leapfrog_count(0, 1000.0, 0.25, 1) == 1
    # an exact ceiling boundary: u T / h = 3 exactly stays 3, the next fp64 above it gives 4
    u = radical_inverse(2)                                # 3/4 + 2^-33, exact in fp64
    h = 0.25
    T = 3.0 * h / u
    r = u * T / h
    assert leapfrog_count(2, T, h) == math.ceil(r)
    lo, hi = np.nextafter(T, 0.0), np.nextafter(T, 10.0)
    assert {leapfrog_count(2, float(t), h) for t in (lo, T, hi)} == {3, 4}


def test_trajectory_adaptation_three_updates_by_hand():
    p = TrajectoryAdaptationParams(learning_rate=1.0, beta2=0.95, clip=0.35)
    c = TrajectoryAdaptation(1.0, p, max_leapfrog_steps=128)
    assert c.value == 1.0 and c.averaged == 1.0 and c.count == 0
    # 1: g = 2.  v = 0.05 * 4 = 0.2, v-hat = 0.2 / 0.05 = 4, delta = 2 / (2 + 1e-8) -> clipped to 0.35
    c.step(2.0, 10.0, 0.1)
    assert c.count == 1 and c.v == pytest.approx(0.2, rel=1e-15)
    assert c.log_length == 0.35 and c.log_averaged == 0.35                 # w = 1
    # an update without weight, or with a g-hat that is not finite, leaves everything alone
    c.step(5.0, 0.0, 50.0)
    c.step(math.inf, 3.0, 50.0)
    c.step(math.nan, 3.0, 50.0)
    assert (c.count, c.log_length, c.log_averaged) == (1, 0.35, 0.35) and c.v == pytest.approx(0.2, rel=1e-15)
    # 2: g = -3, the step size jumped to 2.  v = 0.19 + 0.45 = 0.64, delta = -3 / sqrt(0.64 / 0.0975) -> -0.35,
    # log T = 0 < log 2: the lower clamp
    c.step(-3.0, 1.0, 2.0)
    assert c.count == 2 and c.v == pytest.approx(0.64, rel=1e-14)
    assert c.log_length == math.log(2.0)
    w = 2.0 ** -0.75
    assert c.log_averaged == pytest.approx(w * math.log(2.0) + (1 - w) * 0.35, rel=1e-15)
    bar2 = c.log_averaged
    # 3: g = 0.01 (no clip): v = 0.608 + 5e-6, delta = 0.01 / (sqrt(v / (1 - 0.95^3)) + 1e-8); h = 0.001: the upper clamp
    c.step(0.01, 1.0, 0.001)
    v3 = 0.95 * 0.64 + 0.05 * 1e-4
    assert c.v == pytest.approx(v3, rel=1e-14)
    delta = 0.01 / (math.sqrt(v3 / (1 - 0.95 ** 3)) + 1e-8)
    assert 0 < delta < 0.35 and math.log(2.0) + delta > math.log(0.128)
    assert c.log_length == math.log(128 * 0.001)
    w = 3.0 ** -0.75
    assert c.log_averaged == pytest.approx(w * math.log(0.128) + (1 - w) * bar2, rel=1e-15)
    assert c.value == math.exp(c.log_length) and c.averaged == math.exp(c.log_averaged)
    # unclipped, unclamped move
    c2 = TrajectoryAdaptation(2.0, TrajectoryAdaptationParams(), 128)
    c2.step(0.5, 1.0, 0.1)
    assert c2.log_length == pytest.approx(math.log(2.0) + 0.025 * 0.5 / (0.5 + 1e-8), rel=1e-15)


# ------------------------------------------------------------------------------------------------ refusals
def _hmc(cls_name='HMC', **params):
    from nfmc_amd.potentials import SumOfSquares
    from nfmc_amd.samplers import mcmc
    d = 4
    s = getattr(mcmc, cls_name)((d,), SumOfSquares((d,)), mcmc.HMCKernel(event_size=d, step_size=0.1),
                                mcmc.HMCParameters(n_iterations=3, n_warmup_iterations=3, **params))
    return s, SumOfSquares((d,))


def _run(world=1):
    shard = None if world == 1 else types.SimpleNamespace(world=world)
    return types.SimpleNamespace(shard=shard)


@pytest.mark.parametrize('how', ['adapt', 'frozen'])
def test_trajectory_refusals_name_their_reason(monkeypatch, how):
    from nfmc_amd import hip

    def make(cls='HMC'):
        s, pot = _hmc(cls, tune_trajectory_length=(how == 'adapt'))
        if how == 'adapt':
            s.params.tuning_mode()
        else:
            s.kernel.trajectory_length = 0.7
        return s, pot
    s, pot = make()
    assert s._trajectory_mode(_run(), pot) == (hip.TRAJECTORY_ADAPT if how == 'adapt' else hip.TRAJECTORY_FROZEN)
    s, pot = make('UHMC')
    with pytest.raises(ValueError, match='uhmc'):
        s._trajectory_mode(_run(), pot)
    s, pot = make()
    with pytest.raises(ValueError, match='split path'):
        s._trajectory_mode(_run(), None)
    with pytest.raises(ValueError, match='sharded'):
        s._trajectory_mode(_run(world=2), pot)
    monkeypatch.setenv('NFMC_TUNE_DEVICE', '0')
    with pytest.raises(ValueError, match='NFMC_TUNE_DEVICE=0'):
        s._trajectory_mode(_run(), pot)
    monkeypatch.delenv('NFMC_TUNE_DEVICE')
    s.rng_rounds = 7
    with pytest.raises(ValueError, match='rng_rounds=7'):
        s._trajectory_mode(_run(), pot)


def test_off_is_off_on_the_host():
    from nfmc_amd import hip
    s, pot = _hmc()
    assert s._trajectory_mode(_run(), pot) == hip.TRAJECTORY_OFF
    s.params.tuning_mode()
    assert s._trajectory_mode(_run(), None) == hip.TRAJECTORY_OFF       # nothing is refused with the option off
    assert 'leapfrogs: 20' in repr(s.kernel)
    s.kernel.trajectory_length = 1.5
    assert 'ignored' in repr(s.kernel) and '1.5' in repr(s.kernel)
    p = type(s.params)()
    assert p.tune_trajectory_length is False and p.max_leapfrog_steps == 128 and p.trajectory_adaptation is None


@pytest.mark.parametrize('strategy', ['jump_hmc', 'jump_uhmc', 'neutra_hmc'])
@pytest.mark.parametrize('field', ['tune_trajectory_length', 'trajectory_length'])
def test_inner_hmc_kernels_refuse_the_trajectory_fields(strategy, field):
    from nfmc_amd.potentials import SumOfSquares
    from nfmc_amd.sample import create_sampler
    d = 4
    kw = dict(inner_param_kwargs={'tune_trajectory_length': True}) if field == 'tune_trajectory_length' else \
        dict(inner_kernel_kwargs={'trajectory_length': 0.5})
    s = create_sampler(target=SumOfSquares((d,)), event_shape=(d,), strategy=strategy, **kw)
    x0 = torch.randn(8, d)
    for call in (s.warmup, s.sample):
        with pytest.raises(ValueError, match='fixed number of leapfrog steps'):
            call(x0, show_progress=False)


# ------------------------------------------------------------------------------------------------ ABI
def test_header_binding_and_library_agree():
    """Header against binding is tests/test_host_abi.py; here, the library's answers against the binding's words."""
    from nfmc_amd import hip
    lib = hip.lib()
    assert hip.limits().abi_version == 4
    assert lib.nfmc_tune_trajectory_doubles(0) == hip.TRAJ_WORDS == 16
    assert lib.nfmc_tune_trajectory_doubles(12) == hip.TRAJ_WORDS + 12 * hip.TRAJ_ROW_WORDS
    assert lib.nfmc_tune_trajectory_doubles(-1) == 0
    for d in (1, 3, 8, 25, 64, 130):                      # the tuning state in front of the block is what it was
        assert lib.nfmc_tune_state_doubles(d) == hip.TUNE_WORDS + 3 * hip.padded_d(d) + hip.STAT_TAIL


# ------------------------------------------------------------------------------------------------ the reference
def test_free_run_settles_and_follows_the_scales():
    """The fp64 reference the GPU behaviour test is held against: T-bar on N(0, I), d = 8 over 8 seeds stays within a
    factor 1.15 of the median, and the target with scales 1 .. 10 asks for more than 5 times that."""
    unit = np.array([CH.behaviour_reference('unit8', s) for s in range(8)])
    med = float(np.median(unit))
    print('T-bar unit8:', np.round(unit, 3))
    assert (unit < 1.15 * med).all() and (unit > med / 1.15).all(), unit
    lin = np.array([CH.behaviour_reference('lin16', s) for s in range(8)])
    print('T-bar lin16:', np.round(lin, 3))
    assert lin.min() > 5 * med, (lin, med)
