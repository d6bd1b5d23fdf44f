"""The fp64 warmup oracle (oracle/samplers.py: mcmc_warmup, replay_controller) against the reference's recorded warmups
and against the package's host-side controller; the warmup's argument checks.  No GPU."""
import math

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import potentials as opot
from oracle import samplers as osamp


def _params(fx, d, beta=None):
    return osamp.ControllerParams(step_size=float(fx['step_size0']), inv_mass_diag=torch.ones(d),
                                  imd_adjustment=1e-3 if beta is None else beta)


def test_oracle_warmup_reproduces_the_reference_tuning_fixture():
    fx = load_golden('tuning')
    n, d = fx['x0'].shape
    T = fx['exp/samples'].shape[0]
    noise = osamp.ReplayNoise(torch.from_numpy(fx['noise/normals']).double(), torch.from_numpy(fx['noise/uniforms']).double())
    tr, ups, _h, _m = osamp.mcmc_warmup(torch.from_numpy(fx['x0']).double(), opot.sum_squares, 'langevin', T,
                                       _params(fx, d), noise=noise)
    np.testing.assert_allclose(tr.stacked().numpy(), fx['exp/samples'], atol=3e-5, rtol=0)
    assert len(ups) == T and ups[-1].iteration == 10 + T
    np.testing.assert_allclose(ups[-1].step_size, float(fx['tuned_step_size']), rtol=1e-5)
    np.testing.assert_allclose(ups[-1].inv_mass_diag.numpy(), fx['tuned_inv_mass_diag'], atol=1e-6)
    assert (tr.n_accepted, tr.n_attempted) == tuple(int(v) for v in fx['exp/counters'][:2])


@pytest.mark.parametrize('name', ['warmup_mala_offset', 'warmup_mala_offset_imd05', 'warmup_hmc_offset',
                                  'warmup_hmc_offset_imd05'])
def test_oracle_warmup_reproduces_the_reference_offset_warmups(name):
    """MALA and HMC warmups on a diagonal Gaussian away from the origin, at the default EMA weight and at 0.5: the
    mass diagonal follows a variance about a non-zero mean."""
    fx = load_golden(name)
    n, d = fx['x0'].shape
    T = fx['exp/samples'].shape[0]
    mu, sig = torch.from_numpy(fx['mu']).double(), torch.from_numpy(fx['sigma']).double()
    target = opot.quadratic(0.5 / sig ** 2, mu)
    kind = 'langevin' if 'mala' in name else 'hmc'
    p = _params(fx, d, float(fx['imd_adjustment']))
    noise = osamp.ReplayNoise(torch.from_numpy(fx['noise/normals']).double(), torch.from_numpy(fx['noise/uniforms']).double())
    x0 = torch.from_numpy(fx['x0']).double()
    tr, ups, _h, _m = osamp.mcmc_warmup(x0, lambda x: target(x), kind, T, p, n_leapfrog=3, noise=noise)
    np.testing.assert_allclose(tr.stacked().numpy(), fx['exp/samples'], atol=1e-4, rtol=1e-5)
    assert ups[-1].iteration == int(fx['da_iteration']) == 10 + T
    np.testing.assert_allclose(ups[-1].step_size, float(fx['tuned_step_size']), rtol=1e-5)
    np.testing.assert_allclose(ups[-1].inv_mass_diag.numpy(), fx['tuned_inv_mass_diag'], rtol=1e-5, atol=1e-7)
    assert (tr.n_accepted, tr.n_attempted) == tuple(int(v) for v in fx['exp/counters'][:2])
    # the replay of the oracle's own states gives the same controller
    acc = [int(m.sum()) for m in tr.masks]
    ups2, _h2, _m2 = osamp.replay_controller(tr.stacked(), acc, 1, p)
    assert [u.step_size for u in ups2] == [u.step_size for u in ups]
    assert all(torch.equal(a.inv_mass_diag, b.inv_mass_diag) for a, b in zip(ups, ups2))


@pytest.mark.parametrize('every,T', [(1, 9), (3, 10), (4, 8)])
@pytest.mark.parametrize('beta', [1e-3, 0.5])
def test_replay_controller_equals_the_package_controller(every, T, beta):
    """replay_controller against nfmc_amd's MetropolisSampler.update_kernel + tuning.DualAveraging, fed the same
    states (CPU tensors).  For every > 1 the package's controller is fed the pooled states of each block."""
    from nfmc_amd.potentials import SumOfSquares
    from nfmc_amd.samplers import mcmc
    g = torch.Generator().manual_seed(3)
    n, d = 40, 6
    mu = torch.linspace(-20.0, 30.0, d)
    states = (mu + torch.rand(d, generator=g) * torch.randn(T, n, d, generator=g)).float()
    masks = torch.rand(T, n, generator=g) < 0.6
    s = mcmc.MALA((d,), SumOfSquares((d,)), mcmc.LangevinKernel(event_size=d, step_size=0.3),
                  mcmc.LangevinParameters(imd_adjustment=beta))
    p = osamp.ControllerParams(step_size=0.3, inv_mass_diag=torch.ones(d), imd_adjustment=beta)
    ups, h_t, imd_t = osamp.replay_controller(states, masks.sum(1), every, p)
    assert len(ups) == math.ceil(T / every) == len(osamp.pools(T, every))
    for u, (s0, k) in zip(ups, osamp.pools(T, every)):
        assert h_t[s0] == (0.3 if s0 == 0 else ups[s0 // every - 1].step_size)
        s.update_kernel({'x': states[s0:s0 + k].reshape(k * n, d), 'mask': masks[s0:s0 + k].reshape(-1)})
        np.testing.assert_allclose(s.kernel.step_size, u.step_size, rtol=1e-6)
        np.testing.assert_allclose(s.kernel.da.error_sum, u.error_sum, rtol=1e-6, atol=1e-7)
        assert s.kernel.da.iteration == u.iteration
        # torch.var in fp32 (the package's host controller) against two-pass fp64: a few fp32 ulps of the result
        np.testing.assert_allclose(s.kernel.inv_mass_diag.numpy(), u.inv_mass_diag.numpy(), rtol=4e-6)
        assert u.inv_mass_diag.dtype == torch.float32


def test_tune_every_above_one_call_is_refused():
    """tune_every > 512 (the transitions of one call) cannot be honoured: a ValueError, before anything launches."""
    from nfmc_amd.potentials import SumOfSquares
    from nfmc_amd.samplers import mcmc
    s = mcmc.MALA((3,), SumOfSquares((3,)), None, mcmc.LangevinParameters(n_warmup_iterations=10, tune_every=513))
    with pytest.raises(ValueError, match='tune_every'):
        s.warmup(torch.zeros(4, 3), show_progress=False)


def test_shadow_workload_takes_per_transition_step_and_mass():
    from oracle import shadow
    wl = shadow.Workload('mala', opot.sum_squares, step_size=[0.1, 0.2, 0.3], inv_mass_diag=torch.ones(3, 2) * 2,
                         step0=5)
    assert wl.h_at(6) == 0.2
    assert torch.equal(wl.imd_at(7, 2, torch.float64), torch.full((2,), 2.0, dtype=torch.float64))
    assert shadow.Workload('mh', opot.sum_squares).imd_at(0, 3, torch.float32).tolist() == [1.0, 1.0, 1.0]
