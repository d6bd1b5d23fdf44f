"""Stochastic volatility on the host: argument validation (one case per rule), the defaults, U and grad U of the torch
potential against the fp64 loop of tests/sv_fp64.py and the model's log densities, the descriptor and the header's kind
constant, the launch-family routing, the sampler factory and the constrain / unconstrain round trip (no GPU needed)."""
import math

import pytest
import torch

from sv_fp64 import SVU64, constrained_u64, simulate, start_states
from nfmc_amd import hip
from nfmc_amd.potentials import FAMILIES, Potential, StochasticVolatility, recognize
from nfmc_amd.samplers.common import resolve_target



def _u_and_grad(pot, x, dtype):
    t = x.to(dtype).detach().requires_grad_(True)
    u = pot(t)
    (g,) = torch.autograd.grad(u.sum(), t)
    return u.detach(), g


Y = [0.1, -0.3, 0.2]
BAD = [
    ('y scalar', dict(y=0.5), 'y'),
    ('y 2-D', dict(y=[[0.1, 0.2]]), 'y'),
    ('y empty', dict(y=[]), 'y'),
    ('y nan', dict(y=[0.1, float('nan')]), 'y'),
    ('y inf', dict(y=[float('inf')]), 'y'),
    ('y overflows fp32', dict(y=[1e39]), 'y'),
    ('mu_scale zero', dict(y=Y, mu_scale=0.0), 'mu_scale'),
    ('mu_scale negative', dict(y=Y, mu_scale=-1.0), 'mu_scale'),
    ('mu_scale inf', dict(y=Y, mu_scale=float('inf')), 'mu_scale'),
    ('mu_scale underflows fp32', dict(y=Y, mu_scale=1e-50), 'mu_scale'),
    ('mu_scale not a scalar', dict(y=Y, mu_scale=[1.0, 2.0]), 'mu_scale'),
    ('sigma_scale zero', dict(y=Y, sigma_scale=0.0), 'sigma_scale'),
    ('sigma_scale nan', dict(y=Y, sigma_scale=float('nan')), 'sigma_scale'),
    ('sigma_scale overflows fp32', dict(y=Y, sigma_scale=1e40), 'sigma_scale'),
    ('sigma_scale a bool', dict(y=Y, sigma_scale=True), 'sigma_scale'),
    ('alpha zero', dict(y=Y, phi_prior=(0.0, 1.0)), 'alpha'),
    ('alpha negative', dict(y=Y, phi_prior=(-2.0, 1.0)), 'alpha'),
    ('beta nan', dict(y=Y, phi_prior=(1.0, float('nan'))), 'beta'),
    ('beta overflows fp32', dict(y=Y, phi_prior=(1.0, 1e39)), 'beta'),
    ('phi_prior one value', dict(y=Y, phi_prior=(1.0,)), 'phi_prior'),
    ('phi_prior a scalar', dict(y=Y, phi_prior=2.0), 'phi_prior'),
]


@pytest.mark.parametrize('what,kw,name', BAD, ids=[b[0] for b in BAD])
def test_argument_validation(what, kw, name):
    with pytest.raises(ValueError, match=name):
        StochasticVolatility(**kw)


def test_defaults_and_accepted_edges():
    pot = StochasticVolatility(Y)
    assert (pot.mu_scale, pot.sigma_scale, pot.alpha, pot.beta) == (10.0, 5.0, 1.0, 1.0)
    assert pot.T == 3 and pot.event_shape == (6,) and pot.event_size == 6
    assert pot.y.dtype == torch.float64 and pot.y.tolist() == Y
    StochasticVolatility([0.0])
    StochasticVolatility(torch.tensor(Y, dtype=torch.float32), mu_scale=torch.tensor(2.0), sigma_scale=1,
                         phi_prior=[20.0, 1.5])
    assert StochasticVolatility(torch.zeros(1021)).event_shape == (1024,)


def _points(T, n, seed):
    """model-like states: a simulated series and chains jittered around its path, plus a few far ones"""
    y, x, _ = start_states(T, n, seed, spread=0.3)
    gen = torch.Generator().manual_seed(seed + 5)
    x[-4:, :3] += 2.0 * torch.randn(4, 3, generator=gen, dtype=torch.float64)   # mu, s, r far from the truth
    return y, x


@pytest.mark.parametrize('T', [1, 2, 3, 5, 17, 64, 250, 1021])
def test_u_and_grad_match_the_fp64_loop(T):
    y, x = _points(T, 24, T)
    kw = dict(mu_scale=3.0, sigma_scale=0.7, phi_prior=(20.0, 1.5))
    pot = StochasticVolatility(y, **kw)
    ref = SVU64(y, 3.0, 0.7, 20.0, 1.5)
    u64, g64 = ref(x), ref.grad(x)
    # the gradient formulas of the issue / header, term by term
    mu, s, r, h = x[:, 0], x[:, 1], x[:, 2], x[:, 3:]
    w, phi = torch.exp(-2 * s), torch.tanh(r)
    q = 1 - phi ** 2
    d0 = h[:, 0] - mu
    e = h[:, 1:] - mu[:, None] - phi[:, None] * (h[:, :-1] - mu[:, None])
    a = h[:, :-1] - mu[:, None]
    S1, S2, S3 = e.sum(1), (e * e).sum(1), (e * a).sum(1)
    sg = torch.sigmoid
    want = torch.empty_like(x)
    want[:, 0] = 2 * mu / (9.0 + mu ** 2) - q * w * d0 - (1 - phi) * w * S1
    want[:, 1] = 2 * sg(2 * (s - math.log(0.7))) - q * w * d0 ** 2 - w * S2 + (T - 1)
    want[:, 2] = 2 * 2.0 * sg(2 * r) - 2 * 20.5 * sg(-2 * r) - phi * q * w * d0 ** 2 - q * w * S3
    gh = 0.5 - 0.5 * torch.as_tensor(y) ** 2 * torch.exp(-h)
    gh[:, 0] += q * w * d0
    gh[:, 1:] += w[:, None] * e
    gh[:, :-1] -= (phi * w)[:, None] * e
    want[:, 3:] = gh
    torch.testing.assert_close(g64, want, rtol=1e-12, atol=1e-10)
    u, g = _u_and_grad(pot, x, torch.float64)
    torch.testing.assert_close(u, u64, rtol=1e-12, atol=1e-10)
    torch.testing.assert_close(g, g64, rtol=1e-12, atol=1e-10)
    u, g = _u_and_grad(pot, x, torch.float32)
    mag = ref(x).abs() + 0.5 * (x[:, 3:].abs() + torch.as_tensor(y) ** 2 * torch.exp(-x[:, 3:])).sum(1) + 1.0
    assert bool(((u.double() - u64).abs() <= 1e-6 * math.sqrt(T) * mag).all())
    gs = 1.0 + g64.abs().amax(1, keepdim=True)
    assert bool(((g.double() - g64).abs() <= 2e-5 * gs).all())


@pytest.mark.parametrize('T', [1, 2, 40])
def test_u_matches_the_model_log_densities_up_to_one_constant(T):
    y, x = _points(T, 16, 100 + T)
    x = x[:-4]   # the far (mu, s, r): log(1 - phi^2) of the naive densities loses digits as |phi| -> 1
    for kw in (dict(), dict(mu_scale=2.0, sigma_scale=0.3, phi_prior=(20.0, 1.5))):
        pot = StochasticVolatility(y, **kw)
        args = (kw.get('mu_scale', 10.0), kw.get('sigma_scale', 5.0)) + tuple(kw.get('phi_prior', (1.0, 1.0)))
        diff = pot(x) - constrained_u64(x, y, *args)
        assert float(diff.max() - diff.min()) < 1e-8 * (1 + float(pot(x).abs().max())), diff


def test_stable_where_the_naive_forms_overflow():
    """s, r and mu far out: the softplus / sigmoid forms stay finite in fp32 and their gradients too."""
    T = 6
    y, h = simulate(T, seed=3)
    pot = StochasticVolatility(y)
    x = torch.zeros(5, T + 3, dtype=torch.float64)
    x[:, 3:] = h
    x[0, 1] = 60.0             # e^{2s} overflows fp32
    x[1, 2] = 30.0             # 1 - phi^2 underflows
    x[2, 2] = -30.0
    x[3, 0] = 1e15             # (mu / c_mu)^2 fine, mu^2 fine in fp64 autograd
    x[4, 1], x[4, 2] = 40.0, 25.0
    u, g = _u_and_grad(pot, x[:3], torch.float32)
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(g).all())
    ref = SVU64(y)
    torch.testing.assert_close(u.double(), ref(x[:3]), rtol=1e-5, atol=1e-3)
    u, g = _u_and_grad(pot, x, torch.float64)
    assert bool(torch.isfinite(u).all()) and bool(torch.isfinite(g).all())
    torch.testing.assert_close(g, ref.grad(x), rtol=1e-10, atol=1e-10)


def test_descriptor_and_header_constant(monkeypatch):
    y = [0.5, -1.25, 2.0, 0.0]
    pot = StochasticVolatility(y, mu_scale=3.0, sigma_scale=0.5, phi_prior=(20.0, 1.5))
    monkeypatch.setattr(hip, 'ptr', lambda t, dtype=torch.float32: None if t is None else t.data_ptr())
    desc = pot.descriptor(torch.device('cpu'))
    assert desc.kind == 6 == hip.POT_STOCHASTIC_VOLATILITY
    assert desc.n_components == 4 == pot.event_size - 3            # the header's n_components: T
    assert desc.a_scalar == 3.0 and desc.b_scalar == 0.5
    y32, _, ab32 = pot._dev[('cpu', torch.float32)]
    assert desc.a == y32.data_ptr() and desc.b == ab32.data_ptr()
    assert y32.dtype == torch.float32 and y32.tolist() == y
    assert ab32.dtype == torch.float32 and ab32.tolist() == [20.0, 1.5]
    assert pot.descriptor(torch.device('cpu')).a == desc.a      # one copy per device


FUSED = {'mcmc': True, 'flow_mh': True, 'imh_parallel': False, 'neutra': True, 'dlmc_step': False, 'fit': False}


def test_routing_table():
    assert set(FUSED) == set(FAMILIES)
    pot = StochasticVolatility(Y)
    assert isinstance(pot, Potential)
    for fam, want in FUSED.items():
        assert pot.fused_in(fam) is want, fam
        assert resolve_target(pot, (6,), family=fam) is (pot if want else None)
    assert resolve_target(pot, (6,)) is pot
    with pytest.raises(ValueError):
        pot.fused_in('transport')


@pytest.mark.parametrize('T', [1, 4])
def test_recognize_never_infers_it(T):
    y, _ = simulate(T, seed=T)
    pot = StochasticVolatility(y)
    d = T + 3
    assert recognize(lambda x: pot(x), (d,)) is None
    assert resolve_target(lambda x: pot(x), (d,), fuse='never', family='mcmc') is None
    assert resolve_target(lambda x: pot(x), (d,), fuse='auto', family='mcmc') is None


@pytest.mark.parametrize('strategy', ['mala', 'hmc', 'mh', 'jump_mala', 'imh', 'neutra_hmc'])
def test_create_sampler_takes_the_event_shape_of_the_object(strategy):
    from nfmc_amd.sample import create_sampler
    pot = StochasticVolatility(torch.linspace(-1, 1, 9))
    s = create_sampler(pot, flow='realnvp' if strategy in ('jump_mala', 'imh', 'neutra_hmc') else None,
                       strategy=strategy)
    assert tuple(s.event_shape) == (12,)
    assert s.target is pot


def test_constrain_unconstrain_round_trip():
    T = 7
    y, x, _ = start_states(T, 11, 5, spread=0.5)
    pot = StochasticVolatility(y)
    mu, sigma, phi, h = pot.constrain(x)
    assert mu.shape == sigma.shape == phi.shape == (11,) and h.shape == (11, T)
    assert bool((sigma > 0).all()) and bool((phi.abs() < 1).all())
    torch.testing.assert_close(sigma, torch.exp(x[:, 1]))
    torch.testing.assert_close(phi, torch.tanh(x[:, 2]))
    torch.testing.assert_close(pot.unconstrain(mu, sigma, phi, h), x, rtol=1e-12, atol=1e-12)
    # leading dimensions (kept samples (steps, chains, d)) and broadcast scalars
    xs = x.reshape(1, 11, T + 3).expand(3, 11, T + 3)
    parts = pot.constrain(xs)
    assert parts[3].shape == (3, 11, T)
    torch.testing.assert_close(pot.unconstrain(*parts), xs, rtol=1e-12, atol=1e-12)
    one = pot.unconstrain(-1.0, 0.25, 0.95, torch.zeros(T))
    assert one.shape == (T + 3,)
    torch.testing.assert_close(one[:3], torch.tensor([-1.0, math.log(0.25), math.atanh(0.95)]), rtol=1e-6, atol=1e-6)
    with pytest.raises(ValueError):
        pot.unconstrain(0.0, -1.0, 0.5, torch.zeros(T))
    with pytest.raises(ValueError):
        pot.unconstrain(0.0, 1.0, 1.0, torch.zeros(T))
    with pytest.raises(ValueError):
        pot.unconstrain(0.0, 1.0, 0.5, torch.zeros(T + 1))
    with pytest.raises(ValueError):
        pot.constrain(torch.zeros(4, T + 2))


def test_simulator_is_seeded_and_stationary():
    y1, h1 = simulate(4000, seed=9)
    y2, h2 = simulate(4000, seed=9)
    assert torch.equal(y1, y2) and torch.equal(h1, h2)
    # the AR(1) path has the stationary mean mu and variance sigma^2 / (1 - phi^2) (loose: autocorrelated draws)
    assert abs(float(h1.mean()) + 1.0) < 0.2
    assert abs(float(h1.var()) / (0.0625 / (1 - 0.95 ** 2)) - 1.0) < 0.35


def test_hessian_diagonal_matches_autograd():
    T = 5
    y, x = _points(T, 6, 21)
    ref = SVU64(y, 3.0, 0.7, 20.0, 1.5)
    hd = ref.hess_diag(x)
    for i in range(x.shape[0]):
        H = torch.autograd.functional.hessian(lambda v: ref(v[None])[0], x[i])
        torch.testing.assert_close(hd[i], torch.diagonal(H), rtol=1e-10, atol=1e-10)
