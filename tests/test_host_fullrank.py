"""FullRankGaussian on the host: argument validation (one case per rule), covariance and precision inputs, U and grad U of
the torch potential against fp64 autograd of a restatement of its formula (tests/fullrank_fp64.py), the descriptor and
the header's kind constant, the launch-family routing and the sampler factory (no GPU needed)."""
import math

import pytest
import torch

from fullrank_fp64 import FullRankU64, spd
from nfmc_amd import hip
from nfmc_amd.potentials import FAMILIES, FullRankGaussian, Potential, recognize
from nfmc_amd.samplers.common import resolve_target



def _u_and_grad(pot, x, dtype):
    t = x.to(dtype).detach().requires_grad_(True)
    u = pot(t)
    (g,) = torch.autograd.grad(u.sum(), t)
    return u.detach(), g


BAD = [
    ('neither matrix', dict(mu=torch.zeros(3))),
    ('both matrices', dict(mu=torch.zeros(3), covariance=torch.eye(3), precision=torch.eye(3))),
    ('not square', dict(mu=torch.zeros(3), covariance=torch.ones(3, 2))),
    ('not 2-D', dict(mu=torch.zeros(3), precision=torch.ones(3))),
    ('empty', dict(mu=torch.zeros(0), precision=torch.zeros(0, 0))),
    ('not finite', dict(mu=torch.zeros(2), precision=torch.tensor([[1.0, float('nan')], [float('nan'), 1.0]]))),
    ('mu not finite', dict(mu=torch.tensor([0.0, float('inf')]), precision=torch.eye(2))),
    ('not symmetric', dict(mu=torch.zeros(2), covariance=torch.tensor([[2.0, 0.5], [0.4, 2.0]]))),
    ('not positive definite', dict(mu=torch.zeros(2), precision=torch.tensor([[1.0, 2.0], [2.0, 1.0]]))),
    ('singular', dict(mu=torch.zeros(2), covariance=torch.tensor([[1.0, 1.0], [1.0, 1.0]], dtype=torch.float64))),
    ('mu of the wrong length', dict(mu=torch.zeros(4), precision=torch.eye(3))),
    ('event_shape of the wrong size', dict(mu=torch.zeros(6), precision=torch.eye(6), event_shape=(2, 2))),
    ('precision overflows fp32', dict(mu=torch.zeros(2), precision=1e39 * torch.eye(2, dtype=torch.float64))),
    ('covariance too small for an fp32 precision', dict(mu=torch.zeros(2), covariance=1e-40 * torch.eye(2, dtype=torch.float64))),
]


@pytest.mark.parametrize('what,kw', BAD, ids=[b[0] for b in BAD])
def test_argument_validation(what, kw):
    with pytest.raises(ValueError):
        FullRankGaussian(**kw)


def test_symmetry_tolerance_and_symmetrisation():
    """An asymmetry of fp32 rounding (relative 1e-7) is accepted and averaged away; 1e-4 is refused."""
    lam = spd(5, 30.0, 1)
    noise = torch.randn(5, 5, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    pot = FullRankGaussian(torch.zeros(5), precision=lam + 1e-7 * float(lam.abs().max()) * noise)
    assert torch.equal(pot.precision, pot.precision.t())
    with pytest.raises(ValueError):
        FullRankGaussian(torch.zeros(5), precision=lam + 1e-4 * float(lam.abs().max()) * noise)


@pytest.mark.parametrize('d,cond', [(1, 1.0), (3, 10.0), (25, 1e3), (130, 1e3)])
def test_covariance_and_precision_are_the_same_target(d, cond):
    lam = spd(d, cond, d)
    cov = torch.linalg.inv(lam)
    cov = 0.5 * (cov + cov.t())
    mu = torch.randn(d, generator=torch.Generator().manual_seed(d), dtype=torch.float64)
    a = FullRankGaussian(mu, covariance=cov)
    b = FullRankGaussian(mu, precision=lam)
    # fp64 Cholesky inverse of a matrix of condition `cond`: relative error ~ cond * eps64
    torch.testing.assert_close(a.precision, b.precision, rtol=0, atol=1e-10 * cond * float(lam.abs().max()))
    x = torch.randn(16, d, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    torch.testing.assert_close(a(x), b(x), rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize('d,cond', [(1, 1.0), (3, 10.0), (8, 1e3), (64, 1e3), (256, 100.0)])
def test_u_and_grad_match_fp64_autograd(d, cond):
    lam = spd(d, cond, 3 * d)
    mu = torch.randn(d, generator=torch.Generator().manual_seed(d), dtype=torch.float64)
    pot = FullRankGaussian(mu, precision=lam)
    ref = FullRankU64(lam, mu)
    x = mu + torch.randn(32, d, generator=torch.Generator().manual_seed(d + 1), dtype=torch.float64)
    u64, g64 = ref(x), ref.grad(x)
    torch.testing.assert_close(g64, (x - mu) @ lam, rtol=1e-12, atol=1e-12)   # grad U = Lambda (x - mu)
    u, g = _u_and_grad(pot, x, torch.float64)                                 # fp64 input: the fp64 masters
    torch.testing.assert_close(u, u64, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(g, g64, rtol=1e-12, atol=1e-10)
    u, g = _u_and_grad(pot, x, torch.float32)                                 # fp32 on the CPU: the masters in fp32
    # fp32 sums of d terms of size |Lambda| |r|^2: relative 1e-6 sqrt(d) of the sum of magnitudes
    mag_u = 0.5 * torch.einsum('ni,ij,nj->n', (x - mu).abs(), lam.abs(), (x - mu).abs())
    assert bool(((u.double() - u64).abs() <= 1e-6 * math.sqrt(d) * mag_u + 1e-6).all())
    mag_g = (x - mu).abs() @ lam.abs()
    assert bool(((g.double() - g64).abs() <= 1e-6 * math.sqrt(d) * mag_g + 1e-6).all())


def test_two_dimensional_events_flatten_row_major():
    lam = spd(6, 20.0, 5)
    mu = torch.arange(6, dtype=torch.float64)
    pot = FullRankGaussian(mu.reshape(2, 3), precision=lam, event_shape=(2, 3))
    flat = FullRankGaussian(mu, precision=lam)
    assert pot.event_shape == (2, 3) and pot.event_size == 6 and flat.event_shape == (6,)
    x = torch.randn(5, 2, 3, dtype=torch.float64)
    torch.testing.assert_close(pot(x), flat(x.reshape(5, 6)), rtol=0, atol=0)
    assert FullRankGaussian(mu, precision=lam, event_shape=6).event_shape == (6,)


def test_descriptor_and_header_constant(monkeypatch):
    d = 9
    lam = spd(d, 50.0, 4)
    mu = torch.linspace(-1, 1, d, dtype=torch.float64)
    pot = FullRankGaussian(mu, covariance=torch.linalg.inv(lam))
    # host copies stand in for device memory: the descriptor's fields, not its pointers, are under test here
    monkeypatch.setattr(hip, 'ptr', lambda t, dtype=torch.float32: t.data_ptr())
    desc = pot.descriptor(torch.device('cpu'))
    assert desc.kind == 4 == hip.POT_GAUSSIAN_FULL
    assert desc.n_components == d                                   # the header's n_components: d
    assert desc.a_scalar == 0.0 and desc.b_scalar == 0.0
    lam32, mu32 = pot._dev['cpu']
    assert desc.a == lam32.data_ptr() and desc.b == mu32.data_ptr()
    assert lam32.dtype == torch.float32 and lam32.shape == (d, d) and lam32.is_contiguous()
    assert torch.equal(lam32, pot.precision.float()) and torch.equal(mu32, mu.float())
    assert pot.descriptor(torch.device('cpu')).a == desc.a      # one copy per device


FUSED = {'mcmc': True, 'flow_mh': True, 'imh_parallel': False, 'neutra': True, 'dlmc_step': False, 'fit': False}


def test_routing_table():
    assert set(FUSED) == set(FAMILIES)
    pot = FullRankGaussian(torch.zeros(3), precision=spd(3, 10.0, 1))
    assert isinstance(pot, Potential)
    for fam, want in FUSED.items():
        assert pot.fused_in(fam) is want, fam
        assert resolve_target(pot, (3,), family=fam) is (pot if want else None)
    assert resolve_target(pot, (3,)) is pot
    with pytest.raises(ValueError):
        pot.fused_in('transport')


def test_recognize_never_infers_a_full_rank_gaussian():
    """A dense quadratic is not of the diagonal form recognize() fits, so a plain callable stays on the split path."""
    lam = spd(4, 10.0, 6)
    pot = FullRankGaussian(torch.ones(4), precision=lam)
    dense = lambda x: 0.5 * torch.einsum('ni,ij,nj->n', x - 1, lam.to(x), x - 1)   # noqa: E731
    assert recognize(dense, (4,)) is None
    assert recognize(lambda x: pot(x), (4,)) is None
    assert resolve_target(dense, (4,), fuse='auto', family='mcmc') is None


@pytest.mark.parametrize('strategy', ['mala', 'hmc', 'mh', 'jump_mala', 'imh', 'neutra_hmc'])
def test_create_sampler_takes_the_event_shape_of_the_object(strategy):
    from nfmc_amd.sample import create_sampler
    pot = FullRankGaussian(torch.zeros(6), precision=spd(6, 10.0, 2), event_shape=(2, 3))
    s = create_sampler(pot, flow='realnvp' if strategy in ('jump_mala', 'imh', 'neutra_hmc') else None,
                       strategy=strategy)
    assert tuple(s.event_shape) == (2, 3)
    assert s.target is pot
