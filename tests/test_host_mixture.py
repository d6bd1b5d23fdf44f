"""GaussianMixture on the host: the torch potential against an fp64 restatement of its formula, its gradient, argument
validation, the descriptor block layout of include/nfmc_hip.h, and the launch-family routing (no GPU needed)."""
import math

import pytest
import torch

from nfmc_amd.potentials import (FAMILIES, DiagonalGaussian, Funnel, GaussianMixture, Potential, QuadraticPotential,
                                 SumOfSquares, recognize)
from nfmc_amd.samplers.common import resolve_target


def _params(K, d, scale_kind, seed):
    g = torch.Generator().manual_seed(seed)
    means = 3.0 * torch.randn(K, d, generator=g, dtype=torch.float64)
    if scale_kind == 'scalar':
        scales = 0.7
    elif scale_kind == 'K':
        scales = 0.3 + torch.rand(K, generator=g, dtype=torch.float64)
    else:
        scales = 0.3 + torch.rand(K, d, generator=g, dtype=torch.float64)
    weights = 0.1 + torch.rand(K, generator=g, dtype=torch.float64)   # uneven
    return means, scales, weights


def _u64(x, means, scales, weights):
    """U(x) = -log sum_k w_k prod_j N(x_j; mu_kj, sigma_kj) - d/2 log 2 pi (the class's constant), term by term in fp64
    (math.fsum), with log N = -log sigma - (x - mu)^2 / (2 sigma^2) - 1/2 log 2 pi."""
    K, d = means.shape
    s = torch.as_tensor(scales, dtype=torch.float64)
    s = s.expand(K, d) if s.dim() == 0 else (s[:, None].expand(K, d) if s.dim() == 1 else s)
    w = torch.as_tensor(weights, dtype=torch.float64)
    w = w / w.sum()
    out = []
    for row in x.reshape(x.shape[0], -1).double():
        logs = []
        for k in range(K):
            q = math.fsum(float((row[j] - means[k, j]) ** 2 / s[k, j] ** 2) for j in range(d))
            logs.append(math.log(float(w[k])) - math.fsum(math.log(float(s[k, j])) for j in range(d)) - 0.5 * q)
        m = max(logs)
        out.append(-(m + math.log(math.fsum(math.exp(v - m) for v in logs))))
    return torch.tensor(out, dtype=torch.float64)


def _grad64(x, means, scales, weights):
    K, d = means.shape
    s = torch.as_tensor(scales, dtype=torch.float64)
    s = s.expand(K, d) if s.dim() == 0 else (s[:, None].expand(K, d) if s.dim() == 1 else s)
    w = torch.as_tensor(weights, dtype=torch.float64)
    w = w / w.sum()
    lam = 1.0 / s ** 2
    xf = x.reshape(x.shape[0], -1).double()
    e = torch.log(w) + 0.5 * torch.log(lam).sum(1) - 0.5 * (lam * (xf[:, None] - means) ** 2).sum(-1)
    r = torch.softmax(e, dim=1)
    return (r[:, :, None] * lam * (xf[:, None] - means)).sum(1)


@pytest.mark.parametrize('K', [1, 3, 8])
@pytest.mark.parametrize('d', [1, 2, 7, 64])
@pytest.mark.parametrize('scale_kind', ['scalar', 'K', 'Kd'])
def test_call_matches_fp64_formula(K, d, scale_kind):
    means, scales, weights = _params(K, d, scale_kind, 100 * K + d)
    pot = GaussianMixture((d,), means, scales, weights)
    g = torch.Generator().manual_seed(7)
    near = means[torch.arange(6) % K] + torch.randn(6, d, generator=g, dtype=torch.float64)
    far = means.mean(0) + 1e3 * torch.sign(torch.randn(3, d, generator=g, dtype=torch.float64))   # 1e3 from every mode
    x = torch.cat([near, far])
    want = _u64(x, means, scales, weights)
    got = pot(x)
    assert got.dtype == torch.float64
    assert torch.allclose(got, want, rtol=1e-12, atol=1e-9)
    got32 = pot(x.float())
    assert got32.dtype == torch.float32 and torch.isfinite(got32).all()
    assert torch.allclose(got32.double(), got, rtol=2e-6, atol=1e-4)


@pytest.mark.parametrize('K,d,scale_kind', [(1, 2, 'scalar'), (3, 7, 'K'), (8, 64, 'Kd')])
def test_autograd_matches_closed_form_gradient(K, d, scale_kind):
    means, scales, weights = _params(K, d, scale_kind, 11 * K + d)
    pot = GaussianMixture(d, means, scales, weights)
    g = torch.Generator().manual_seed(3)
    x = torch.cat([means[torch.arange(5) % K] + 0.8 * torch.randn(5, d, generator=g, dtype=torch.float64),
                   1e3 + torch.zeros(1, d, dtype=torch.float64)]).requires_grad_(True)
    gr, = torch.autograd.grad(pot(x).sum(), x)
    want = _grad64(x.detach(), means, scales, weights)
    assert torch.isfinite(gr).all()
    assert torch.allclose(gr, want, rtol=1e-10, atol=1e-10)


def test_event_shape_and_mean_layouts():
    means = torch.randn(2, 3, 4, dtype=torch.float64)
    a = GaussianMixture((3, 4), means)
    b = GaussianMixture((3, 4), means.reshape(2, 12))
    x = torch.randn(5, 3, 4, dtype=torch.float64)
    assert torch.equal(a(x), b(x))
    assert a.event_size == 12 and a.n_components == 2


def test_far_points_are_finite_and_stable():
    pot = GaussianMixture(4, [[0.0] * 4, [5.0] * 4], scales=[0.1, 2.0], weights=[0.2, 0.8])
    x = torch.full((1, 4), 1e3, dtype=torch.float32)
    u = pot(x)
    assert torch.isfinite(u).all()
    xr = x.clone().requires_grad_(True)
    gr, = torch.autograd.grad(pot(xr).sum(), xr)
    assert torch.isfinite(gr).all()


@pytest.mark.parametrize('kw', [
    dict(means=torch.zeros(0, 3)),                                  # K = 0
    dict(means=torch.zeros(2, 4)),                                  # d mismatch
    dict(means=torch.zeros(2, 3), scales=torch.ones(3)),            # scales neither (K,) nor (K, d)
    dict(means=torch.zeros(2, 3), scales=torch.ones(2, 2)),
    dict(means=torch.zeros(2, 3), scales=0.0),                      # non-positive scale
    dict(means=torch.zeros(2, 3), scales=torch.tensor([1.0, -1.0])),
    dict(means=torch.zeros(2, 3), weights=[1.0]),                   # wrong number of weights
    dict(means=torch.zeros(2, 3), weights=[1.0, 0.0]),              # non-positive weight
    dict(means=torch.tensor([[0.0, float('nan'), 0.0], [0.0] * 3])),   # non-finite
    dict(means=torch.zeros(2, 3), scales=float('inf')),
    dict(means=torch.zeros(2, 3), weights=[1.0, float('inf')]),
])
def test_argument_validation(kw):
    with pytest.raises(ValueError):
        GaussianMixture((3,), **kw)


def test_packed_block_layout():
    K, d = 3, 5
    means, scales, weights = _params(K, d, 'Kd', 5)
    pot = GaussianMixture(d, means, scales, weights)
    a, b = pot.packed()
    assert a.dtype == torch.float32 and b.dtype == torch.float32 and not a.is_cuda
    assert a.shape == (K * d + K,) and b.shape == (K * d,)
    lam = 1.0 / scales ** 2
    w = weights / weights.sum()
    c = torch.log(w) + 0.5 * torch.log(lam).sum(1)
    assert torch.allclose(a[:K * d].double(), lam.reshape(-1), rtol=1e-6)          # lam (K, d) row-major
    assert torch.allclose(a[K * d:].double(), c, rtol=1e-6, atol=1e-6)             # then c (K)
    assert torch.equal(b, means.reshape(-1).float())                               # means (K, d) row-major


ROUTES = {   # family -> (quadratic, funnel, mixture K <= 8, mixture K = 9)
    'mcmc': (True, True, True, False),
    'flow_mh': (True, True, True, False),
    'imh_parallel': (True, True, False, False),
    'neutra': (True, True, False, False),
    'dlmc_step': (True, True, False, False),
    'fit': (True, True, False, False),
}


def test_routing_helper_every_family_and_kind():
    assert set(ROUTES) == set(FAMILIES)
    pots = (QuadraticPotential(4, 2.0, 0.5), Funnel(4), GaussianMixture(4, torch.randn(8, 4)),
            GaussianMixture(4, torch.randn(9, 4)))
    extra = (SumOfSquares(4), DiagonalGaussian(4, 1.0, 2.0))
    for fam, want in ROUTES.items():
        assert tuple(p.fused_in(fam) for p in pots) == want, fam
        assert all(p.fused_in(fam) for p in extra)
        for p, w in zip(pots, want):
            assert resolve_target(p, (4,), family=fam) is (p if w else None)
        assert resolve_target(pots[2], (4,)) is pots[2]   # no family: the object itself, as before
    with pytest.raises(ValueError):
        pots[0].fused_in('transport')


def test_recognize_never_infers_a_mixture():
    pot = GaussianMixture(3, [[0.0] * 3, [4.0] * 3], 1.0, [0.7, 0.3])
    assert recognize(lambda x: pot(x), (3,)) is None
    assert resolve_target(lambda x: pot(x), (3,), fuse='auto') is None
    # a one-component mixture is a Gaussian: the recogniser may find the quadratic, never a mixture
    one = GaussianMixture(3, [[1.0, 2.0, 3.0]], 0.5)
    r = recognize(lambda x: one(x), (3,))
    assert r is None or (type(r) is QuadraticPotential)
    assert isinstance(pot, Potential)

