"""fp64 restatement of the full-rank Gaussian target (potentials.FullRankGaussian), for the host and GPU tests: U and its
autograd gradient, and seeded symmetric positive-definite matrices with a chosen condition number."""
import math

import torch


class FullRankU64:
    """U(x) = 1/2 (x - mu)^T Lambda (x - mu) in fp64, Lambda the precision.  Written as the quadratic form through
    torch.einsum, not the class's (r @ Lambda) * r.  Callable on (n, ...) tensors of any dtype; works under autograd."""

    def __init__(self, precision, mu):
        self.lam = torch.as_tensor(precision).double()
        self.mu = torch.as_tensor(mu).double().reshape(-1)

    def __call__(self, x):
        r = x.reshape(x.shape[0], -1).double() - self.mu
        return 0.5 * torch.einsum('ni,ij,nj->n', r, self.lam, r)

    def grad(self, x):
        t = x.reshape(x.shape[0], -1).double().detach().requires_grad_(True)
        (g,) = torch.autograd.grad(self(t).sum(), t)
        return g


def spd(d, cond, seed):
    """(d, d) fp64 symmetric positive definite: Q diag(lam) Q^T with Q the orthogonal factor of a seeded Gaussian
    matrix (signs fixed by R's diagonal) and lam log-spaced from 1 to `cond`, so the condition number is `cond`."""
    g = torch.Generator().manual_seed(seed)
    q, r = torch.linalg.qr(torch.randn(d, d, generator=g, dtype=torch.float64))
    q = q * torch.sign(torch.diagonal(r))
    lam = torch.logspace(0.0, math.log10(cond), d, dtype=torch.float64) if d > 1 else torch.ones(1, dtype=torch.float64)
    m = (q * lam) @ q.t()
    return 0.5 * (m + m.t())


def draw(precision, mu, n, seed, spread=1.0):
    """n fp64 draws of N(mu, spread^2 Lambda^-1): mu + spread L^-T z with Lambda = L L^T."""
    lam = torch.as_tensor(precision).double()
    L = torch.linalg.cholesky(lam)
    z = torch.randn(n, lam.shape[0], generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    return torch.as_tensor(mu).double().reshape(1, -1) + spread * torch.linalg.solve_triangular(L.t(), z.t(), upper=True).t()
