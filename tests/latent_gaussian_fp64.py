"""fp64 restatement of the latent Gaussian model (potentials.LatentGaussianModel), for the host and GPU tests, and the
seeded problems both use.  Written differently from the class: the quadratic form through torch.einsum, the latent
values as an explicit m + z L^T, the three likelihoods from torch.nn.functional / torch.log where the class uses
logaddexp / log1p, the unobserved coordinates by an index list instead of a select, and the gradient by autograd."""
import math

import torch
import torch.nn.functional as F

LIKELIHOODS = ('poisson', 'binomial', 'student_t')
PARAMETERIZATIONS = ('centered', 'whitened')
PAIRS = [(lik, par) for lik in LIKELIHOODS for par in PARAMETERIZATIONS]


class LatentGaussian64:
    """U of the latent Gaussian model in fp64 (constants dropped), callable on (n, ...) tensors of any dtype, works under
    autograd.  centred: x = f, U = 1/2 (x-m)^T K^-1 (x-m) + sum_j l_j(x_j); whitened: x = z, f = m + L z,
    U = 1/2 |z|^2 + sum_j l_j(f_j), K = L L^T.  l_j: w e^f - y f | w softplus(f) - y f |
    w (nu+1)/2 log(1 + (y-f)^2 / (nu s^2)), summed over the coordinates with w_j > 0 only."""

    def __init__(self, y, covariance, likelihood, mean, weight, whitened, dof=4.0, scale=1.0):
        assert likelihood in LIKELIHOODS
        self.K = torch.as_tensor(covariance).double()
        self.d = int(self.K.shape[0])
        self.L = torch.linalg.cholesky(self.K)
        self.lam = torch.linalg.inv(self.K)
        self.lam = 0.5 * (self.lam + self.lam.t())
        self.y = torch.as_tensor(y).double().reshape(-1)
        self.m = torch.as_tensor(mean).double().expand(self.d).clone()
        self.w = torch.as_tensor(weight).double().expand(self.d).clone()
        self.on = torch.nonzero(self.w > 0).reshape(-1)
        self.likelihood, self.whitened = likelihood, bool(whitened)
        self.dof, self.scale = float(dof), float(scale)

    def latent(self, x):
        x = x.reshape(x.shape[0], -1).double()
        if not self.whitened:
            return x
        return self.m[None, :] + torch.einsum('ni,ji->nj', x, self.L)

    def coordinates(self, f):
        f = f.reshape(f.shape[0], -1).double()
        if not self.whitened:
            return f
        return torch.linalg.solve(self.L, (f - self.m).t()).t()

    def data_term(self, f):
        f, y, w = f[:, self.on], self.y[self.on], self.w[self.on]
        if self.likelihood == 'poisson':
            l = w * torch.exp(f) - y * f
        elif self.likelihood == 'binomial':
            l = w * F.softplus(f, beta=1.0, threshold=1e9) - y * f
        else:
            l = w * 0.5 * (self.dof + 1.0) * torch.log(1.0 + (y - f) ** 2 / (self.dof * self.scale ** 2))
        return l.sum(dim=1)

    def __call__(self, x):
        x = x.reshape(x.shape[0], -1).double()
        if self.whitened:
            prior = 0.5 * torch.einsum('ni,ni->n', x, x)
        else:
            r = x - self.m
            prior = 0.5 * torch.einsum('ni,ij,nj->n', r, self.lam, r)
        return prior + self.data_term(self.latent(x))

    def grad(self, x):
        t = x.reshape(x.shape[0], -1).double().detach().requires_grad_(True)
        (g,) = torch.autograd.grad(self(t).sum(), t)
        return g

    def hessian_lmax(self, x):
        """lambda_max of the autograd Hessian of U at one state x (d,)."""
        H = torch.autograd.functional.hessian(lambda t: self(t[None])[0], x.double().reshape(-1))
        return float(torch.linalg.eigvalsh(0.5 * (H + H.t())).max())


def se_covariance(points, variance, lengthscale, jitter):
    """variance exp(-|p_i - p_j|^2 / (2 lengthscale^2)) + jitter I through torch.cdist."""
    r = torch.cdist(points.double(), points.double())
    return variance * torch.exp(-(r / lengthscale) ** 2 / 2.0) + jitter * torch.eye(points.shape[0], dtype=torch.float64)


NU, SCALE = 4.0, 0.5


def problem_data(d, likelihood, seed):
    """The seeded problem of the GPU tests, independent of the parameterisation: d uniform points in the unit square,
    K = SE(variance 1, lengthscale 0.25) + 0.05 I, m = 1 (Poisson) or 0, a generating state z* ~ N(0, I), f* = m + L z*,
    weights U(0.5, 1.5) (Poisson), trials 1 .. 5 (binomial) or 1 (Student-t, nu = 4, s = 0.5, 10 % outliers of 5 s),
    observations drawn at f*, and a seeded 20 % of the coordinates unobserved (weight 0).  Returns a dict."""
    g = torch.Generator().manual_seed(int(seed))
    pts = torch.rand(d, 2, generator=g, dtype=torch.float64)
    K = se_covariance(pts, 1.0, 0.25, 0.05)
    L = torch.linalg.cholesky(K)
    m = torch.full((d,), 1.0 if likelihood == 'poisson' else 0.0, dtype=torch.float64)
    zs = torch.randn(d, generator=g, dtype=torch.float64)
    fs = m + L @ zs
    if likelihood == 'poisson':
        w = 0.5 + torch.rand(d, generator=g, dtype=torch.float64)
        y = torch.poisson(w * torch.exp(fs), generator=g)
    elif likelihood == 'binomial':
        w = torch.randint(1, 6, (d,), generator=g).double()
        hits = torch.rand(5, d, generator=g, dtype=torch.float64) < torch.sigmoid(fs)
        y = (hits & (torch.arange(5)[:, None] < w[None, :])).sum(0).double()
    else:
        w = torch.ones(d, dtype=torch.float64)
        noise = SCALE * torch.randn(d, generator=g, dtype=torch.float64)
        out = torch.rand(d, generator=g, dtype=torch.float64) < 0.10
        sign = torch.where(torch.rand(d, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0).double()
        y = fs + torch.where(out, 5.0 * SCALE * sign, noise)
    observed = torch.rand(d, generator=g, dtype=torch.float64) >= 0.20
    return dict(points=pts, K=K, L=L, mean=m, z_star=zs, f_star=fs, weight=w, y=y, observed=observed,
                likelihood=likelihood)


def make_pair(data, parameterization, event_shape=None):
    """(package potential, fp64 restatement) of problem_data's dict in one parameterisation."""
    from nfmc_amd.potentials import LatentGaussianModel
    lik = data['likelihood']
    pot = LatentGaussianModel(data['y'], data['K'], likelihood=lik, mean=data['mean'], weight=data['weight'],
                              observed=data['observed'], parameterization=parameterization, dof=NU, scale=SCALE,
                              event_shape=event_shape)
    w = torch.where(data['observed'], data['weight'], torch.zeros_like(data['weight']))
    ref = LatentGaussian64(data['y'], data['K'], lik, data['mean'], w, parameterization == 'whitened', NU, SCALE)
    return pot, ref


def starts(data, ref, n, seed, spread=0.3):
    """n fp32 starts in the coordinates of `ref`: z* + spread eps in the whitened coordinates, mapped to f = m + L z when
    centred, rounded to fp32."""
    g = torch.Generator().manual_seed(int(seed))
    z = data['z_star'][None, :] + spread * torch.randn(n, data['z_star'].numel(), generator=g, dtype=torch.float64)
    x = z if ref.whitened else data['mean'][None, :] + z @ data['L'].t()
    return x.float()


def truth(data, ref):
    """The generating state in the coordinates of `ref`, (d,) fp64."""
    return data['z_star'] if ref.whitened else data['f_star']
