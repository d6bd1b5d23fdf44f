"""The latent Gaussian model with a dense prior covariance (csrc/pot_lgm.hpp)."""
import math

import torch

from .. import hip
from ._base import VALU_FAMILIES, Potential, _as_fp64, _check_finite, _event_shape, _one_of, _spd, _spd_inverse
from ._observations import SiteObservations


class LatentGaussianModel(SiteObservations, Potential):
    """A latent Gaussian model: a Gaussian (process) prior f ~ N(m, K) on a latent vector of d coordinates and a
    non-Gaussian likelihood on each coordinate.  The log-Gaussian Cox process, GP classification and robust GP regression;
    the model class elliptical slice sampling was written for.  Coordinate j carries an observation y_j and a weight
    w_j >= 0; w_j = 0 (or `observed[j]` False) means "not observed": the coordinate adds exactly 0 to U and grad U.
    The negative log-likelihood l_j(f), constants dropped:

        'poisson'    l = w e^f - y f                              w: exposure / cell area, y a count
        'binomial'   l = w softplus(f) - y f                      w: number of trials (1 = Bernoulli), 0 <= y <= w
        'student_t'  l = w (nu+1)/2 log1p((y-f)^2 / (nu s^2))     w: a 0 / 1 mask or a weight, nu = `dof`, s = `scale`

    One object holds one of two parameterisations of the same posterior, K = L L^T (Cholesky), Lambda = K^-1:

        'centered'   x = f:             U = 1/2 (x-m)^T Lambda (x-m) + sum_j l_j(x_j),  grad U = Lambda (x-m) + l'(x)
        'whitened'   x = z, f = m + L z:  U = 1/2 |z|^2 + sum_j l_j(f_j),                 grad U = z + L^T l'(f)

    The whitened posterior is close to N(0, I) where the centred one is badly conditioned; `reparameterized` gives the
    other form of the same data and prior.  `latent` / `coordinates` convert between x and f, `mean_response` is the rate,
    probability or location, `prior_draws` draws from the prior and `hessian_bound` gives lambda_max of the Hessian at a
    state, for step sizes.  Validated in fp64 on the host: K finite, symmetric to a relative 1e-6 of its largest entry
    (then symmetrised) and positive definite (the Cholesky factorisation succeeds); counts non-negative integers;
    0 <= y <= w and integer trials for the binomial family; w >= 0; nu > 0 and s > 0; everything finite in fp32 (the
    kernels read fp32 copies).  The fused kernels evaluate it in the mcmc, flow-MH and NeuTra launch families (NeuTra on
    its VALU kernels, conditioners of at most 32 units) for d up to 1024; every other family runs on the split or
    composed path (`fused_in`).  It is never inferred from a plain callable: pass the object as the target."""

    neutra_matrix_cores = False
    fused_families, fused_max_dim = VALU_FAMILIES, 1024
    PARAMETERIZATIONS = ('centered', 'whitened')
    SYMMETRY_RTOL = 1e-6
    CHUNK_FLOATS = 1 << 24   # __call__ forms at most this many entries of the (chunk, d) products' inputs at once

    def __init__(self, y, covariance, likelihood='poisson', mean=0.0, weight=None, observed=None,
                 parameterization='whitened', dof=4.0, scale=1.0, event_shape=None):
        _one_of('likelihood', likelihood, self.LIKELIHOODS)
        _one_of('parameterization', parameterization, self.PARAMETERIZATIONS)
        K, chol = _spd('covariance', _as_fp64(covariance), self.SYMMETRY_RTOL)
        d = int(K.shape[0])
        lam = _spd_inverse(chol)
        for name, v in (('the Cholesky factor of covariance', chol), ('the precision matrix', lam)):
            _check_finite(v, '%s must be finite in fp32 too (the kernels read an fp32 copy)' % name)
        yv = _as_fp64(y).reshape(-1)
        if yv.numel() != d:
            raise ValueError('y must have d = %d entries, got %d' % (d, yv.numel()))
        self._set_observations(yv, d, 'd', likelihood, mean, weight, observed, dof, scale)
        self.event_shape = _event_shape(event_shape, d)
        self.dim = d
        self.parameterization = parameterization
        self.whitened = parameterization == 'whitened'
        self.covariance = K.contiguous()
        self.cholesky = chol.contiguous()
        self.precision = lam.contiguous()
        self._dev = {}

    # ------------------------------------------------------------------ kernel builders and presets
    @staticmethod
    def _sqdist(points):
        P = _as_fp64(points)
        if P.dim() == 1:
            P = P[:, None]
        if P.dim() != 2 or P.shape[0] < 1 or not bool(torch.isfinite(P).all()):
            raise ValueError('points must be a finite (d, k) array, got shape %s' % (tuple(P.shape),))
        diff = P[:, None, :] - P[None, :, :]
        return (diff * diff).sum(-1)

    @staticmethod
    def _kernel_args(variance, lengthscale, jitter):
        v, l, j = float(variance), float(lengthscale), float(jitter)
        if not (math.isfinite(v) and v > 0 and math.isfinite(l) and l > 0 and math.isfinite(j) and j >= 0):
            raise ValueError('variance > 0, lengthscale > 0 and jitter >= 0, all finite, got %r, %r, %r'
                             % (variance, lengthscale, jitter))
        return v, l, j

    @staticmethod
    def squared_exponential(points, variance=1.0, lengthscale=1.0, jitter=1e-6):
        """K_ij = variance exp(-|p_i - p_j|^2 / (2 lengthscale^2)) + jitter [i = j], fp64 (d, d), of points (d, k)."""
        v, l, j = LatentGaussianModel._kernel_args(variance, lengthscale, jitter)
        s = LatentGaussianModel._sqdist(points)
        return v * torch.exp(-0.5 * s / (l * l)) + j * torch.eye(s.shape[0], dtype=torch.float64)

    @staticmethod
    def matern32(points, variance=1.0, lengthscale=1.0, jitter=1e-6):
        """K_ij = variance (1 + sqrt(3) r / lengthscale) exp(-sqrt(3) r / lengthscale) + jitter [i = j], r = |p_i - p_j|."""
        v, l, j = LatentGaussianModel._kernel_args(variance, lengthscale, jitter)
        s = LatentGaussianModel._sqdist(points)
        a = math.sqrt(3.0) * torch.sqrt(s) / l
        return v * (1.0 + a) * torch.exp(-a) + j * torch.eye(s.shape[0], dtype=torch.float64)

    @classmethod
    def log_gaussian_cox(cls, counts, variance=1.91, lengthscale=None, mean=None, jitter=1e-6, kernel='squared_exponential',
                         **model):
        """The log-Gaussian Cox process on an (H, W) grid of unit-square cells (H W <= 1024): `counts` (H, W) points per
        cell, cell centres ((i + 1/2) / H, (j + 1/2) / W), exposure 1 / (H W) per cell, prior mean log(total count)
        - variance / 2 unless given (so the prior expectation of the total rate is the total count), lengthscale
        2 / max(H, W) (two cells) unless given.  event_shape (H, W).  `model`: further constructor keywords."""
        c = torch.as_tensor(counts)
        if c.dim() != 2 or c.shape[0] < 1 or c.shape[1] < 1 or c.numel() > 1024:
            raise ValueError('counts must be an (H, W) grid with H W <= 1024, got shape %s' % (tuple(c.shape),))
        H, W = (int(v) for v in c.shape)
        c = _as_fp64(c)
        ii, jj = torch.meshgrid((torch.arange(H, dtype=torch.float64) + 0.5) / H,
                                (torch.arange(W, dtype=torch.float64) + 0.5) / W, indexing='ij')
        pts = torch.stack([ii.reshape(-1), jj.reshape(-1)], dim=1)
        if lengthscale is None:
            lengthscale = 2.0 / max(H, W)
        if mean is None:
            mean = math.log(max(float(c.sum()), 1.0)) - 0.5 * float(variance)
        build = {'squared_exponential': cls.squared_exponential, 'matern32': cls.matern32}
        if kernel not in build:
            raise ValueError('kernel must be one of %s, got %r' % (', '.join(build), kernel))
        K = build[kernel](pts, variance, lengthscale, jitter)
        args = dict(likelihood='poisson', mean=mean, weight=1.0 / (H * W), event_shape=(H, W))
        args.update(model)
        return cls(c.reshape(-1), K, **args)

    @classmethod
    def gp_classification(cls, points, labels, variance=1.0, lengthscale=1.0, jitter=1e-6, kernel='squared_exponential',
                          **model):
        """GP classification: labels 0 / 1 (or bools) at `points` (d, k), a Bernoulli likelihood with the logit link."""
        build = {'squared_exponential': cls.squared_exponential, 'matern32': cls.matern32}
        if kernel not in build:
            raise ValueError('kernel must be one of %s, got %r' % (', '.join(build), kernel))
        lab = _as_fp64(labels).reshape(-1)
        if not bool(((lab == 0) | (lab == 1)).all()):
            raise ValueError('labels must be 0 or 1')
        args = dict(likelihood='binomial', weight=1.0)
        args.update(model)
        return cls(lab, build[kernel](points, variance, lengthscale, jitter), **args)

    @classmethod
    def synthetic(cls, n, likelihood, seed, **model):
        """(potential, truth): n seeded uniform points in the unit square, K = squared_exponential(variance 1,
        lengthscale 0.25) + 0.05 I, a whitened generating state z* ~ N(0, I), f* = m + L z*, and observations drawn from
        the likelihood at f* (Poisson exposure 1, Bernoulli, Student-t noise of the model's dof and scale); all draws in
        fp64 from one CPU torch.Generator seeded with `seed`.  `model`: the constructor's keywords (mean, weight,
        parameterization, dof, scale, ...).  `truth` is the generating state in the object's own coordinates (d,), fp64."""
        n = int(n)
        if n < 1 or likelihood not in cls.LIKELIHOODS:
            raise ValueError('n >= 1 and a likelihood of %s, got %r, %r' % (', '.join(cls.LIKELIHOODS), n, likelihood))
        g = torch.Generator().manual_seed(int(seed))
        pts = torch.rand(n, 2, generator=g, dtype=torch.float64)
        K = cls.squared_exponential(pts, 1.0, 0.25, 0.05)
        proto = cls(torch.zeros(n), K, likelihood=likelihood, **model)     # validates the model, gives m, w, L
        z = torch.randn(n, generator=g, dtype=torch.float64)
        f = proto.mean + proto.cholesky @ z
        w = proto.weight
        if likelihood == 'poisson':
            y = torch.poisson(w * torch.exp(f), generator=g)
        elif likelihood == 'binomial':
            trials = int(w.max())
            draws = torch.rand(max(trials, 1), n, generator=g, dtype=torch.float64) < torch.sigmoid(f)
            y = (draws & (torch.arange(max(trials, 1))[:, None] < w[None, :])).sum(0).to(torch.float64)
        else:
            chi2 = 2.0 * torch._standard_gamma(torch.full((n,), 0.5 * proto.dof, dtype=torch.float64), generator=g)
            t = torch.randn(n, generator=g, dtype=torch.float64) / torch.sqrt(chi2 / proto.dof)
            y = f + proto.scale * t
        args = dict(model)
        args['weight'] = w
        pot = cls(y, K, likelihood=likelihood, **args)
        return pot, pot.coordinates(f)

    # ------------------------------------------------------------------ helpers
    def latent(self, x):
        """f (..., d) of the coordinates x of this object's parameterisation: x itself when centred, m + L x when
        whitened."""
        xf = self._flat(x)
        if not self.whitened:
            return xf
        return self.mean.to(xf) + xf @ self.cholesky.to(xf).t()

    def coordinates(self, f):
        """The coordinates x (..., d) of latent values f in this object's parameterisation: the inverse of `latent`
        (a triangular solve when whitened)."""
        ff = self._flat(f)
        if not self.whitened:
            return ff
        r = (ff - self.mean.to(ff))
        sol = torch.linalg.solve_triangular(self.cholesky.to(ff), r.reshape(-1, self.dim).t(), upper=False)
        return sol.t().reshape(r.shape)

    def prior_draws(self, n, seed):
        """n draws from the prior in this object's coordinates, (n, d) fp64 on the CPU: N(0, I) when whitened, N(m, K)
        when centred; one CPU torch.Generator seeded with `seed`."""
        n = int(n)
        if n < 1:
            raise ValueError('n must be >= 1, got %r' % (n,))
        z = torch.randn(n, self.dim, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float64)
        return z if self.whitened else self.mean + z @ self.cholesky.t()

    def reparameterized(self, parameterization):
        """The same data and prior in the form `parameterization`: U_whitened(z) = U_centred(m + L z) up to a constant."""
        _one_of('parameterization', parameterization, self.PARAMETERIZATIONS)
        return type(self)(self.y, self.covariance, likelihood=self.likelihood, mean=self.mean, weight=self.weight,
                          parameterization=parameterization, dof=self.dof, scale=self.scale, event_shape=self.event_shape)

    def hessian_bound(self, x):
        """lambda_max of the fp64 Hessian of U at the state x (d,) (or event-shaped) of this object's parameterisation:
        Lambda + diag(l'') when centred, I + L^T diag(l'') L when whitened.  For step sizes: MALA h ~ d^(-1/3) / bound,
        HMC h ~ d^(-1/4) / sqrt(bound)."""
        xf = self._flat(torch.as_tensor(x).detach().to('cpu', torch.float64)).reshape(self.dim)
        c = self._lik(self.latent(xf), self.y, self.weight, second=True)
        if self.whitened:
            Hm = torch.eye(self.dim, dtype=torch.float64) + self.cholesky.t() @ (c[:, None] * self.cholesky)
        else:
            Hm = self.precision + torch.diag(c)
        return float(torch.linalg.eigvalsh(0.5 * (Hm + Hm.t())).max())

    # ------------------------------------------------------------------ evaluation in torch ops
    def _copy(self, device, dtype=torch.float32):
        """(matrix, m, y, w) of `device` in `dtype`, made once per (device, dtype): the matrix is L^T when whitened (so
        that f = m + z @ L^T) and Lambda when centred."""
        def make():
            M = self.cholesky.t() if self.whitened else self.precision
            return tuple(v.to(device, dtype).contiguous() for v in (M, self.mean, self.y, self.weight))
        return self._cached((str(device), dtype), make)

    def _u_chunk(self, xf, M, m, y, w):
        if self.whitened:
            f = m + xf @ M
            prior = 0.5 * torch.sum(xf * xf, dim=1)
        else:
            f = xf
            r = xf - m
            prior = 0.5 * torch.sum((r @ M) * r, dim=1)
        return prior + torch.sum(self._lik(f, y, w), dim=1)

    def __call__(self, x, chunk=None):
        """U (n,) of states x (n, ...) in torch ops.  Evaluated in chunks of chains so that at most CHUNK_FLOATS entries
        of the (chunk, d) intermediates exist at once (`chunk` overrides the chunk's number of chains)."""
        n = x.shape[0]
        xf = x.reshape(n, -1)
        M, m, y, w = self._copy(xf.device, xf.dtype)
        k = int(chunk) if chunk is not None else max(1, self.CHUNK_FLOATS // self.dim)
        if k < 1:
            raise ValueError('chunk must be >= 1, got %r' % (chunk,))
        if k >= n:
            return self._u_chunk(xf, M, m, y, w)
        return torch.cat([self._u_chunk(xf[i:i + k], M, m, y, w) for i in range(0, n, k)])

    # ------------------------------------------------------------------ the kernels' view
    def code(self):
        """a_scalar of the descriptor: likelihood code + 4 [whitened]."""
        return float(self.LIKELIHOODS.index(self.likelihood) + (4 if self.whitened else 0))

    def data_block(self):
        """The kernels' view (NFMC_POT_LATENT_GAUSSIAN, include/nfmc_hip.h), fp32 on the CPU: (matrix block, table).
        Matrix block: Lambda (d, d) when centred; (2, d, d) = L^T then L when whitened.  Table: 8 floats
        ((nu+1)/2, 1/(nu s^2), nu s^2, nu+1, 0, 0, 0, 0), zeros unless Student-t, then the rows m, y, w of
        d4 = 4 ceil(d / 4) floats each, zero past d."""
        if self.whitened:
            A = torch.stack([self.cholesky.t(), self.cholesky]).to(torch.float32).contiguous()
        else:
            A = self.precision.to(torch.float32).contiguous()
        return A, self._table(self.dim).to(torch.float32)

    def descriptor(self, device):
        A, tab = self._descriptor_blocks(device)
        return hip.NfmcPotential(hip.POT_LATENT_GAUSSIAN, self.dim, hip.ptr(A), hip.ptr(tab), self.code(), 0.0)
