"""Kinds 0 to 3, the kinds of csrc/pot_basic.hpp: quadratic (with its named special cases), funnel, Gaussian mixture and
Bayesian logistic regression."""
import math

import torch

from .. import hip
from ._base import Potential, _design_and_labels, _event_shape


class QuadraticPotential(Potential):
    """U(x) = sum_j a_j (x_j - b_j)^2 with per-coordinate or scalar a, b."""

    def __init__(self, event_shape, a=1.0, b=0.0):
        self.event_shape = _event_shape(event_shape)
        d = self.event_size
        self.a = self._norm(a, d)
        self.b = self._norm(b, d)
        self._dev = {}

    @staticmethod
    def _norm(v, d):
        if isinstance(v, (int, float)):
            return float(v)
        t = torch.as_tensor(v, dtype=torch.float32).reshape(-1)
        if t.numel() == 1:
            return float(t)
        if t.numel() != d:
            raise ValueError('potential parameter must be a scalar or have event_size entries')
        return t.contiguous()

    def __call__(self, x):
        n = x.shape[0]
        xf = x.reshape(n, -1)
        a, b = self._params_like(xf)
        return torch.sum(a * (xf - b) ** 2, dim=-1)

    def _params_like(self, xf):
        """a, b next to `xf`: the device copies the descriptor uses are kept (a host-to-device copy per call would also keep
        a fit step that evaluates the potential out of a HIP graph)"""
        if isinstance(self.a, float) and isinstance(self.b, float):
            return self.a, self.b
        if xf.dtype == torch.float32 and xf.is_cuda:
            da, db = self._copy(xf.device)
            return (self.a if da is None else da), (self.b if db is None else db)
        return (self.a if isinstance(self.a, float) else self.a.to(xf)), (self.b if isinstance(self.b, float) else self.b.to(xf))

    def _copy(self, device):
        """(a, b) of `device`, None for a scalar one, made once per device"""
        return self._cached(str(device), lambda: tuple(None if isinstance(v, float) else v.to(device) for v in (self.a, self.b)))

    def descriptor(self, device):
        da, db = self._copy(device)
        return hip.NfmcPotential(hip.POT_QUADRATIC, 0, hip.ptr(da), hip.ptr(db),
                                 self.a if isinstance(self.a, float) else 0.0,
                                 self.b if isinstance(self.b, float) else 0.0)


class SumOfSquares(QuadraticPotential):
    """U(x) = sum x^2: the reference's "standard Gaussian potential" (target N(0, I/2))."""

    def __init__(self, event_shape):
        super().__init__(event_shape, 1.0, 0.0)


class DiagonalGaussian(QuadraticPotential):
    """U(x) = sum (x - mu)^2 / (2 sigma^2) (normalising constant dropped, as MH ratios ignore it)."""

    def __init__(self, event_shape, mu=0.0, sigma=1.0):
        s = torch.as_tensor(sigma, dtype=torch.float32)
        super().__init__(event_shape, (1.0 / (2.0 * s * s)) if s.numel() > 1 else 1.0 / (2.0 * float(s) ** 2), mu)


class Funnel(Potential):
    """U(x) = x_0^2/(2 s^2) + sum_{i>=1} [ x_i^2 / (2 e^{x_0}) + x_0/2 ]  (Neal's funnel, s = 3)."""

    def __init__(self, event_shape, scale: float = 3.0):
        self.event_shape = _event_shape(event_shape)
        self.scale = float(scale)

    def __call__(self, x):
        n = x.shape[0]
        xf = x.reshape(n, -1)
        x0 = xf[:, 0]
        return x0 ** 2 / (2 * self.scale ** 2) + 0.5 * torch.exp(-x0) * torch.sum(xf[:, 1:] ** 2, dim=-1) \
            + 0.5 * (xf.shape[1] - 1) * x0

    def descriptor(self, device):
        return hip.NfmcPotential(hip.POT_FUNNEL, 0, None, None, self.scale, 0.0)


class GaussianMixture(Potential):
    """Diagonal Gaussian mixture:  U(x) = -logsumexp_k [ c_k - 1/2 sum_j lam_kj (x_j - mu_kj)^2 ],
    lam_kj = 1 / sigma_kj^2,  c_k = log w_k + 1/2 sum_j log lam_kj  (the constant d/2 log 2 pi is dropped).

    means (K, *event_shape) or (K, d); scales (standard deviations) a scalar, (K,) or (K, d); weights None (uniform) or
    (K,), normalised here.  The fused kernels take K <= 8 (hip.MIXTURE_MAX_COMPONENTS) in the mcmc and flow-MH launch
    families; every other family, and a larger K, runs on the split or composed path (`fused_in`)."""

    fused_families = ('mcmc', 'flow_mh')

    def __init__(self, event_shape, means, scales=1.0, weights=None):
        self.event_shape = _event_shape(event_shape)
        d = self.event_size
        mu = torch.as_tensor(means, dtype=torch.float64)
        if mu.dim() < 1 or mu.shape[0] < 1:
            raise ValueError('means must have a leading component axis with K >= 1 entries')
        K = int(mu.shape[0])
        if mu[0].numel() != d or (tuple(mu.shape[1:]) not in (self.event_shape, (d,))):
            raise ValueError('means must be (K, *event_shape) or (K, d), got %s' % (tuple(mu.shape),))
        mu = mu.reshape(K, d)
        sg = torch.as_tensor(scales, dtype=torch.float64)
        if sg.dim() == 0:
            sg = sg.expand(K, d)
        elif tuple(sg.shape) == (K,):
            sg = sg[:, None].expand(K, d)
        elif sg.shape[0] == K and sg[0].numel() == d:
            sg = sg.reshape(K, d)
        else:
            raise ValueError('scales must be a scalar, (K,) or (K, d), got %s' % (tuple(sg.shape),))
        if weights is None:
            w = torch.full((K,), 1.0 / K, dtype=torch.float64)
        else:
            w = torch.as_tensor(weights, dtype=torch.float64).reshape(-1)
            if w.numel() != K:
                raise ValueError('weights must have K = %d entries' % K)
        for name, v in (('means', mu), ('scales', sg), ('weights', w)):
            if not bool(torch.isfinite(v).all()):
                raise ValueError('%s must be finite' % name)
        if not bool((sg > 0).all()):
            raise ValueError('scales must be positive')
        if not bool((w > 0).all()):
            raise ValueError('weights must be positive')
        w = w / w.sum()
        lam = 1.0 / (sg * sg)
        self.n_components = K
        self.means = mu.contiguous()                                   # (K, d), fp64 masters; the kernels get fp32
        self.lam = lam.contiguous()                                    # (K, d)
        self.weights = w
        self.log_norm = torch.log(w) + 0.5 * torch.log(lam).sum(1)   # c_k
        self._dev = {}

    def fused_in(self, family: str) -> bool:
        return super().fused_in(family) and self.n_components <= hip.MIXTURE_MAX_COMPONENTS

    def packed(self):
        """The descriptor's two blocks on the host: a = [lam (K, d) row-major | c (K)], b = means (K, d) row-major."""
        return torch.cat([self.lam.reshape(-1), self.log_norm]).float(), self.means.reshape(-1).float()

    def _params_like(self, xf):
        """(lam, mu, c) next to `xf`; fp32 device copies are kept (like QuadraticPotential._params_like)."""
        if xf.dtype == torch.float32 and xf.is_cuda:
            return self._pack(xf.device)[2]
        return tuple(v.to(xf) for v in (self.lam, self.means, self.log_norm))

    def _pack(self, device):
        """(a, b, (lam, mu, c) as views of them) of `device`, made once per device"""
        def make():
            a, b = self.packed()
            a, b = a.to(device), b.to(device)
            K, d = self.n_components, self.event_size
            return a, b, (a[:K * d].view(K, d), b.view(K, d), a[K * d:])
        return self._cached(str(device), make)

    def __call__(self, x):
        n = x.shape[0]
        xf = x.reshape(n, -1)
        lam, mu, c = self._params_like(xf)
        diff = xf[:, None, :] - mu                                                 # (n, K, d)
        e = c - 0.5 * torch.sum(lam * diff * diff, dim=-1)                        # (n, K)
        return -torch.logsumexp(e, dim=-1)

    def descriptor(self, device):
        a, b, _ = self._pack(device)
        return hip.NfmcPotential(hip.POT_GAUSSIAN_MIXTURE, self.n_components, hip.ptr(a), hip.ptr(b), 0.0, 0.0)


class BayesianLogisticRegression(Potential):
    """Bayesian logistic regression, labels y in {0, 1}, prior theta ~ N(0, prior_scale^2 I):
        U(theta) = sum_i [softplus(z_i) - y_i z_i] + |theta|^2 / (2 prior_scale^2),   z = X theta,
        softplus(z) = max(z, 0) + log1p(exp(-|z|))   (finite for every finite z; constants dropped).
    X (N, d), y (N,) of bools or numbers; an intercept is a column of ones in X.  The fused kernels evaluate it in the mcmc
    and flow-MH launch families; every other family runs on the split or composed path (`fused_in`).  It is never
    inferred from a plain callable: pass the object as the target."""

    fused_families = ('mcmc', 'flow_mh')

    def __init__(self, X, y, prior_scale=1.0):
        X, y = _design_and_labels(X, y, 'd')
        N, d = (int(v) for v in X.shape)
        s = float(prior_scale)
        if not (s > 0 and math.isfinite(s)):
            raise ValueError('prior_scale must be positive and finite, got %r' % (prior_scale,))
        iv32 = float(torch.tensor(1.0 / (s * s), dtype=torch.float32))
        if not (iv32 > 0 and math.isfinite(iv32)):   # the kernels take 1/prior_scale^2 in fp32
            raise ValueError('1 / prior_scale^2 must be a positive finite fp32 number, prior_scale = %r' % (prior_scale,))
        self.event_shape = (d,)
        self.n_rows = N
        self.X, self.y = X, y            # fp64 masters; the kernels get fp32
        self.prior_scale = s
        self.inv_var = 1.0 / (s * s)
        self._dev = {}

    def _copy(self, device):
        """The fp32 (X, y) of `device`, made once per device (every shard of a sharded run gets its own)."""
        return self._cached(str(device), lambda: (self.X.float().to(device).contiguous(), self.y.float().to(device).contiguous()))

    def __call__(self, x):
        n = x.shape[0]
        xf = x.reshape(n, -1)
        if xf.dtype == torch.float32 and xf.is_cuda:
            X, y = self._copy(xf.device)
        else:
            X, y = self.X.to(xf), self.y.to(xf)
        z = xf @ X.t()                                                            # (n, N)
        data = torch.sum(torch.clamp(z, min=0) + torch.log1p(torch.exp(-z.abs())) - y * z, dim=1)
        return data + (0.5 * self.inv_var) * torch.sum(xf * xf, dim=1)

    def descriptor(self, device):
        X, y = self._copy(device)
        return hip.NfmcPotential(hip.POT_LOGISTIC_REGRESSION, self.n_rows, hip.ptr(X), hip.ptr(y), self.inv_var, 0.0)
