"""Closed-form potential descriptors: callables (usable as `target` exactly like the reference's
`target(x) -> (n,)` callables, nfmc/sample.py:35-37) that ALSO describe themselves to the HIP kernels,
so U and grad U are evaluated in-kernel instead of by `torch.autograd.grad` (langevin.py:66-68).

The reference's own potential objects live in the absent third-party package `potentials`
(nfmc/sample.py:17); `SumOfSquares` is the README/test potential (README.md:45-46, test/util.py:4-5),
`Funnel` is the build's C4 potential.

`recognize(target, event_shape)` lets plain Python callables such as the README's
`lambda x: torch.sum(x**2, dim=1)` take the fused path: it probes the callable, fits
U = sum_j a_j (x_j - b_j)^2 + c and accepts it only if the fit reproduces the callable (and its autograd
gradient) on fresh points at radii from 0.1 to 100 and around the run's own x0 to 1e-5 relative.  It is an
inference from finitely many probes (see its docstring); `fuse='never'` turns it off.
"""
import ctypes as C
import logging
import math
import numbers
from typing import Optional, Sequence, Tuple, Union

import torch

from . import hip


# Launch families a closed-form potential can be routed to (Potential.fused_in):
#   'mcmc'          mala / ula / mh / hmc / uhmc, device warmup tuning, the jump_* inner loop and its fused jump tail
#   'flow_mh'       the flow-MH step of imh / adaptive_imh / jump_* / dlmc (nfmc_flow_mh_steps_f32)
#   'imh_parallel'  the data-parallel FixedIMH kernel (nfmc_imh_parallel_f32)
#   'neutra'        the NeuTra gradient and HMC kernels
#   'dlmc_step'     dlmc's fused gradient step (nfmc_dlmc_step_f32)
#   'fit'           the device variational fit (nfmc_flow_variational_fit_step_f32)
FAMILIES = ('mcmc', 'flow_mh', 'imh_parallel', 'neutra', 'dlmc_step', 'fit')


class Potential:
    """Base: `event_shape`, `__call__(x) -> (n,)` in torch ops, `descriptor(device)` for the kernels."""

    event_shape: Tuple[int, ...]
    # NeuTra may present this kind to its matrix-core kernels (csrc/neutra_mfma.hip), which evaluate quadratic and funnel
    # targets only: every other kind of the NeuTra family sets it False and keeps the flow's own width (VALU kernels)
    neutra_matrix_cores = True

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        raise NotImplementedError

    def descriptor(self, device) -> hip.NfmcPotential:
        raise NotImplementedError

    def fused_in(self, family: str) -> bool:
        """Whether the kernels of launch family `family` (FAMILIES) may be handed this potential's descriptor.  False
        sends the family to the split or composed path, exactly as for an arbitrary callable.  The quadratic and funnel
        kinds answer True everywhere: their kernels decide by themselves, as before."""
        if family not in FAMILIES:
            raise ValueError('unknown launch family %r (one of %s)' % (family, ', '.join(FAMILIES)))
        return True

    def jump_tail_ok(self) -> bool:
        """Whether a jump sampler with `fuse_jump_tail` set may run the jump behind the inner kernel's launch for this
        potential (True), or should leave it on the flow-MH kernel where the tail measures slower (ParticleSystem)."""
        return True

    @property
    def event_size(self):
        return int(math.prod(self.event_shape))


class QuadraticPotential(Potential):
    """U(x) = sum_j a_j (x_j - b_j)^2 with per-coordinate or scalar a, b."""

    def __init__(self, event_shape, a=1.0, b=0.0):
        if isinstance(event_shape, int):
            event_shape = (event_shape,)
        self.event_shape = tuple(event_shape)
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
            key = str(xf.device)
            if key not in self._dev:
                self._dev[key] = tuple(None if isinstance(v, float) else v.to(xf.device) for v in (self.a, self.b))
            da, db = self._dev[key]
            return (self.a if da is None else da), (self.b if db is None else db)
        return (self.a if isinstance(self.a, float) else self.a.to(xf)), (self.b if isinstance(self.b, float) else self.b.to(xf))

    def descriptor(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = tuple(None if isinstance(v, float) else v.to(device) for v in (self.a, self.b))
        da, db = self._dev[key]
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
        if isinstance(event_shape, int):
            event_shape = (event_shape,)
        self.event_shape = tuple(event_shape)
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

    def __init__(self, event_shape, means, scales=1.0, weights=None):
        if isinstance(event_shape, int):
            event_shape = (event_shape,)
        self.event_shape = tuple(event_shape)
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
        return super().fused_in(family) and family in ('mcmc', 'flow_mh') and \
            self.n_components <= hip.MIXTURE_MAX_COMPONENTS

    def packed(self):
        """The descriptor's two blocks on the host: a = [lam (K, d) row-major | c (K)], b = means (K, d) row-major."""
        return torch.cat([self.lam.reshape(-1), self.log_norm]).float(), self.means.reshape(-1).float()

    def _params_like(self, xf):
        """(lam, mu, c) next to `xf`; fp32 device copies are kept (like QuadraticPotential._params_like)."""
        if xf.dtype == torch.float32 and xf.is_cuda:
            key = str(xf.device)
            if key not in self._dev:
                self._pack(xf.device)
            return self._dev[key][2]
        return tuple(v.to(xf) for v in (self.lam, self.means, self.log_norm))

    def _pack(self, device):
        a, b = self.packed()
        a, b = a.to(device), b.to(device)
        K, d = self.n_components, self.event_size
        self._dev[str(device)] = (a, b, (a[:K * d].view(K, d), b.view(K, d), a[K * d:]))

    def __call__(self, x):
        n = x.shape[0]
        xf = x.reshape(n, -1)
        lam, mu, c = self._params_like(xf)
        diff = xf[:, None, :] - mu                                                 # (n, K, d)
        e = c - 0.5 * torch.sum(lam * diff * diff, dim=-1)                        # (n, K)
        return -torch.logsumexp(e, dim=-1)

    def descriptor(self, device):
        key = str(device)
        if key not in self._dev:
            self._pack(device)
        a, b, _ = self._dev[key]
        return hip.NfmcPotential(hip.POT_GAUSSIAN_MIXTURE, self.n_components, hip.ptr(a), hip.ptr(b), 0.0, 0.0)



class BayesianLogisticRegression(Potential):
    """Bayesian logistic regression, labels y in {0, 1}, prior theta ~ N(0, prior_scale^2 I):
        U(theta) = sum_i [softplus(z_i) - y_i z_i] + |theta|^2 / (2 prior_scale^2),   z = X theta,
        softplus(z) = max(z, 0) + log1p(exp(-|z|))   (finite for every finite z; constants dropped).
    X (N, d), y (N,) of bools or numbers; an intercept is a column of ones in X.  The fused kernels evaluate it in the mcmc
    and flow-MH launch families; every other family runs on the split or composed path (`fused_in`).  It is never
    inferred from a plain callable: pass the object as the target."""

    def __init__(self, X, y, prior_scale=1.0):
        X = torch.as_tensor(X)
        if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError('X must be 2-D (N, d) with N, d >= 1, got shape %s' % (tuple(X.shape),))
        X = X.detach().to('cpu', torch.float64)
        if not bool(torch.isfinite(X).all()) or not bool(torch.isfinite(X.float()).all()):
            raise ValueError('X must be finite, in fp32 too (the kernels read an fp32 copy)')
        N, d = (int(v) for v in X.shape)
        y = torch.as_tensor(y).detach().to('cpu')
        if y.dim() != 1 or y.shape[0] != N:
            raise ValueError('y must be a vector of N = %d labels, got shape %s' % (N, tuple(y.shape)))
        y = y.to(torch.float64)
        if not bool(((y == 0) | (y == 1)).all()):
            raise ValueError('labels must be 0 or 1')
        s = float(prior_scale)
        if not (s > 0 and math.isfinite(s)):
            raise ValueError('prior_scale must be positive and finite, got %r' % (prior_scale,))
        iv32 = float(torch.tensor(1.0 / (s * s), dtype=torch.float32))
        if not (iv32 > 0 and math.isfinite(iv32)):   # the kernels take 1/prior_scale^2 in fp32
            raise ValueError('1 / prior_scale^2 must be a positive finite fp32 number, prior_scale = %r' % (prior_scale,))
        self.event_shape = (d,)
        self.n_rows = N
        self.X = X.contiguous()          # fp64 masters; the kernels get fp32
        self.y = y.contiguous()
        self.prior_scale = s
        self.inv_var = 1.0 / (s * s)
        self._dev = {}

    def fused_in(self, family: str) -> bool:
        return super().fused_in(family) and family in ('mcmc', 'flow_mh')

    def _copy(self, device):
        """The fp32 (X, y) of `device`, made once per device (every shard of a sharded run gets its own)."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (self.X.float().to(device).contiguous(), self.y.float().to(device).contiguous())
        return self._dev[key]

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


class FullRankGaussian(Potential):
    """Gaussian with a full (correlated) covariance:  U(x) = 1/2 (x - mu)^T Lambda (x - mu),  grad U = Lambda (x - mu),
    Lambda the precision matrix (constants dropped).  Give exactly one of `covariance` / `precision`, a (d, d) symmetric
    positive-definite matrix; `mu` has d entries; `event_shape` (default (d,)) has d elements and flattens row-major as
    for the other potentials.  Validated in fp64 on the host: finite, symmetric to a relative 1e-6 of its largest entry
    (then symmetrised), positive definite (the Cholesky factorisation succeeds), and Lambda finite in fp32 (the kernels
    read an fp32 copy).  A covariance is inverted through its fp64 Cholesky factor.  The fused kernels evaluate it in the
    mcmc, flow-MH and NeuTra launch families (NeuTra on its VALU kernels, conditioners of at most 32 units); every other
    family runs on the split or composed path (`fused_in`).  It is never inferred from a plain callable: pass the object
    as the target."""

    neutra_matrix_cores = False
    SYMMETRY_RTOL = 1e-6

    def __init__(self, mu, covariance=None, precision=None, event_shape=None):
        if (covariance is None) == (precision is None):
            raise ValueError('give exactly one of covariance / precision')
        name = 'covariance' if covariance is not None else 'precision'
        m = torch.as_tensor(covariance if covariance is not None else precision).detach().to('cpu', torch.float64)
        if m.dim() != 2 or m.shape[0] != m.shape[1] or m.shape[0] < 1:
            raise ValueError('%s must be a square (d, d) matrix with d >= 1, got shape %s' % (name, tuple(m.shape)))
        d = int(m.shape[0])
        if not bool(torch.isfinite(m).all()):
            raise ValueError('%s must be finite' % name)
        scale = float(m.abs().max())
        if float((m - m.t()).abs().max()) > self.SYMMETRY_RTOL * scale:
            raise ValueError('%s must be symmetric (to a relative %g of its largest entry)' % (name, self.SYMMETRY_RTOL))
        m = 0.5 * (m + m.t())
        chol, info = torch.linalg.cholesky_ex(m)
        if int(info) != 0:
            raise ValueError('%s must be positive definite (its Cholesky factorisation fails)' % name)
        mu = torch.as_tensor(mu).detach().to('cpu', torch.float64).reshape(-1)
        if mu.numel() != d:
            raise ValueError('mu must have d = %d entries, got %d' % (d, mu.numel()))
        if not bool(torch.isfinite(mu).all()):
            raise ValueError('mu must be finite')
        if event_shape is None:
            event_shape = (d,)
        elif isinstance(event_shape, int):
            event_shape = (event_shape,)
        self.event_shape = tuple(int(v) for v in event_shape)
        if self.event_size != d:
            raise ValueError('event_shape %s must have d = %d elements' % (self.event_shape, d))
        if covariance is not None:
            lam = torch.cholesky_inverse(chol)
            lam = 0.5 * (lam + lam.t())
        else:
            lam = m
        if not bool(torch.isfinite(lam).all()) or not bool(torch.isfinite(lam.float()).all()):
            raise ValueError('the precision matrix must be finite in fp32 too (the kernels read an fp32 copy)')
        self.dim = d
        self.mean = mu.contiguous()          # fp64 masters; the kernels get fp32
        self.precision = lam.contiguous()
        self._dev = {}

    def fused_in(self, family: str) -> bool:
        return super().fused_in(family) and family in ('mcmc', 'flow_mh', 'neutra')

    def _copy(self, device):
        """The fp32 (Lambda, mu) of `device`, made once per device (every shard of a sharded run gets its own)."""
        key = str(device)
        if key not in self._dev:
            self._dev[key] = (self.precision.float().to(device).contiguous(), self.mean.float().to(device).contiguous())
        return self._dev[key]

    def __call__(self, x):
        n = x.shape[0]
        xf = x.reshape(n, -1)
        if xf.dtype == torch.float32 and xf.is_cuda:
            lam, mu = self._copy(xf.device)
        else:
            lam, mu = self.precision.to(xf), self.mean.to(xf)
        r = xf - mu
        return 0.5 * torch.sum((r @ lam) * r, dim=1)

    def descriptor(self, device):
        lam, mu = self._copy(device)
        return hip.NfmcPotential(hip.POT_GAUSSIAN_FULL, self.dim, hip.ptr(lam), hip.ptr(mu), 0.0, 0.0)


class Rosenbrock(Potential):
    """Blocked (hybrid) Rosenbrock, the banana-shaped curved target.  The d coordinates of `event_shape`, flattened
    row-major, split into consecutive blocks of `block` coordinates (the last one may be shorter); coordinate c is a
    block head when c % block == 0:

        U(x) = sum_{heads c} a (x_c - mu)^2 + sum_{non-heads c} b (x_c - x_{c-1}^2)^2

    (constants dropped).  Within a block the density factorises: x_head ~ N(mu, 1/(2a)) and x_c | x_{c-1} ~
    N(x_{c-1}^2, 1/(2b)), so the target can be drawn exactly by ancestral sampling.  The defaults are the 2-D case of the
    hybrid Rosenbrock of Pagani, Wiegand and Nadarajah (2022); `block = 1` is a diagonal Gaussian.  Long blocks with a
    wide head (small a) grow doubly exponentially along the block: their later coordinates overflow fp32, and nothing
    guards against it.  Validated in fp64 on the host: a and b finite and > 0, mu finite, all three finite (a and b
    nonzero) in fp32; `block` an int in 1 .. d.  The fused kernels evaluate it in the mcmc, flow-MH and NeuTra launch
    families (NeuTra on its VALU kernels, conditioners of at most 32 units); every other family runs on the split or
    composed path (`fused_in`).  It is never inferred from a plain callable: pass the object as the target."""

    neutra_matrix_cores = False

    def __init__(self, event_shape, mu=1.0, a=0.05, b=5.0, block=2):
        if event_shape is None:
            raise ValueError('event_shape must be given')
        if isinstance(event_shape, int):
            event_shape = (event_shape,)
        self.event_shape = tuple(int(v) for v in event_shape)
        d = self.event_size
        if d < 1:
            raise ValueError('event_shape %s must have at least one element' % (self.event_shape,))
        vals = {}
        for name, v in (('mu', mu), ('a', a), ('b', b)):
            if isinstance(v, bool) or not isinstance(v, (int, float)) and not (torch.is_tensor(v) and v.numel() == 1):
                raise ValueError('%s must be a real scalar' % name)
            v = float(v)
            if not math.isfinite(v) or not math.isfinite(float(torch.tensor(v, dtype=torch.float32))):
                raise ValueError('%s must be finite in fp32 (the kernels read an fp32 copy), got %r' % (name, v))
            if name != 'mu' and not (v > 0.0 and float(torch.tensor(v, dtype=torch.float32)) > 0.0):
                raise ValueError('%s must be > 0 in fp32, got %r' % (name, v))
            vals[name] = v
        if isinstance(block, bool) or not isinstance(block, int):
            raise ValueError('block must be an int, got %r' % (block,))
        if not 1 <= block <= d:
            raise ValueError('block must lie in 1 .. d = %d, got %d' % (d, block))
        self.dim = d
        self.mu, self.a, self.b = vals['mu'], vals['a'], vals['b']   # fp64 masters; the kernels get fp32
        self.block = int(block)
        self._dev = {}

    def fused_in(self, family: str) -> bool:
        return super().fused_in(family) and family in ('mcmc', 'flow_mh', 'neutra')

    def _tables(self, device, dtype):
        """(head mask (d,), weights a / b (d,), mu (1,)) of `device` in `dtype`, made once per (device, dtype)"""
        key = (str(device), dtype)
        if key not in self._dev:
            head = torch.arange(self.dim, device=device) % self.block == 0
            w = torch.where(head, torch.tensor(self.a, dtype=torch.float64), torch.tensor(self.b, dtype=torch.float64))
            self._dev[key] = (head, w.to(device, dtype), torch.tensor([self.mu], dtype=dtype, device=device))
        return self._dev[key]

    def __call__(self, x):
        n = x.shape[0]
        xf = x.reshape(n, -1)
        head, w, mu = self._tables(xf.device, xf.dtype)
        prev2 = torch.cat([torch.zeros_like(xf[:, :1]), xf[:, :-1] * xf[:, :-1]], dim=1)   # x_{c-1}^2 (0 for c = 0)
        r = xf - torch.where(head, mu, prev2)
        return torch.sum(w * (r * r), dim=1)

    def descriptor(self, device):
        _, _, mu = self._tables(device, torch.float32)
        return hip.NfmcPotential(hip.POT_ROSENBROCK, self.block, hip.ptr(mu), None, self.a, self.b)


def _positive_fp32(name, v):
    """float(v) of a real scalar that is > 0 and finite in fp64 and in fp32 (the kernels read an fp32 copy)"""
    if isinstance(v, bool) or not isinstance(v, (int, float)) and not (torch.is_tensor(v) and v.numel() == 1):
        raise ValueError('%s must be a real scalar, got %r' % (name, v))
    v = float(v)
    v32 = float(torch.tensor(v, dtype=torch.float32))
    if not (v > 0.0 and math.isfinite(v) and v32 > 0.0 and math.isfinite(v32)):
        raise ValueError('%s must be > 0 and finite in fp32 (the kernels read an fp32 copy), got %r' % (name, v))
    return v


class StochasticVolatility(Potential):
    """The stochastic-volatility model of the Stan User's Guide: a hierarchical latent-variable posterior with data.  For
    returns y_0 .. y_{T-1}:

        mu ~ Cauchy(0, mu_scale),  sigma ~ HalfCauchy(0, sigma_scale),  (phi + 1)/2 ~ Beta(alpha, beta),
        h_0 ~ N(mu, sigma^2 / (1 - phi^2)),  h_t | h_{t-1} ~ N(mu + phi (h_{t-1} - mu), sigma^2),  y_t ~ N(0, e^{h_t})

    with (alpha, beta) = `phi_prior`; the defaults are Stan's (phi uniform).  Sampled on d = T + 3 unconstrained
    coordinates x = (mu, s = log sigma, r = atanh phi, h_0, .., h_{T-1}) (`constrain` / `unconstrain` convert), so U
    includes the Jacobians of s and r.  With w = e^{-2s}, q = 1 - phi^2, delta_0 = h_0 - mu, e_t = h_t - mu - phi (h_{t-1}
    - mu), constants dropped:

        U = log1p((mu/c_mu)^2) + softplus(2(s - log c_sigma)) + (alpha + 1/2) softplus(-2r) + (beta + 1/2) softplus(2r)
          + 1/2 q w delta_0^2 + (T - 1) s + sum_{t>=1} 1/2 w e_t^2 + sum_{t>=0} 1/2 [h_t + y_t^2 e^{-h_t}]

    q is formed as 4 sigmoid(2r) sigmoid(-2r), which stays finite where log(1 - phi^2) would not.  Validated in fp64 on
    the host: y 1-D with T >= 1 entries, finite in fp32 too; mu_scale, sigma_scale, alpha and beta > 0 and finite in fp32.
    The fused kernels evaluate it in the mcmc, flow-MH and NeuTra launch families (NeuTra on its VALU kernels,
    conditioners of at most 32 units) for d up to 1024 (T up to 1021); every other family runs on the split or composed
    path (`fused_in`).  It is never inferred from a plain callable: pass the object as the target."""

    neutra_matrix_cores = False

    def __init__(self, y, mu_scale=10.0, sigma_scale=5.0, phi_prior=(1.0, 1.0)):
        y = y if torch.is_tensor(y) else torch.as_tensor(y, dtype=torch.float64)
        if y.dim() != 1 or y.shape[0] < 1:
            raise ValueError('y must be a 1-D series of T >= 1 returns, got shape %s' % (tuple(y.shape),))
        y = y.detach().to('cpu', torch.float64)
        if not bool(torch.isfinite(y).all()) or not bool(torch.isfinite(y.float()).all()):
            raise ValueError('y must be finite, in fp32 too (the kernels read an fp32 copy)')
        if isinstance(phi_prior, (str, bytes)) or not hasattr(phi_prior, '__len__') or len(phi_prior) != 2:
            raise ValueError('phi_prior must be a pair (alpha, beta), got %r' % (phi_prior,))
        self.mu_scale = _positive_fp32('mu_scale', mu_scale)
        self.sigma_scale = _positive_fp32('sigma_scale', sigma_scale)
        self.alpha = _positive_fp32('phi_prior alpha', phi_prior[0])
        self.beta = _positive_fp32('phi_prior beta', phi_prior[1])
        self.y = y.contiguous()          # fp64 master; the kernels get fp32
        self.T = int(y.shape[0])
        self.event_shape = (self.T + 3,)
        self._dev = {}

    def fused_in(self, family: str) -> bool:
        return super().fused_in(family) and family in ('mcmc', 'flow_mh', 'neutra')

    def _tables(self, device, dtype):
        """(y (T,), y^2 (T,), (alpha, beta) (2,)) of `device` in `dtype`, made once per (device, dtype)"""
        key = (str(device), dtype)
        if key not in self._dev:
            y = self.y.to(device, dtype).contiguous()
            ab = torch.tensor([self.alpha, self.beta], dtype=torch.float64).to(device, dtype).contiguous()
            self._dev[key] = (y, (self.y * self.y).to(device, dtype), ab)
        return self._dev[key]

    def __call__(self, x):
        n = x.shape[0]
        xf = x.reshape(n, -1)
        _, y2, _ = self._tables(xf.device, xf.dtype)
        mu, s, r, h = xf[:, 0], xf[:, 1], xf[:, 2], xf[:, 3:]
        sp = torch.nn.functional.softplus
        w = torch.exp(-2.0 * s)
        phi = torch.tanh(r)
        q = 4.0 * torch.sigmoid(2.0 * r) * torch.sigmoid(-2.0 * r)
        d0 = h[:, 0] - mu
        hc = h - mu[:, None]
        e = hc[:, 1:] - phi[:, None] * hc[:, :-1]
        u = (torch.log1p((mu / self.mu_scale) ** 2) + sp(2.0 * (s - math.log(self.sigma_scale)))
             + (self.alpha + 0.5) * sp(-2.0 * r) + (self.beta + 0.5) * sp(2.0 * r)
             + 0.5 * q * w * d0 * d0 + (self.T - 1) * s)
        return u + 0.5 * w * torch.sum(e * e, dim=1) + 0.5 * torch.sum(h + y2 * torch.exp(-h), dim=1)

    def constrain(self, x):
        """(mu, sigma, phi, h) of unconstrained states x (..., T + 3): sigma = e^s, phi = tanh r, h (..., T)."""
        x = torch.as_tensor(x)
        if x.shape[-1:] != self.event_shape:
            raise ValueError('x must end in the event shape %s, got shape %s' % (self.event_shape, tuple(x.shape)))
        return x[..., 0], torch.exp(x[..., 1]), torch.tanh(x[..., 2]), x[..., 3:]

    def unconstrain(self, mu, sigma, phi, h):
        """The unconstrained state x (..., T + 3) of (mu, sigma > 0, -1 < phi < 1, h (..., T)); the leading shapes
        broadcast.  Inverse of `constrain`."""
        h = torch.as_tensor(h)
        if h.dim() < 1 or h.shape[-1] != self.T:
            raise ValueError('h must end in T = %d entries, got shape %s' % (self.T, tuple(h.shape)))
        dt = h.dtype if h.is_floating_point() else torch.get_default_dtype()
        mu, sigma, phi = (torch.as_tensor(v, dtype=dt, device=h.device) for v in (mu, sigma, phi))
        if not bool((sigma > 0).all()) or not bool((phi.abs() < 1).all()):
            raise ValueError('sigma must be > 0 and phi inside (-1, 1)')
        lead = torch.broadcast_shapes(mu.shape, sigma.shape, phi.shape, h.shape[:-1])
        glob = torch.stack(torch.broadcast_tensors(mu, torch.log(sigma), torch.atanh(phi)), dim=-1)
        return torch.cat([glob.expand(lead + (3,)), h.to(dt).expand(lead + (self.T,))], dim=-1)

    def descriptor(self, device):
        y, _, ab = self._tables(device, torch.float32)
        return hip.NfmcPotential(hip.POT_STOCHASTIC_VOLATILITY, self.T, hip.ptr(y), hip.ptr(ab), self.mu_scale,
                                 self.sigma_scale)


class SparseLogisticRegression(Potential):
    """Sparse logistic regression with a hierarchical shrinkage prior: the German-credit sparse model of the Inference Gym
    and the 51-dimensional benchmark of the NeuTra paper.  A global scale tau and per-coefficient local scales lambda_j
    multiply the weights, with Gamma(a, b) priors (shape a = `scale_shape`, rate b = `scale_rate`):

        tau ~ Gamma(a, b),  lambda_j ~ Gamma(a, b),  w_j ~ N(0, 1),  beta_j = tau lambda_j w_j,
        y_i ~ Bernoulli(sigmoid(z_i)),  z = X beta

    X (N, D), y (N,) of bools or numbers; an intercept is a column of ones in X, shrunk like every other column.  Sampled
    on d = 2 D + 1 unconstrained coordinates: each weight beside its log local scale, the log global scale last,

        x_{2j} = w_j,  x_{2j+1} = l_j = log lambda_j  (j = 0 .. D-1),  x_{2D} = s = log tau

    (`constrain` / `unconstrain` convert).  The order is deliberate: in the kernels' interleaved 4-block register layout
    every register quad of a lane holds 4 consecutive coordinates, so each pair (w_j, l_j) lies in one quad and only s
    crosses lanes.  With r = sigmoid(z) - y and g = X^T r, the Jacobians of the two logs included, constants dropped:

        U = sum_i [softplus(z_i) - y_i z_i] + 1/2 sum_j w_j^2 + sum_j (b e^{l_j} - a l_j) + (b e^s - a s)
        dU/dw_j = e^{s + l_j} g_j + w_j,  dU/dl_j = beta_j g_j + b e^{l_j} - a,  dU/ds = sum_j beta_j g_j + b e^s - a

    Validated in fp64 on the host: X 2-D, finite, finite in fp32 too; y N labels in {0, 1}; a and b > 0 and finite in
    fp32.  Far in the tails e^{s + l_j}, e^{l_j}, e^s or z overflow fp32; the kernels then reject the proposal and count
    its log ratio as non-finite.  The fused kernels evaluate it in the mcmc, flow-MH and NeuTra launch families (NeuTra
    on its VALU kernels, conditioners of at most 32 units) for d up to 1024 (D up to 511); every other family runs on the
    split or composed path (`fused_in`).  It is never inferred from a plain callable: pass the object as the target."""

    neutra_matrix_cores = False   # its d = 2 D + 1 is odd, so it never meets the d = 64 / 128 test; stated all the same

    def __init__(self, X, y, scale_shape=0.5, scale_rate=0.5):
        X = torch.as_tensor(X)
        if X.dim() != 2 or X.shape[0] < 1 or X.shape[1] < 1:
            raise ValueError('X must be 2-D (N, D) with N, D >= 1, got shape %s' % (tuple(X.shape),))
        X = X.detach().to('cpu', torch.float64)
        if not bool(torch.isfinite(X).all()) or not bool(torch.isfinite(X.float()).all()):
            raise ValueError('X must be finite, in fp32 too (the kernels read an fp32 copy)')
        N, D = (int(v) for v in X.shape)
        y = torch.as_tensor(y).detach().to('cpu')
        if y.dim() != 1 or y.shape[0] != N:
            raise ValueError('y must be a vector of N = %d labels, got shape %s' % (N, tuple(y.shape)))
        y = y.to(torch.float64)
        if not bool(((y == 0) | (y == 1)).all()):
            raise ValueError('labels must be 0 or 1')
        self.scale_shape = _positive_fp32('scale_shape', scale_shape)
        self.scale_rate = _positive_fp32('scale_rate', scale_rate)
        self.n_rows, self.n_features = N, D
        self.event_shape = (2 * D + 1,)
        self.X = X.contiguous()          # fp64 masters; the kernels get fp32
        self.y = y.contiguous()
        self._dev = {}

    def fused_in(self, family: str) -> bool:
        return super().fused_in(family) and family in ('mcmc', 'flow_mh', 'neutra')

    def _copy(self, device, dtype=torch.float32):
        """(X, y) of `device` in `dtype`, made once per (device, dtype) (every shard of a sharded run gets its own)."""
        key = (str(device), dtype)
        if key not in self._dev:
            self._dev[key] = (self.X.to(device, dtype).contiguous(), self.y.to(device, dtype).contiguous())
        return self._dev[key]

    def __call__(self, x):
        n = x.shape[0]
        xf = x.reshape(n, -1)
        X, y = self._copy(xf.device, xf.dtype)
        D = self.n_features
        w, l, s = xf[:, 0:2 * D:2], xf[:, 1:2 * D:2], xf[:, 2 * D]
        a, b = self.scale_shape, self.scale_rate
        z = (torch.exp(s[:, None] + l) * w) @ X.t()                                # (n, N)
        data = torch.sum(torch.nn.functional.softplus(z) - y * z, dim=1)
        prior = torch.sum(0.5 * w * w + b * torch.exp(l) - a * l, dim=1) + b * torch.exp(s) - a * s
        return data + prior

    def constrain(self, x):
        """(tau, lam, w, beta) of unconstrained states x (..., 2 D + 1): tau = e^s (...), lam = e^l (..., D), w (..., D),
        beta = tau lam w (..., D)."""
        x = torch.as_tensor(x)
        if x.shape[-1:] != self.event_shape:
            raise ValueError('x must end in the event shape %s, got shape %s' % (self.event_shape, tuple(x.shape)))
        D = self.n_features
        tau, lam, w = torch.exp(x[..., 2 * D]), torch.exp(x[..., 1:2 * D:2]), x[..., 0:2 * D:2]
        return tau, lam, w, tau[..., None] * lam * w

    def unconstrain(self, tau, lam, w):
        """The unconstrained state x (..., 2 D + 1) of (tau > 0, lam > 0 (..., D), w (..., D)); the leading shapes
        broadcast.  Inverse of `constrain`."""
        w = torch.as_tensor(w)
        dt = w.dtype if w.is_floating_point() else torch.get_default_dtype()
        tau, lam, w = (torch.as_tensor(v, dtype=dt, device=w.device) for v in (tau, lam, w))
        D = self.n_features
        if lam.dim() < 1 or lam.shape[-1] != D or w.dim() < 1 or w.shape[-1] != D:
            raise ValueError('lam and w must end in D = %d entries, got shapes %s, %s'
                             % (D, tuple(lam.shape), tuple(w.shape)))
        if not bool((tau > 0).all()) or not bool((lam > 0).all()):
            raise ValueError('tau and lam must be > 0')
        lead = torch.broadcast_shapes(tau.shape, lam.shape[:-1], w.shape[:-1])
        pairs = torch.stack(torch.broadcast_tensors(w, torch.log(lam)), dim=-1).expand(lead + (D, 2))
        return torch.cat([pairs.reshape(lead + (2 * D,)), torch.log(tau).expand(lead)[..., None]], dim=-1)

    def descriptor(self, device):
        X, y = self._copy(device)
        return hip.NfmcPotential(hip.POT_SPARSE_LOGISTIC_REGRESSION, self.n_rows, hip.ptr(X), hip.ptr(y),
                                 self.scale_shape, self.scale_rate)


def _finite_fp32(name, v):
    """float(v) of a real scalar (a Python or numpy number, or a one-element tensor) that is finite in fp64 and in fp32
    (the kernels read an fp32 copy)"""
    if isinstance(v, bool) or not isinstance(v, numbers.Real) and not (torch.is_tensor(v) and v.numel() == 1):
        raise ValueError('%s must be a real scalar, got %r' % (name, v))
    v = float(v)
    if not (math.isfinite(v) and math.isfinite(float(torch.tensor(v, dtype=torch.float32)))):
        raise ValueError('%s must be finite in fp32 (the kernels read an fp32 copy), got %r' % (name, v))
    return v


class LatticePhi4(Potential):
    """The phi^4 scalar field on a lattice: the bimodal target of flow-assisted MCMC.  `shape` is (L,) or (H, W); the
    d = prod(shape) sites are flattened row-major:

        U(x) = sum_c [1/2 m2 x_c^2 + 1/4 lam x_c^4] + 1/2 kappa sum_axes sum_bonds (x_c' - x_c)^2
        dU/dx_c = m2 x_c + lam x_c^3 + kappa sum_{neighbours c'} (x_c - x_c')

    (constants dropped).  `boundary='periodic'`: every site has one forward bond per axis, wrapping round, so an axis of
    length 2 counts its bond twice and an axis of length 1 contributes nothing.  `boundary='zero'`: the field is 0
    outside the lattice, so an axis of length n has n + 1 bonds, both boundary bonds included, and in the gradient a
    missing neighbour reads as 0.  With m2 < 0 and lam > 0 (the broken phase) the whole field sits in one of two wells
    related by x -> -x, at about +-sqrt(-m2 / lam) per site; a local sampler (MALA, HMC) does not cross between them,
    a flow jump does.  `magnetisation(x)`, the mean over the sites, is the order parameter that tells the wells apart.

    The 1-D double well of Gabrie, Rotskoff and Vanden-Eijnden (2022), U = beta sum_i [a/(2 Delta) (phi_{i+1} - phi_i)^2
    + Delta/(4a) (1 - phi_i^2)^2] with phi = 0 at both ends (inverse temperature beta, stiffness a, spacing Delta), is
    this model with kappa = beta a / Delta, lam = beta Delta / a, m2 = -beta Delta / a and boundary='zero', up to the
    constant beta Delta N / (4a).

    Validated in fp64 on the host: 1 or 2 axes of length >= 1; m2, lam and kappa finite in fp32; lam >= 0, kappa >= 0;
    normalisable (lam > 0, or lam == 0 and m2 > 0); `boundary` one of the two strings.  `precision()` is the precision
    matrix of the Gaussian lam = 0 model.  The fused kernels evaluate it in the mcmc, flow-MH and NeuTra launch
    families (NeuTra on its VALU kernels, conditioners of at most 32 units) when the last axis' length is a multiple of
    4 and d <= 1024: every lattice row then starts on a 16-byte register quad.  Every other lattice, and every other
    family, runs on the split or composed path like any callable (`fused_in`).  It is never inferred from a plain
    callable: pass the object as the target."""

    neutra_matrix_cores = False
    BOUNDARIES = ('periodic', 'zero')

    def __init__(self, shape, m2=-1.0, lam=1.0, kappa=1.0, boundary='periodic'):
        if isinstance(shape, bool):
            raise ValueError('shape must be (L,) or (H, W), got %r' % (shape,))
        if isinstance(shape, int):
            shape = (shape,)
        try:
            shape = tuple(shape)
        except TypeError:
            raise ValueError('shape must be (L,) or (H, W), got %r' % (shape,)) from None
        if len(shape) not in (1, 2) or any(isinstance(v, bool) or not isinstance(v, int) or v < 1 for v in shape):
            raise ValueError('shape must be (L,) or (H, W) with integer lengths >= 1, got %r' % (shape,))
        self.m2 = _finite_fp32('m2', m2)
        self.lam = _finite_fp32('lam', lam)
        self.kappa = _finite_fp32('kappa', kappa)
        if self.lam < 0.0 or self.kappa < 0.0:
            raise ValueError('lam and kappa must be >= 0, got lam = %r, kappa = %r' % (self.lam, self.kappa))
        if not (self.lam > 0.0 or self.m2 > 0.0):
            raise ValueError('not normalisable: lam > 0, or lam == 0 and m2 > 0, got m2 = %r, lam = %r' % (self.m2, self.lam))
        if boundary not in self.BOUNDARIES:
            raise ValueError('boundary must be one of %s, got %r' % (', '.join(map(repr, self.BOUNDARIES)), boundary))
        self.event_shape = shape
        self.boundary = boundary
        self.dim = self.event_size
        self._dev = {}

    def fused_in(self, family: str) -> bool:
        return (super().fused_in(family) and family in ('mcmc', 'flow_mh', 'neutra')
                and self.event_shape[-1] % 4 == 0 and self.dim <= 1024)

    def _shifted(self, f, axis, step):
        """f moved by `step` (+1 / -1) sites along lattice axis `axis` (batch axis 0 excluded): wrapped round, or with
        zeros moved in."""
        ax = axis + 1
        if self.boundary == 'periodic':
            return torch.roll(f, step, dims=ax)
        n = f.shape[ax]
        pad = torch.zeros_like(f.narrow(ax, 0, 1))
        return torch.cat([pad, f.narrow(ax, 0, n - 1)] if step > 0 else [f.narrow(ax, 1, n - 1), pad], dim=ax)

    def __call__(self, x):
        n = x.shape[0]
        f = x.reshape((n,) + self.event_shape)
        f2 = f * f
        u = torch.sum((0.5 * self.m2) * f2 + (0.25 * self.lam) * (f2 * f2), dim=tuple(range(1, f.dim())))
        for axis in range(len(self.event_shape)):
            df = self._shifted(f, axis, -1) - f                     # the forward bond of every site
            bonds = torch.sum(df * df, dim=tuple(range(1, f.dim())))
            if self.boundary == 'zero':                             # and the bond into the axis' first site
                first = f.narrow(axis + 1, 0, 1)
                bonds = bonds + torch.sum(first * first, dim=tuple(range(1, f.dim())))
            u = u + (0.5 * self.kappa) * bonds
        return u

    def precision(self):
        """The (d, d) fp64 matrix m2 I + kappa Laplacian: U(x) = 1/2 x^T precision() x when lam = 0."""
        d = self.dim
        eye = torch.eye(d, dtype=torch.float64).reshape((d,) + self.event_shape)
        lap = torch.zeros_like(eye)
        for axis in range(len(self.event_shape)):
            lap = lap + (2.0 * eye - self._shifted(eye, axis, 1) - self._shifted(eye, axis, -1))
        return self.m2 * torch.eye(d, dtype=torch.float64) + self.kappa * lap.reshape(d, d)

    def magnetisation(self, x):
        """The mean of the field over the sites of states x (..., *shape) or (..., d): the order parameter."""
        x = torch.as_tensor(x)
        k = len(self.event_shape)
        if k > 1 and x.shape[-k:] == self.event_shape:
            return x.mean(dim=tuple(range(-k, 0)))
        if x.shape[-1:] != (self.dim,):
            raise ValueError('x must end in the lattice shape %s or in d = %d, got shape %s'
                             % (self.event_shape, self.dim, tuple(x.shape)))
        return x.mean(dim=-1)

    def descriptor(self, device):
        key = str(device)
        if key not in self._dev:
            # one row with the zero boundary on both axes, shape (1, W): the kernels' 1-D lattice with the two vertical
            # boundary bonds of every site, 1/2 kappa 2 x^2, folded into the mass term
            fold = self.boundary == 'zero' and len(self.event_shape) == 2 and self.event_shape[0] == 1
            m2 = _finite_fp32('m2 + 2 kappa', self.m2 + 2.0 * self.kappa) if fold else self.m2
            self._dev[key] = torch.tensor([m2, self.lam, self.kappa, float(self.BOUNDARIES.index(self.boundary))],
                                          dtype=torch.float64).to(device, torch.float32).contiguous()
        return hip.NfmcPotential(hip.POT_LATTICE_PHI4, self.event_shape[-1], hip.ptr(self._dev[key]), None, 0.0, 0.0)


class ItemResponseTheory(Potential):
    """The one-parameter item-response-theory model (the Inference Gym's `SyntheticItemResponseTheory`): a hierarchical
    posterior with crossed random effects.  S students answer Q questions; `responses` (S, Q) holds 1 for a correct and 0
    for a wrong answer (numbers or bools, NaN = missing), `observed` is an optional (S, Q) bool mask, and a pair is used
    when it is observed and not NaN:

        mu ~ N(m0, sigma_mu^2),  alpha_s ~ N(0, sigma_a^2),  beta_q ~ N(0, sigma_b^2),
        y_sq ~ Bernoulli(sigmoid(l_sq)),  l_sq = mu + alpha_s - beta_q

    with (m0, sigma_mu) = `mean_ability_prior`, sigma_a = `ability_scale`, sigma_b = `difficulty_scale`; the defaults are
    the Inference Gym's.  Sampled on d = S + Q + 1 coordinates x = [alpha (S) | beta (Q) | mu] (`unpack` / `pack`
    convert).  With precisions p = 1 / sigma^2 and r_sq = sigmoid(l_sq) - y_sq over the used pairs, constants dropped:

        U = 1/2 p_mu (mu - m0)^2 + 1/2 p_a sum_s alpha_s^2 + 1/2 p_b sum_q beta_q^2 + sum_sq [softplus(l_sq) - y_sq l_sq]
        dU/dalpha_s = p_a alpha_s + sum_q r_sq,  dU/dbeta_q = p_b beta_q - sum_s r_sq,  dU/dmu = p_mu (mu - m0) + sum r_sq

    Validated in fp64 on the host: responses 2-D with S, Q >= 1 and 0 or 1 wherever used; the three scales > 0 and
    finite in fp32, their precisions too; m0 finite in fp32.  `synthetic` draws a data set from the model.  The fused
    kernels evaluate it in the mcmc, flow-MH and NeuTra launch families (NeuTra on its VALU kernels, conditioners of at
    most 32 units) for d up to 1024, with no cap on S Q; every other family runs on the split or composed path
    (`fused_in`).  It is never inferred from a plain callable: pass the object as the target."""

    neutra_matrix_cores = False

    def __init__(self, responses, observed=None, mean_ability_prior=(0.75, 1.0), ability_scale=1.0, difficulty_scale=1.0):
        R = torch.as_tensor(responses)
        if R.dim() != 2 or R.shape[0] < 1 or R.shape[1] < 1:
            raise ValueError('responses must be 2-D (S, Q) with S, Q >= 1, got shape %s' % (tuple(R.shape),))
        R = R.detach().to('cpu', torch.float64)
        used = ~torch.isnan(R)
        if observed is not None:
            ob = torch.as_tensor(observed).detach().to('cpu')
            if ob.dtype != torch.bool or ob.shape != R.shape:
                raise ValueError('observed must be a bool mask of shape %s, got %s of shape %s'
                                 % (tuple(R.shape), ob.dtype, tuple(ob.shape)))
            used = used & ob
        if not bool(((R == 0) | (R == 1) | ~used).all()):
            raise ValueError('responses must be 0 or 1 wherever they are observed')
        if (isinstance(mean_ability_prior, (str, bytes)) or not hasattr(mean_ability_prior, '__len__')
                or len(mean_ability_prior) != 2):
            raise ValueError('mean_ability_prior must be a pair (mean, scale), got %r' % (mean_ability_prior,))
        self.mean_ability_mean = _finite_fp32('mean_ability_prior mean', mean_ability_prior[0])
        self.mean_ability_scale = _positive_fp32('mean_ability_prior scale', mean_ability_prior[1])
        self.ability_scale = _positive_fp32('ability_scale', ability_scale)
        self.difficulty_scale = _positive_fp32('difficulty_scale', difficulty_scale)
        # the kernels read the precisions, so they too must be positive and finite in fp32
        self.p_mu = _positive_fp32('1 / mean_ability_prior scale^2', self.mean_ability_scale ** -2)
        self.p_a = _positive_fp32('1 / ability_scale^2', self.ability_scale ** -2)
        self.p_b = _positive_fp32('1 / difficulty_scale^2', self.difficulty_scale ** -2)
        self.n_students, self.n_questions = (int(v) for v in R.shape)
        self.event_shape = (self.n_students + self.n_questions + 1,)
        self.observed = used.contiguous()
        self.responses = torch.where(used, R, torch.zeros_like(R)).contiguous()   # fp64 master, 0 where unused
        self._dev = {}

    @classmethod
    def synthetic(cls, n_students, n_questions, seed, missing=0.25, **prior):
        """(potential, truth): (mu, alpha, beta) drawn from the prior given by `prior` (the constructor's keywords), the
        responses from the model, every pair dropped with probability `missing`; all draws in fp64 from one CPU
        torch.Generator seeded with `seed`.  `truth` is the packed generating state (d,), fp64."""
        S, Q = int(n_students), int(n_questions)
        if S < 1 or Q < 1 or not 0.0 <= float(missing) <= 1.0:
            raise ValueError('n_students, n_questions >= 1 and 0 <= missing <= 1, got %r, %r, %r' % (n_students, n_questions, missing))
        proto = cls(torch.zeros(1, 1), **prior)   # validates the prior
        g = torch.Generator().manual_seed(int(seed))
        mu = proto.mean_ability_mean + proto.mean_ability_scale * torch.randn((), generator=g, dtype=torch.float64)
        alpha = proto.ability_scale * torch.randn(S, generator=g, dtype=torch.float64)
        beta = proto.difficulty_scale * torch.randn(Q, generator=g, dtype=torch.float64)
        prob = torch.sigmoid(mu + alpha[:, None] - beta[None, :])
        R = (torch.rand(S, Q, generator=g, dtype=torch.float64) < prob).to(torch.float64)
        observed = torch.rand(S, Q, generator=g, dtype=torch.float64) >= float(missing)
        pot = cls(R, observed, **prior)
        return pot, pot.pack(mu, alpha, beta)

    def fused_in(self, family: str) -> bool:
        return super().fused_in(family) and family in ('mcmc', 'flow_mh', 'neutra')

    def _copy(self, device, dtype=torch.float32):
        """(responses, mask) of `device` in `dtype`, made once per (device, dtype)."""
        key = (str(device), dtype)
        if key not in self._dev:
            self._dev[key] = (self.responses.to(device, dtype).contiguous(), self.observed.to(device, dtype).contiguous())
        return self._dev[key]

    def __call__(self, x):
        n = x.shape[0]
        xf = x.reshape(n, -1)
        R, M = self._copy(xf.device, xf.dtype)
        S, Q = self.n_students, self.n_questions
        alpha, beta, mu = xf[:, :S], xf[:, S:S + Q], xf[:, S + Q]
        l = mu[:, None, None] + alpha[:, :, None] - beta[:, None, :]               # (n, S, Q)
        # softplus(l) as logaddexp(0, l): exact in every range (torch's softplus is the identity above l = 20), and its
        # derivative is sigmoid(l) everywhere
        data = torch.sum(M * (torch.logaddexp(l.new_zeros(()), l) - R * l), dim=(1, 2))
        dm = mu - self.mean_ability_mean
        return (data + (0.5 * self.p_mu) * dm * dm + (0.5 * self.p_a) * torch.sum(alpha * alpha, dim=1)
                + (0.5 * self.p_b) * torch.sum(beta * beta, dim=1))

    def unpack(self, x):
        """(mean_ability (...), ability (..., S), difficulty (..., Q)) of states x (..., S + Q + 1)."""
        x = torch.as_tensor(x)
        if x.shape[-1:] != self.event_shape:
            raise ValueError('x must end in the event shape %s, got shape %s' % (self.event_shape, tuple(x.shape)))
        S, Q = self.n_students, self.n_questions
        return x[..., S + Q], x[..., :S], x[..., S:S + Q]

    def pack(self, mean_ability, ability, difficulty):
        """The state x (..., S + Q + 1) of (mean_ability (...), ability (..., S), difficulty (..., Q)); the leading
        shapes broadcast.  Inverse of `unpack`."""
        ability = torch.as_tensor(ability)
        dt = ability.dtype if ability.is_floating_point() else torch.get_default_dtype()
        mu, a, b = (torch.as_tensor(v, dtype=dt, device=ability.device) for v in (mean_ability, ability, difficulty))
        S, Q = self.n_students, self.n_questions
        if a.dim() < 1 or a.shape[-1] != S or b.dim() < 1 or b.shape[-1] != Q:
            raise ValueError('ability must end in S = %d and difficulty in Q = %d entries, got shapes %s, %s'
                             % (S, Q, tuple(a.shape), tuple(b.shape)))
        lead = torch.broadcast_shapes(mu.shape, a.shape[:-1], b.shape[:-1])
        return torch.cat([a.expand(lead + (S,)), b.expand(lead + (Q,)), mu.expand(lead)[..., None]], dim=-1)

    def data_block(self):
        """The kernels' view of the responses (NFMC_POT_ITEM_RESPONSE, include/nfmc_hip.h): (Q, SA) fp32 on the CPU,
        SA = 4 ceil(S / 4), entry [q, s] = the response of student s to question q where it is used and -1 where it is
        not and in the padding s >= S."""
        S, Q = self.n_students, self.n_questions
        A = torch.full((Q, 4 * ((S + 3) // 4)), -1.0, dtype=torch.float32)
        A[:, :S] = torch.where(self.observed, self.responses, torch.full_like(self.responses, -1.0)).t().float()
        return A

    def descriptor(self, device):
        key = (str(device), 'descriptor')
        if key not in self._dev:
            par = torch.tensor([self.mean_ability_mean, self.p_mu, self.p_a, self.p_b], dtype=torch.float64)
            self._dev[key] = (self.data_block().to(device).contiguous(), par.to(device, torch.float32).contiguous())
        A, par = self._dev[key]
        return hip.NfmcPotential(hip.POT_ITEM_RESPONSE, self.n_students, hip.ptr(A), hip.ptr(par), 0.0, 0.0)


class VaryingEffectsRegression(Potential):
    """Gaussian regression with group-level (varying) effects: the radon models (varying intercepts, varying slopes,
    both) and eight schools, the textbook funnel between a group-level scale and its group effects.  Observation i has a
    response y_i, an optional covariate x_i and a group g_i in 0 .. C-1 (`group`, integers, no empty group):

        y_i ~ N(a[g_i] + b[g_i] x_i, sigma_i^2)

    `intercepts` is 'varying' (a_c ~ N(mu_a, sigma_a^2), mu_a ~ N(0, m^2), sigma_a ~ HalfNormal(h)) or 'shared' (one
    a ~ N(0, m^2)); `slopes` is 'varying', 'shared' or 'none' (b = 0, x unused); at least one side varies.
    `noise_scale=None` is the unknown noise sigma_i = sigma_y ~ HalfNormal(h); a positive scalar or (N,) array gives known
    scales and no noise coordinate.  m = `location_scale`, h = `scale_scale`.  Scales are sampled as logs s = log sigma,
    Jacobian included.  `centered=True`: the group coordinates are a_c, b_c themselves; `centered=False`: standardised
    t_c ~ N(0, 1) with a_c = mu_a + e^{s_a} t_c (`effects` gives the natural scale in either case).

    Coordinates (`unpack` / `pack` convert): the group block, [a_0, b_0, a_1, b_1, ...] when both sides vary and
    [v_0 .. v_{C-1}] when one does; then the globals that exist, in this order: mu_a, s_a or a; mu_b, s_b or b; s_y.
    d = 2 C + 5 for radon "both", C + 4 for "intercepts" or "slopes", C + 2 for eight schools.

    The likelihood enters through six statistics per group, formed in fp64 with weights omega_i = 1 / sigma_i^2 (1 when
    the noise is unknown): n_c = sum omega, the weighted means xbar_c, ybar_c and the centred weighted sums Sxx_c, Sxy_c,
    Syy_c, so an evaluation costs O(d), not O(N).  With P = 1 / m^2, Hh = 1 / h^2, w_y = e^{-2 s_y} (1 when known) and
    e_c = ybar_c - a_c - b_c xbar_c, constants dropped:

        Q_c = n_c e_c^2 + Syy_c - 2 b_c Sxy_c + b_c^2 Sxx_c
        U = 1/2 w_y sum_c Q_c  [+ N s_y + 1/2 Hh e^{2 s_y} - s_y]
            + per varying side:  centered      C s + 1/2 e^{-2s} sum (v_c - mu)^2 + 1/2 P mu^2 + 1/2 Hh e^{2s} - s
                                 non-centered  1/2 sum t_c^2 + 1/2 P mu^2 + 1/2 Hh e^{2s} - s
            + per shared side:   1/2 P v^2

    Validated in fp64 on the host (ValueError): y, group, x 1-D of equal length N >= 1 and finite; group integers
    0 .. C-1 with no empty group; x required unless slopes='none'; one side varying; noise_scale positive; both scales and
    their inverse squares positive and finite in fp32; the table finite in fp32.  d is not capped: the fused kernels
    evaluate the model in the mcmc, flow-MH and NeuTra launch families (NeuTra on its VALU kernels, conditioners of at
    most 32 units) for d <= 1024, and a larger model, and every other family, runs on the split or composed path like
    any callable (`fused_in`).  It is never inferred from a plain callable: pass the object as the target."""

    neutra_matrix_cores = False
    MODES = {'none': 0, 'shared': 1, 'varying': 2}

    def __init__(self, y, group, x=None, intercepts='varying', slopes='none', noise_scale=None, centered=True,
                 location_scale=10.0, scale_scale=1.0):
        if intercepts not in ('varying', 'shared'):
            raise ValueError("intercepts must be 'varying' or 'shared', got %r" % (intercepts,))
        if slopes not in ('varying', 'shared', 'none'):
            raise ValueError("slopes must be 'varying', 'shared' or 'none', got %r" % (slopes,))
        if intercepts != 'varying' and slopes != 'varying':
            raise ValueError('at least one of intercepts and slopes must be varying')
        if not isinstance(centered, bool):
            raise ValueError('centered must be a bool, got %r' % (centered,))
        yv = torch.as_tensor(y).detach().to('cpu', torch.float64)
        if yv.dim() != 1 or yv.numel() < 1:
            raise ValueError('y must be 1-D with N >= 1 entries, got shape %s' % (tuple(yv.shape),))
        N = yv.numel()
        gv = torch.as_tensor(group).detach().to('cpu')
        if gv.dim() != 1 or gv.numel() != N:
            raise ValueError('group must be 1-D with N = %d entries, got shape %s' % (N, tuple(gv.shape)))
        if gv.dtype == torch.bool or gv.is_complex():
            raise ValueError('group must hold integers, got %s' % gv.dtype)
        if gv.is_floating_point():
            if not bool(torch.isfinite(gv).all()) or not bool((gv == gv.round()).all()):
                raise ValueError('group must hold integers')
        gv = gv.to(torch.int64)
        if int(gv.min()) < 0:
            raise ValueError('group must hold integers 0 .. C-1, got %d' % int(gv.min()))
        C = int(gv.max()) + 1
        counts = torch.bincount(gv, minlength=C)
        if not bool((counts > 0).all()):
            raise ValueError('group must use every label 0 .. C-1 = %d: group %d is empty' % (C - 1, int((counts == 0).nonzero()[0])))
        if slopes == 'none':
            xv = torch.zeros_like(yv)
        else:
            if x is None:
                raise ValueError("x is required unless slopes='none'")
            xv = torch.as_tensor(x).detach().to('cpu', torch.float64)
            if xv.dim() != 1 or xv.numel() != N:
                raise ValueError('x must be 1-D with N = %d entries, got shape %s' % (N, tuple(xv.shape)))
        if not bool(torch.isfinite(yv).all()) or not bool(torch.isfinite(xv).all()):
            raise ValueError('y and x must be finite')
        if noise_scale is None:
            sig = None
            om = torch.ones_like(yv)
        else:
            sig = torch.as_tensor(noise_scale).detach().to('cpu', torch.float64)
            if sig.dim() == 0:
                sig = sig.expand(N)
            if sig.dim() != 1 or sig.numel() != N:
                raise ValueError('noise_scale must be a scalar or have N = %d entries, got shape %s' % (N, tuple(sig.shape)))
            if not bool((torch.isfinite(sig) & (sig > 0)).all()):
                raise ValueError('noise_scale must be > 0 and finite')
            sig = sig.contiguous()
            om = sig ** -2
        self.location_scale = _positive_fp32('location_scale', location_scale)
        self.scale_scale = _positive_fp32('scale_scale', scale_scale)
        self.P = _positive_fp32('1 / location_scale^2', self.location_scale ** -2)
        self.Hh = _positive_fp32('1 / scale_scale^2', self.scale_scale ** -2)
        self.intercepts, self.slopes, self.centered = intercepts, slopes, centered
        self.known_noise = sig is not None
        self.n_groups, self.n_obs = C, N
        self.y, self.x, self.group, self.noise_scale = yv.contiguous(), xv.contiguous(), gv.contiguous(), sig
        # the sufficient statistics, fp64, centred before they are squared
        zero = torch.zeros(C, dtype=torch.float64)
        n = zero.index_add(0, gv, om)
        xb = zero.index_add(0, gv, om * xv) / n
        yb = zero.index_add(0, gv, om * yv) / n
        dx, dy = xv - xb[gv], yv - yb[gv]
        self.stats = torch.stack([n, xb, yb, zero.index_add(0, gv, om * dx * dx), zero.index_add(0, gv, om * dx * dy),
                                  zero.index_add(0, gv, om * dy * dy)], dim=1).contiguous()   # (C, 6)
        if not bool(torch.isfinite(self.stats).all()) or not bool(torch.isfinite(self.stats.float()).all()):
            raise ValueError('the group statistics (n, xbar, ybar, Sxx, Sxy, Syy) must be finite in fp32')
        self.both = intercepts == 'varying' and slopes == 'varying'
        self.group_block = 2 * C if self.both else C
        self.names = ((['mu_a', 's_a'] if intercepts == 'varying' else ['a'])
                      + {'varying': ['mu_b', 's_b'], 'shared': ['b'], 'none': []}[slopes]
                      + ([] if self.known_noise else ['s_y']))
        self.event_shape = (self.group_block + len(self.names),)
        self.code = (self.MODES[intercepts] + 4 * self.MODES[slopes] + 16 * int(self.known_noise)
                     + 32 * int(not centered))
        self._dev = {}

    @classmethod
    def synthetic(cls, n_groups, n_obs, seed, **model):
        """(potential, truth): a data set of `n_obs` observations in `n_groups` groups drawn from the model that `model`
        (the constructor's keywords other than y, group and x) describes; every group gets one observation and the rest
        are assigned at random.  The group-level means are drawn from N(0, 1) and the group-level and noise scales from
        HalfNormal(1) + 0.25, not from the wide priors, so that the data are of order one; x ~ N(0, 1); a known
        `noise_scale` is used as given.  All draws in fp64 from one CPU torch.Generator seeded with `seed`.  `truth` is
        the packed generating state (d,), fp64, in the model's own parameterisation."""
        C, N = int(n_groups), int(n_obs)
        if C < 1 or N < C:
            raise ValueError('n_groups >= 1 and n_obs >= n_groups, got %r, %r' % (n_groups, n_obs))
        g = torch.Generator().manual_seed(int(seed))
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
        group = torch.cat([torch.arange(C), torch.randint(0, C, (N - C,), generator=g)])
        group = group[torch.randperm(N, generator=g)]
        x = rn(N)
        ia, sl = model.get('intercepts', 'varying'), model.get('slopes', 'none')
        parts, eff = {}, {}
        for side, mode in (('a', ia), ('b', sl)):
            if mode == 'varying':
                mu, sg, t = rn(()), rn(()).abs() + 0.25, rn(C)
                parts['mu_' + side], parts['s_' + side], eff[side] = mu, sg.log(), mu + sg * t
                parts[side] = eff[side] if model.get('centered', True) else t
            elif mode == 'shared':
                parts[side] = rn(())
                eff[side] = parts[side].expand(C)
            else:
                eff[side] = torch.zeros(C, dtype=torch.float64)
        ns = model.get('noise_scale')
        if ns is None:
            sy = rn(()).abs() + 0.25
            parts['s_y'] = sy.log()
            sig = sy.expand(N)
        else:
            sig = torch.as_tensor(ns, dtype=torch.float64).expand(N)
        y = eff['a'][group] + eff['b'][group] * x + sig * rn(N)
        pot = cls(y, group, None if sl == 'none' else x, **model)
        return pot, pot.pack(**parts)

    @classmethod
    def eight_schools(cls, **model):
        """Rubin's eight schools: one observation per group with known standard errors, varying intercepts, no slope
        (d = 10: theta_0 .. theta_7, mu, log tau).  `model` may set centered, location_scale and scale_scale."""
        y = [28.0, 8.0, -3.0, 7.0, -1.0, 1.0, 18.0, 12.0]
        sigma = [15.0, 10.0, 16.0, 11.0, 9.0, 11.0, 10.0, 18.0]
        return cls(torch.tensor(y, dtype=torch.float64), torch.arange(8), None, intercepts='varying', slopes='none',
                   noise_scale=torch.tensor(sigma, dtype=torch.float64), **model)

    def fused_in(self, family: str) -> bool:
        return super().fused_in(family) and family in ('mcmc', 'flow_mh', 'neutra') and self.event_size <= 1024

    def unpack(self, x):
        """dict of the parts of states x (..., d) that exist: 'a' (..., C) or (...) and 'b' likewise (the group
        coordinates of a varying side, as sampled; the value of a shared side), 'mu_a', 's_a', 'mu_b', 's_b', 's_y'."""
        x = torch.as_tensor(x)
        if x.shape[-1:] != self.event_shape:
            raise ValueError('x must end in the event shape %s, got shape %s' % (self.event_shape, tuple(x.shape)))
        gb, out = self.group_block, {}
        if self.both:
            out['a'], out['b'] = x[..., 0:gb:2], x[..., 1:gb:2]
        else:
            out['a' if self.intercepts == 'varying' else 'b'] = x[..., :gb]
        for k, name in enumerate(self.names):
            out[name] = x[..., gb + k]
        return out

    def pack(self, **parts):
        """The state x (..., d) of the parts `unpack` names (all of them, and no others); the leading shapes
        broadcast.  Inverse of `unpack`."""
        vary = [s for s, m in (('a', self.intercepts), ('b', self.slopes)) if m == 'varying']
        want = set(vary) | set(self.names)
        if set(parts) != want:
            raise ValueError('pack needs exactly the parts %s, got %s' % (sorted(want), sorted(parts)))
        first = torch.as_tensor(parts[vary[0]])
        dt = first.dtype if first.is_floating_point() else torch.get_default_dtype()
        t = {k: torch.as_tensor(v, dtype=dt, device=first.device) for k, v in parts.items()}
        C = self.n_groups
        for s in vary:
            if t[s].dim() < 1 or t[s].shape[-1] != C:
                raise ValueError('%s must end in C = %d entries, got shape %s' % (s, C, tuple(t[s].shape)))
        lead = torch.broadcast_shapes(*[t[k].shape[:-1] if k in vary else t[k].shape for k in t])
        if self.both:
            blk = torch.stack([t['a'].expand(lead + (C,)), t['b'].expand(lead + (C,))], dim=-1).reshape(lead + (2 * C,))
        else:
            blk = t[vary[0]].expand(lead + (C,))
        return torch.cat([blk] + [t[name].expand(lead)[..., None] for name in self.names], dim=-1)

    def effects(self, x):
        """(a_c, b_c), each (..., C), on the natural scale in either parameterisation (a shared side repeated over the
        groups, b = 0 for slopes='none')."""
        p = self.unpack(x)
        out = []
        for side, mode in (('a', self.intercepts), ('b', self.slopes)):
            if mode == 'varying':
                v = p[side]
                out.append(v if self.centered else p['mu_' + side][..., None] + torch.exp(p['s_' + side])[..., None] * v)
            elif mode == 'shared':
                out.append(p[side][..., None].expand(p[side].shape + (self.n_groups,)))
            else:
                ref = out[0]
                out.append(torch.zeros_like(ref))
        return out[0], out[1]

    def _stats(self, device, dtype):
        key = (str(device), dtype)
        if key not in self._dev:
            self._dev[key] = self.stats.to(device, dtype).contiguous()
        return self._dev[key]

    def __call__(self, x):
        n = x.shape[0]
        xf = x.reshape(n, -1)
        st = self._stats(xf.device, xf.dtype)
        nn, xb, yb, sxx, sxy, syy = (st[:, k] for k in range(6))
        p = self.unpack(xf)
        a, b = self.effects(xf)
        C, P, Hh = self.n_groups, self.P, self.Hh
        e = yb - a - b * xb
        q = torch.sum(nn * e * e + syy - 2.0 * b * sxy + b * b * sxx, dim=1)
        if self.known_noise:
            u = 0.5 * q
        else:
            sy = p['s_y']
            u = 0.5 * torch.exp(-2.0 * sy) * q + self.n_obs * sy + 0.5 * Hh * torch.exp(2.0 * sy) - sy
        for side, mode in (('a', self.intercepts), ('b', self.slopes)):
            if mode == 'varying':
                mu, s, v = p['mu_' + side], p['s_' + side], p[side]
                if self.centered:
                    r = v - mu[:, None]
                    u = u + C * s + 0.5 * torch.exp(-2.0 * s) * torch.sum(r * r, dim=1)
                else:
                    u = u + 0.5 * torch.sum(v * v, dim=1)
                u = u + 0.5 * P * mu * mu + 0.5 * Hh * torch.exp(2.0 * s) - s
            elif mode == 'shared':
                u = u + 0.5 * P * p[side] * p[side]
        return u

    def data_block(self):
        """The kernels' group table (NFMC_POT_VARYING_EFFECTS, include/nfmc_hip.h): (C, 8) fp32 on the CPU, rows
        (n, xbar, ybar, Sxx, Sxy, Syy, 0, 0)."""
        T = torch.zeros(self.n_groups, 8, dtype=torch.float32)
        T[:, :6] = self.stats.float()
        return T

    def descriptor(self, device):
        key = (str(device), 'descriptor')
        if key not in self._dev:
            par = torch.tensor([self.P, self.Hh], dtype=torch.float64)
            self._dev[key] = (self.data_block().to(device).contiguous(), par.to(device, torch.float32).contiguous())
        T, par = self._dev[key]
        return hip.NfmcPotential(hip.POT_VARYING_EFFECTS, self.n_groups, hip.ptr(T), hip.ptr(par), float(self.code),
                                 0.0 if self.known_noise else float(self.n_obs))


class ParticleSystem(Potential):
    """P interacting particles in D = 1, 2 or 3 dimensions in a harmonic trap: the many-particle Boltzmann density of
    Boltzmann generators and of adaptive flow-assisted MCMC, in which every coordinate interacts with every other.
    Coordinates are particle-major, x = [r_0 | r_1 | .. | r_{P-1}], d = P D.  With r_ij = |r_i - r_j| and
    beta = 1 / `temperature`:

        U(x) = beta [ k/2 sum_i |r_i|^2 + sum_{i<j} phi(r_ij) ]                      (constants dropped)
        dU/dr_i = beta [ k r_i + sum_{j != i} (phi'(r_ij) / r_ij) (r_i - r_j) ]

    `pair='lennard_jones'`: phi(r) = epsilon [ (r_min / r)^12 - 2 (r_min / r)^6 ], with its minimum -epsilon at r_min,
    evaluated from r^2 alone.  `pair='double_well'`: phi(r) = a (r - r0) + b (r - r0)^2 + c (r - r0)^4.  Two coincident
    particles: Lennard-Jones gives U = inf (the samplers reject the state and count its log ratio as non-finite); the
    double well contributes phi(0) and zero force.

    Deviation from the benchmark papers: the pair terms are invariant under a common translation of all particles, so
    on R^d the density is improper without a confining term.  Those papers sample the mean-free subspace (centre of
    mass removed) instead; here the trap stiffness k = `trap` must be positive and the centre of mass is a coordinate
    like any other, Gaussian with variance 1 / (beta k P) per dimension.

    Validated in fp64 on the host (ValueError): n_particles an integer >= 2; n_dims in {1, 2, 3}; every parameter finite
    in fp32; trap > 0, temperature > 0, epsilon > 0 and r_min > 0; c > 0 for the double well.  beta is folded into the
    kernels' parameters here, in fp64.  The fused kernels evaluate the model in the mcmc, flow-MH and NeuTra launch
    families (NeuTra on its VALU kernels, conditioners of at most 32 units) for d <= 1024; a larger system, and every
    other family, runs on the split or composed path like any callable (`fused_in`).  It is never inferred from a plain
    callable: pass the object as the target.  The samplers' usual N(0, I) starts put Lennard-Jones particles on top
    of each other: take the initial states from `start_states`."""

    neutra_matrix_cores = False
    PAIRS = ('lennard_jones', 'double_well')
    CHUNK_FLOATS = 1 << 24   # __call__ evaluates at most this many pair-matrix entries (chunk P P D) at once

    def __init__(self, n_particles, n_dims=3, pair='lennard_jones', trap=1.0, temperature=1.0, epsilon=1.0, r_min=1.0,
                 a=0.0, b=-4.0, c=0.9, r0=4.0):
        if isinstance(n_particles, bool) or not isinstance(n_particles, int) or n_particles < 2:
            raise ValueError('n_particles must be an integer >= 2, got %r' % (n_particles,))
        if isinstance(n_dims, bool) or n_dims not in (1, 2, 3):
            raise ValueError('n_dims must be 1, 2 or 3, got %r' % (n_dims,))
        if pair not in self.PAIRS:
            raise ValueError('pair must be one of %s, got %r' % (', '.join(map(repr, self.PAIRS)), pair))
        self.trap = _positive_fp32('trap', trap)
        self.temperature = _positive_fp32('temperature', temperature)
        self.epsilon = _positive_fp32('epsilon', epsilon)
        self.r_min = _positive_fp32('r_min', r_min)
        self.a, self.b, self.r0 = _finite_fp32('a', a), _finite_fp32('b', b), _finite_fp32('r0', r0)
        self.c = _finite_fp32('c', c)
        if pair == 'double_well' and not self.c > 0.0:
            raise ValueError('c must be > 0 for the double well (phi must grow at large r), got %r' % (c,))
        self.n_particles, self.n_dims, self.pair = n_particles, int(n_dims), pair
        self.beta = 1.0 / self.temperature
        self.event_shape = (n_particles * self.n_dims,)
        # the kernels' parameters, beta folded in (fp64 here, one rounding to fp32 in descriptor())
        if pair == 'lennard_jones':
            self.params = (self.beta * self.epsilon, self.r_min * self.r_min, 0.0, 0.0)
        else:
            self.params = (self.beta * self.a, self.beta * self.b, self.beta * self.c, self.r0)
        self.beta_trap = self.beta * self.trap
        for name, v in zip(('beta trap', 'pair parameter 0', 'pair parameter 1', 'pair parameter 2', 'pair parameter 3'),
                           (self.beta_trap,) + self.params):
            _finite_fp32(name, v)
        self._dev = {}

    @classmethod
    def double_well_4(cls, **kw):
        """The double-well system of four particles in the plane (P = 4, D = 2, d = 8): a = 0, b = -4, c = 0.9,
        r0 = 4, temperature 1 -- the pair potential of the Boltzmann-generator papers -- in this build's own trap of
        stiffness k = 1 in place of their centre-of-mass removal.  `kw` overrides any of these."""
        args = dict(n_dims=2, pair='double_well', trap=1.0, temperature=1.0, a=0.0, b=-4.0, c=0.9, r0=4.0)
        args.update(kw)
        return cls(4, **args)

    @classmethod
    def lennard_jones(cls, n_particles, **kw):
        """A Lennard-Jones cluster in space (D = 3; the benchmarks are P = 13 and P = 55, d = 39 and 165): epsilon = 1,
        r_min = 1, temperature 1, in this build's own trap of stiffness k = 1 (the papers remove the centre of mass and
        add a weak oscillator about it).  `kw` overrides any of these."""
        args = dict(n_dims=3, pair='lennard_jones', trap=1.0, temperature=1.0, epsilon=1.0, r_min=1.0)
        args.update(kw)
        return cls(n_particles, **args)

    def fused_in(self, family: str) -> bool:
        return super().fused_in(family) and family in ('mcmc', 'flow_mh', 'neutra') and self.event_size <= 1024

    def jump_tail_ok(self) -> bool:
        """d <= 32 only, the jump-tail layouts with four coordinates per lane: at the layouts with eight the tail kernels
        of this kind need all 256 VGPRs, run one wave per SIMD and measure 1.3 to 1.5 times slower than the same jump on
        the flow-MH kernel."""
        return self.event_size <= 32

    @property
    def spacing(self):
        """The pair potential's length: r_min (Lennard-Jones) or r0 (double well)."""
        return self.r_min if self.pair == 'lennard_jones' else self.r0

    def positions(self, x):
        """States x (..., d) as positions (..., P, D)."""
        x = torch.as_tensor(x)
        if x.shape[-1:] != self.event_shape:
            raise ValueError('x must end in the event shape %s, got shape %s' % (self.event_shape, tuple(x.shape)))
        return x.reshape(x.shape[:-1] + (self.n_particles, self.n_dims))

    def flatten(self, r):
        """Positions r (..., P, D) as states (..., d): the inverse of `positions`."""
        r = torch.as_tensor(r)
        if r.shape[-2:] != (self.n_particles, self.n_dims):
            raise ValueError('r must end in (P, D) = (%d, %d), got shape %s' % (self.n_particles, self.n_dims, tuple(r.shape)))
        return r.reshape(r.shape[:-2] + self.event_shape)

    def pair_distances(self, x):
        """The P (P - 1) / 2 pair distances r_ij, i < j, of states x (n, d), in the order of `torch.pdist`: (n, P (P - 1) / 2).
        Their histogram is the observable the benchmark papers compare."""
        r = self.positions(x)
        i, j = torch.triu_indices(self.n_particles, self.n_particles, 1, device=r.device)
        return (r[..., i, :] - r[..., j, :]).norm(dim=-1)

    def start_states(self, n, seed, jitter=0.05):
        """(n, d) fp64 on the CPU: the particles on the first P sites (row-major) of a simple cubic (square, linear)
        lattice of spacing r_min (or r0) with ceil(P^(1/D)) sites per axis, centred at the origin, plus N(0, jitter^2)
        noise from one CPU torch.Generator seeded with `seed`.  No pair starts closer than the spacing minus a few
        jitters."""
        n = int(n)
        if n < 1 or not (math.isfinite(float(jitter)) and float(jitter) >= 0.0):
            raise ValueError('n >= 1 and jitter >= 0 and finite, got %r, %r' % (n, jitter))
        P, D = self.n_particles, self.n_dims
        m = 1
        while m ** D < P:
            m += 1
        axes = torch.meshgrid(*([torch.arange(m, dtype=torch.float64)] * D), indexing='ij')
        sites = torch.stack([a.reshape(-1) for a in axes], dim=1)[:P] * self.spacing
        sites = sites - sites.mean(dim=0, keepdim=True)
        g = torch.Generator().manual_seed(int(seed))
        noise = torch.randn(n, P, D, generator=g, dtype=torch.float64)
        return self.flatten(sites[None] + float(jitter) * noise)

    def _phi(self, s, on):
        """beta phi at squared distances s where `on`, 0 elsewhere (the diagonal of the pair matrix)."""
        q0, q1, q2, q3 = self.params
        safe = torch.where(on, s, torch.ones_like(s))
        if self.pair == 'lennard_jones':
            t3 = (q1 / safe) ** 3
            e = q0 * t3 * (t3 - 2.0)
        else:
            pos = on & (s > 0)                       # r = 0 off the diagonal: phi(0), and no gradient through sqrt
            r = torch.where(pos, torch.sqrt(torch.where(pos, s, torch.ones_like(s))), torch.zeros_like(s))
            u = r - q3
            u2 = u * u
            e = q0 * u + q1 * u2 + q2 * u2 * u2
        return torch.where(on, e, torch.zeros_like(e))

    def _u_chunk(self, r):
        diff = r[:, :, None, :] - r[:, None, :, :]                 # (m, P, P, D)
        s = (diff * diff).sum(dim=-1)
        on = ~torch.eye(self.n_particles, dtype=torch.bool, device=r.device)
        pair = 0.5 * self._phi(s, on.expand_as(s)).sum(dim=(1, 2))   # every unordered pair twice
        return 0.5 * self.beta_trap * (r * r).sum(dim=(1, 2)) + pair

    def __call__(self, x, chunk=None):
        """U (n,) of states x (n, d) in torch ops.  Evaluated in chunks of chains so that at most CHUNK_FLOATS entries of
        the (chunk, P, P, D) difference tensor exist at once (`chunk` overrides the chunk's number of chains)."""
        n = x.shape[0]
        r = self.positions(x.reshape(n, -1))
        P, D = self.n_particles, self.n_dims
        m = int(chunk) if chunk is not None else max(1, self.CHUNK_FLOATS // (P * P * D))
        if m < 1:
            raise ValueError('chunk must be >= 1, got %r' % (chunk,))
        if m >= n:
            return self._u_chunk(r)
        return torch.cat([self._u_chunk(r[k:k + m]) for k in range(0, n, m)])

    def energy(self, x):
        """U / beta: the trap and pair energy in the units of epsilon (or of a, b, c)."""
        return self(x) * self.temperature

    def data_block(self):
        """The kernels' parameter block (NFMC_POT_PARTICLES, include/nfmc_hip.h): 8 fp32 on the CPU,
        (pair code, D, beta k, four pair parameters, 0)."""
        v = [float(self.PAIRS.index(self.pair)), float(self.n_dims), self.beta_trap] + list(self.params) + [0.0]
        return torch.tensor(v, dtype=torch.float64).to(torch.float32)

    def descriptor(self, device):
        key = str(device)
        if key not in self._dev:
            self._dev[key] = self.data_block().to(device).contiguous()
        return hip.NfmcPotential(hip.POT_PARTICLES, self.n_particles, hip.ptr(self._dev[key]), None, 0.0, 0.0)


def _as_fp64(v):
    """`v` on the CPU in fp64; Python numbers and lists are read as fp64 at once (torch.as_tensor would round them to
    fp32 first)."""
    if isinstance(v, torch.Tensor):
        return v.detach().to('cpu', torch.float64)
    return torch.as_tensor(v, dtype=torch.float64)


class LatentGaussianModel(Potential):
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
    LIKELIHOODS = ('poisson', 'binomial', 'student_t')
    PARAMETERIZATIONS = ('centered', 'whitened')
    SYMMETRY_RTOL = 1e-6
    CHUNK_FLOATS = 1 << 24   # __call__ forms at most this many entries of the (chunk, d) products' inputs at once

    def __init__(self, y, covariance, likelihood='poisson', mean=0.0, weight=None, observed=None,
                 parameterization='whitened', dof=4.0, scale=1.0, event_shape=None):
        if likelihood not in self.LIKELIHOODS:
            raise ValueError('likelihood must be one of %s, got %r' % (', '.join(self.LIKELIHOODS), likelihood))
        if parameterization not in self.PARAMETERIZATIONS:
            raise ValueError('parameterization must be one of %s, got %r'
                             % (', '.join(self.PARAMETERIZATIONS), parameterization))
        K = _as_fp64(covariance)
        if K.dim() != 2 or K.shape[0] != K.shape[1] or K.shape[0] < 1:
            raise ValueError('covariance must be a square (d, d) matrix with d >= 1, got shape %s' % (tuple(K.shape),))
        d = int(K.shape[0])
        if not bool(torch.isfinite(K).all()):
            raise ValueError('covariance must be finite')
        if float((K - K.t()).abs().max()) > self.SYMMETRY_RTOL * float(K.abs().max()):
            raise ValueError('covariance must be symmetric (to a relative %g of its largest entry)' % self.SYMMETRY_RTOL)
        K = 0.5 * (K + K.t())
        chol, info = torch.linalg.cholesky_ex(K)
        if int(info) != 0:
            raise ValueError('covariance must be positive definite (its Cholesky factorisation fails)')
        lam = torch.cholesky_inverse(chol)
        lam = 0.5 * (lam + lam.t())
        for name, v in (('the Cholesky factor of covariance', chol), ('the precision matrix', lam)):
            if not bool(torch.isfinite(v).all()) or not bool(torch.isfinite(v.float()).all()):
                raise ValueError('%s must be finite in fp32 too (the kernels read an fp32 copy)' % name)
        yv = _as_fp64(y).reshape(-1)
        if yv.numel() != d:
            raise ValueError('y must have d = %d entries, got %d' % (d, yv.numel()))
        m = _as_fp64(mean)
        m = m.expand(d).clone() if m.numel() == 1 else m.reshape(-1)
        if m.numel() != d:
            raise ValueError('mean must be a number or have d = %d entries, got %d' % (d, m.numel()))
        w = torch.ones(d, dtype=torch.float64) if weight is None else _as_fp64(weight)
        w = w.expand(d).clone() if w.numel() == 1 else w.reshape(-1)
        if w.numel() != d:
            raise ValueError('weight must be a number or have d = %d entries, got %d' % (d, w.numel()))
        if observed is not None:
            ob = torch.as_tensor(observed).detach().to('cpu').reshape(-1)
            if ob.dtype != torch.bool or ob.numel() != d:
                raise ValueError('observed must be a bool mask of d = %d entries, got %s of %d' % (d, ob.dtype, ob.numel()))
            w = torch.where(ob, w, torch.zeros_like(w))
        if not bool(torch.isfinite(w).all()) or not bool((w >= 0).all()):
            raise ValueError('weight must be finite and >= 0')
        on = w > 0
        yv = torch.where(on, yv, torch.zeros_like(yv))      # an unobserved coordinate's y is never read
        for name, v in (('y', yv), ('mean', m), ('weight', w)):
            if not bool(torch.isfinite(v).all()) or not bool(torch.isfinite(v.float()).all()):
                raise ValueError('%s must be finite (in fp32 too: the kernels read an fp32 copy)' % name)
        if likelihood in ('poisson', 'binomial'):
            if not bool(((yv >= 0) & (yv == yv.round())).all()):
                raise ValueError('the counts y of the %s family must be non-negative integers' % likelihood)
        if likelihood == 'binomial':
            if not bool((w == w.round()).all()):
                raise ValueError('the trials (weight) of the binomial family must be integers')
            if not bool((yv <= w).all()):
                raise ValueError('the binomial family needs 0 <= y <= trials (weight)')
        self.dof = _positive_fp32('dof', dof)
        self.scale = _positive_fp32('scale', scale)
        if likelihood == 'student_t':
            for name, v in (('(dof + 1) / 2', 0.5 * (self.dof + 1.0)), ('1 / (dof scale^2)', 1.0 / (self.dof * self.scale ** 2)),
                            ('dof scale^2', self.dof * self.scale ** 2)):
                _positive_fp32(name, v)
        if event_shape is None:
            event_shape = (d,)
        elif isinstance(event_shape, int):
            event_shape = (event_shape,)
        self.event_shape = tuple(int(v) for v in event_shape)
        if self.event_size != d:
            raise ValueError('event_shape %s must have d = %d elements' % (self.event_shape, d))
        self.dim = d
        self.likelihood = likelihood
        self.parameterization = parameterization
        self.whitened = parameterization == 'whitened'
        self.y = yv.contiguous()               # fp64 masters; the kernels get fp32
        self.weight = w.contiguous()
        self.mean = m.contiguous()
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

    # ------------------------------------------------------------------ routing
    def fused_in(self, family: str) -> bool:
        return super().fused_in(family) and family in ('mcmc', 'flow_mh', 'neutra') and self.dim <= 1024

    # ------------------------------------------------------------------ helpers
    def _flat(self, x):
        x = torch.as_tensor(x)
        k = len(self.event_shape)
        if tuple(x.shape[x.dim() - k:]) == self.event_shape and x.dim() >= k:
            return x.reshape(x.shape[:x.dim() - k] + (self.dim,))
        if x.shape[-1:] == (self.dim,):
            return x
        raise ValueError('the states must end in the event shape %s or in d = %d, got shape %s'
                         % (self.event_shape, self.dim, tuple(x.shape)))

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

    def mean_response(self, x):
        """The Poisson rate w e^f, the success probability sigmoid(f), or the location f, at the coordinates x."""
        f = self.latent(x)
        if self.likelihood == 'poisson':
            return self.weight.to(f) * torch.exp(f)
        if self.likelihood == 'binomial':
            return torch.sigmoid(f)
        return f

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
        if parameterization not in self.PARAMETERIZATIONS:
            raise ValueError('parameterization must be one of %s, got %r'
                             % (', '.join(self.PARAMETERIZATIONS), parameterization))
        return type(self)(self.y, self.covariance, likelihood=self.likelihood, mean=self.mean, weight=self.weight,
                          parameterization=parameterization, dof=self.dof, scale=self.scale, event_shape=self.event_shape)

    def _lik(self, f, y, w, second=False):
        """sum-free l_j(f_j) (..., d) in the dtype of f; with `second` its second derivative instead."""
        on = w > 0
        f = torch.where(on, f, torch.zeros_like(f))   # no 0 * inf in autograd where an unobserved e^f overflows
        if self.likelihood == 'poisson':
            e = w * torch.exp(f)
            out = e if second else e - y * f
        elif self.likelihood == 'binomial':
            if second:
                sg = torch.sigmoid(f)
                out = w * sg * (1.0 - sg)
            else:
                out = w * torch.logaddexp(f.new_zeros(()), f) - y * f
        else:
            t = y - f
            q = t * t
            ns2 = self.dof * self.scale ** 2
            if second:
                out = w * (self.dof + 1.0) * (ns2 - q) / (ns2 + q) ** 2
            else:
                out = w * (0.5 * (self.dof + 1.0)) * torch.log1p(q / ns2)
        return torch.where(on, out, torch.zeros_like(out))

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
        key = (str(device), dtype)
        if key not in self._dev:
            M = self.cholesky.t() if self.whitened else self.precision
            self._dev[key] = tuple(v.to(device, dtype).contiguous() for v in (M, self.mean, self.y, self.weight))
        return self._dev[key]

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
        d, d4 = self.dim, 4 * ((self.dim + 3) // 4)
        if self.whitened:
            A = torch.stack([self.cholesky.t(), self.cholesky]).to(torch.float32).contiguous()
        else:
            A = self.precision.to(torch.float32).contiguous()
        tab = torch.zeros(8 + 3 * d4, dtype=torch.float64)
        if self.likelihood == 'student_t':
            ns2 = self.dof * self.scale ** 2
            tab[:4] = torch.tensor([0.5 * (self.dof + 1.0), 1.0 / ns2, ns2, self.dof + 1.0], dtype=torch.float64)
        for k, v in enumerate((self.mean, self.y, self.weight)):
            tab[8 + k * d4:8 + k * d4 + d] = v
        return A, tab.to(torch.float32)

    def descriptor(self, device):
        key = (str(device), 'descriptor')
        if key not in self._dev:
            A, tab = self.data_block()
            self._dev[key] = (A.to(device).contiguous(), tab.to(device).contiguous())
        A, tab = self._dev[key]
        return hip.NfmcPotential(hip.POT_LATENT_GAUSSIAN, self.dim, hip.ptr(A), hip.ptr(tab), self.code(), 0.0)

class LatentGMRF(Potential):
    """A latent Gaussian Markov random field: n sites whose Gaussian prior has a SPARSE precision tau R (random-walk
    smoothers, ICAR / Besag disease mapping on an adjacency graph, the SPDE-Matern field on a grid) and one of
    LatentGaussianModel's likelihoods on every site ('poisson', 'binomial', 'student_t'; observation y_j, weight
    w_j >= 0, w_j = 0 or `observed[j]` False: not observed).  `structure` is the symmetric, positive semi-definite R
    as a dense (n, n) tensor, a torch sparse tensor or a (rows, cols, values) triple (duplicates are summed); `rank` is
    its rank rho (n unless given).  The prior is x | tau ~ tau^(rho/2) exp(-tau/2 r^T R r), r = x - m.  Three modes,
    q = v^T R v:

        fixed tau   d = n, x = f, v = r; `precision` is folded into R:
                    U = 1/2 q + sum_j l_j(x_j)
        'centered'  `precision_prior=(a, b)`: tau ~ Gamma(a, b) (shape, rate), d = n + 1, x = [f | s], s = log tau, v = r:
                    U = 1/2 e^s q - (rho/2) s + sum_j l_j(x_j) + b e^s - a s
        'scaled'    the same posterior in x = [u | s] with f = m + e^(-s/2) u, v = u, which removes most of the funnel:
                    U = 1/2 q + sum_j l_j(f_j) + b e^s - a s + ((n - rho)/2) s

    (`precision` multiplies R in every mode, so with a prior the field's precision is tau * precision * R.)  Constants
    are dropped and nothing is clamped.  A gradient costs O(W n), W the largest number of stored entries in a row of R,
    where the dense LatentGaussianModel costs O(n^2); `to_dense()` gives that dense counterpart.  Validated in fp64 on the
    host: R finite, symmetric to a relative 1e-6 of its largest entry (then symmetrised), diagonal >= 0; y, w, m, dof and
    scale as in LatentGaussianModel; a > 0 and b > 0.  Positive semi-definiteness is the caller's statement (the presets
    build R = D^T D or a power of a diagonally dominant matrix).  The fused kernels evaluate it in the mcmc, flow-MH
    and NeuTra launch families for d <= 1024 and W <= 32; anything else runs on the split or composed path like any
    callable (`fused_in`).  It is never inferred from a plain callable: pass the object as the target."""

    neutra_matrix_cores = False
    LIKELIHOODS = LatentGaussianModel.LIKELIHOODS
    PARAMETERIZATIONS = ('centered', 'scaled')
    SYMMETRY_RTOL = 1e-6
    MAX_WIDTH = 32           # ELL slots the kernels run (check_gmrf, csrc/pot_kinds.hpp)

    def __init__(self, y, structure, likelihood='poisson', mean=0.0, weight=None, observed=None, precision=1.0,
                 precision_prior=None, parameterization='centered', rank=None, dof=4.0, scale=1.0, event_shape=None):
        if likelihood not in self.LIKELIHOODS:
            raise ValueError('likelihood must be one of %s, got %r' % (', '.join(self.LIKELIHOODS), likelihood))
        if parameterization not in self.PARAMETERIZATIONS:
            raise ValueError('parameterization must be one of %s, got %r'
                             % (', '.join(self.PARAMETERIZATIONS), parameterization))
        if parameterization == 'scaled' and precision_prior is None:
            raise ValueError("parameterization 'scaled' needs precision_prior=(a, b): it rescales the field by tau")
        yv = _as_fp64(y).reshape(-1)
        n = int(yv.numel())
        if n < 1:
            raise ValueError('y must have n >= 1 entries')
        self.precision = _positive_fp32('precision', precision)
        rows, cols, vals = self._coo(structure, n)
        self.n_sites = n
        self.rows, self.cols, self.values = rows, cols, vals * self.precision
        if not bool(torch.isfinite(self.values.float()).all()):
            raise ValueError('precision * structure must be finite in fp32 too (the kernels read an fp32 copy)')
        counts = torch.bincount(rows, minlength=n)
        self.width = max(1, int(counts.max())) if rows.numel() else 1
        if rank is None:
            rank = n
        if isinstance(rank, bool) or not isinstance(rank, numbers.Integral) or not 0 <= int(rank) <= n:
            raise ValueError('rank must be an integer in 0 .. n = %d, got %r' % (n, rank))
        self.rank = int(rank)
        self.tau_unknown = precision_prior is not None
        self.prior_shape = self.prior_rate = 0.0
        if self.tau_unknown:
            try:
                a, b = precision_prior
            except (TypeError, ValueError):
                raise ValueError('precision_prior must be a pair (a, b) = (shape, rate), got %r' % (precision_prior,)) from None
            self.prior_shape = _positive_fp32('the shape a of precision_prior', a)
            self.prior_rate = _positive_fp32('the rate b of precision_prior', b)
        m = _as_fp64(mean)
        m = m.expand(n).clone() if m.numel() == 1 else m.reshape(-1)
        if m.numel() != n:
            raise ValueError('mean must be a number or have n = %d entries, got %d' % (n, m.numel()))
        w = torch.ones(n, dtype=torch.float64) if weight is None else _as_fp64(weight)
        w = w.expand(n).clone() if w.numel() == 1 else w.reshape(-1)
        if w.numel() != n:
            raise ValueError('weight must be a number or have n = %d entries, got %d' % (n, w.numel()))
        if observed is not None:
            ob = torch.as_tensor(observed).detach().to('cpu').reshape(-1)
            if ob.dtype != torch.bool or ob.numel() != n:
                raise ValueError('observed must be a bool mask of n = %d entries, got %s of %d' % (n, ob.dtype, ob.numel()))
            w = torch.where(ob, w, torch.zeros_like(w))
        if not bool(torch.isfinite(w).all()) or not bool((w >= 0).all()):
            raise ValueError('weight must be finite and >= 0')
        yv = torch.where(w > 0, yv, torch.zeros_like(yv))      # an unobserved site's y is never read
        for name, v in (('y', yv), ('mean', m), ('weight', w)):
            if not bool(torch.isfinite(v).all()) or not bool(torch.isfinite(v.float()).all()):
                raise ValueError('%s must be finite (in fp32 too: the kernels read an fp32 copy)' % name)
        if likelihood in ('poisson', 'binomial'):
            if not bool(((yv >= 0) & (yv == yv.round())).all()):
                raise ValueError('the counts y of the %s family must be non-negative integers' % likelihood)
        if likelihood == 'binomial':
            if not bool((w == w.round()).all()):
                raise ValueError('the trials (weight) of the binomial family must be integers')
            if not bool((yv <= w).all()):
                raise ValueError('the binomial family needs 0 <= y <= trials (weight)')
        self.dof = _positive_fp32('dof', dof)
        self.scale = _positive_fp32('scale', scale)
        if likelihood == 'student_t':
            for name, v in (('(dof + 1) / 2', 0.5 * (self.dof + 1.0)), ('1 / (dof scale^2)', 1.0 / (self.dof * self.scale ** 2)),
                            ('dof scale^2', self.dof * self.scale ** 2)):
                _positive_fp32(name, v)
        d = n + 1 if self.tau_unknown else n
        if event_shape is None:
            event_shape = (d,)
        elif isinstance(event_shape, int):
            event_shape = (event_shape,)
        self.event_shape = tuple(int(v) for v in event_shape)
        if self.event_size != d:
            raise ValueError('event_shape %s must have d = %d elements%s'
                             % (self.event_shape, d, ' (n sites and log tau)' if self.tau_unknown else ''))
        self.dim = d
        self.likelihood = likelihood
        self.parameterization = parameterization
        self.scaled = parameterization == 'scaled'
        self.y = yv.contiguous()               # fp64 masters; the kernels get fp32
        self.weight = w.contiguous()
        self.mean = m.contiguous()
        self._ell64 = self._ell()
        self._dev = {}

    # ------------------------------------------------------------------ the structure
    @classmethod
    def _coo(cls, structure, n):
        """(rows, cols, values) of the validated structure: int64, int64, fp64, sorted by row then column, duplicates
        summed, exact zeros dropped, symmetrised."""
        if isinstance(structure, torch.Tensor) and structure.layout != torch.strided:
            sp = structure.detach().to('cpu').to_sparse_coo().coalesce()
            if sp.dim() != 2 or tuple(sp.shape) != (n, n):
                raise ValueError('structure must be (n, n) = (%d, %d), got shape %s' % (n, n, tuple(sp.shape)))
            r, c, v = sp.indices()[0], sp.indices()[1], sp.values().to(torch.float64)
        elif isinstance(structure, (tuple, list)) and len(structure) == 3 and not isinstance(structure[0], numbers.Number):
            r = torch.as_tensor(structure[0]).detach().to('cpu').reshape(-1)
            c = torch.as_tensor(structure[1]).detach().to('cpu').reshape(-1)
            v = _as_fp64(structure[2]).reshape(-1)
            if r.numel() != c.numel() or r.numel() != v.numel():
                raise ValueError('the (rows, cols, values) of structure must have equal lengths, got %d, %d, %d'
                                 % (r.numel(), c.numel(), v.numel()))
            if r.is_floating_point() or c.is_floating_point() or r.dtype == torch.bool or c.dtype == torch.bool:
                raise ValueError('the rows and cols of structure must be integers')
            r, c = r.long(), c.long()
            if r.numel() and (int(r.min()) < 0 or int(c.min()) < 0 or int(r.max()) >= n or int(c.max()) >= n):
                raise ValueError('the rows and cols of structure must lie in 0 .. n - 1 = %d' % (n - 1))
        else:
            R = _as_fp64(structure)
            if R.dim() != 2 or tuple(R.shape) != (n, n):
                raise ValueError('structure must be (n, n) = (%d, %d), got shape %s' % (n, n, tuple(R.shape)))
            if not bool(torch.isfinite(R).all()):
                raise ValueError('structure must be finite')
            r, c = torch.nonzero(R, as_tuple=True)
            v = R[r, c]
        if not bool(torch.isfinite(v).all()):
            raise ValueError('structure must be finite')
        # symmetrise: 1/2 (R + R^T), duplicates summed by the coalesce
        both = torch.sparse_coo_tensor(torch.stack([torch.cat([r, c]), torch.cat([c, r])]), torch.cat([v, v]) * 0.5, (n, n)).coalesce()
        anti = torch.sparse_coo_tensor(torch.stack([torch.cat([r, c]), torch.cat([c, r])]), torch.cat([v, -v]) * 0.5, (n, n)).coalesce()
        big = float(both.values().abs().max()) if both.values().numel() else 0.0
        if anti.values().numel() and float(anti.values().abs().max()) > cls.SYMMETRY_RTOL * big:
            raise ValueError('structure must be symmetric (to a relative %g of its largest entry)' % cls.SYMMETRY_RTOL)
        ri, ci, vi = both.indices()[0], both.indices()[1], both.values()
        keep = vi != 0
        ri, ci, vi = ri[keep], ci[keep], vi[keep]
        if bool((vi[ri == ci] < 0).any()):
            raise ValueError('structure must have a non-negative diagonal (it is positive semi-definite)')
        return ri.contiguous(), ci.contiguous(), vi.contiguous()

    def _ell(self):
        """(values (W, n4) fp64, columns (W, n4) int64): slot-major ELL, a padding slot 0 at its own row."""
        n, n4, W = self.n_sites, 4 * ((self.n_sites + 3) // 4), self.width
        val = torch.zeros(W, n4, dtype=torch.float64)
        col = torch.arange(n4)[None, :].repeat(W, 1)
        if self.rows.numel():
            first = torch.zeros(n + 1, dtype=torch.long)
            first[1:] = torch.cumsum(torch.bincount(self.rows, minlength=n), 0)
            slot = torch.arange(self.rows.numel()) - first[self.rows]     # rows are sorted: position within the row
            val[slot, self.rows] = self.values
            col[slot, self.rows] = self.cols
        return val, col

    def structure_dense(self):
        """precision * R as a dense (n, n) fp64 tensor."""
        R = torch.zeros(self.n_sites, self.n_sites, dtype=torch.float64)
        R[self.rows, self.cols] = self.values
        return R

    # ------------------------------------------------------------------ presets
    @staticmethod
    def _matmul(A, B, inner):
        """The product of two sparse matrices given as (rows, cols, values) triples, B sorted by row with `inner` rows;
        a triple with duplicates (the constructor sums them).  Index arithmetic only: every entry (i, k) of A meets the
        stored entries of row k of B."""
        ra, ca, va = A
        rb, cb, vb = B
        per = torch.bincount(rb, minlength=inner)
        first = torch.cumsum(per, 0) - per
        rep = per[ca]
        ia = torch.arange(ra.numel()).repeat_interleave(rep)
        ib = first[ca[ia]] + torch.arange(int(rep.sum())) - (torch.cumsum(rep, 0) - rep).repeat_interleave(rep)
        return ra[ia], cb[ib], va[ia] * vb[ib]

    @classmethod
    def random_walk(cls, y, order=1, cyclic=False, **model):
        """A random-walk smoother of order 1 (R = D1^T D1, first differences) or 2 (second differences) on the n sites
        of y in their order; `cyclic` closes the walk into a ring.  Rank n - order, or n - 1 when cyclic."""
        n = int(torch.as_tensor(y).numel())
        if order not in (1, 2) or n < order + 1 + (1 if cyclic else 0):
            raise ValueError('order 1 or 2 and more than order%s sites, got order %r, n = %d' % (' + 1' if cyclic else '', order, n))
        stencil = [-1.0, 1.0] if order == 1 else [1.0, -2.0, 1.0]
        k = n if cyclic else n - order
        r = torch.arange(k).repeat_interleave(len(stencil))
        c = (torch.arange(k)[:, None] + torch.arange(len(stencil))[None, :]).reshape(-1) % n
        v = torch.tensor(stencil, dtype=torch.float64).repeat(k)
        args = dict(rank=n - 1 if cyclic else n - order)
        args.update(model)
        return cls(y, cls._matmul((c, r, v), (r, c, v), k), **args)    # D^T D, D (k, n) sorted by row

    @classmethod
    def icar(cls, y, edges, **model):
        """The intrinsic conditional autoregression (Besag) on the undirected graph `edges` ((E, 2) site pairs; self
        loops dropped, duplicates merged): R = D - A, rank n minus the number of connected components."""
        n = int(torch.as_tensor(y).numel())
        e = torch.as_tensor(edges).detach().to('cpu').reshape(-1, 2).long()
        if e.numel() and (int(e.min()) < 0 or int(e.max()) >= n):
            raise ValueError('edges must name sites 0 .. n - 1 = %d' % (n - 1))
        e = e[e[:, 0] != e[:, 1]]
        lo, hi = torch.minimum(e[:, 0], e[:, 1]), torch.maximum(e[:, 0], e[:, 1])
        e = torch.unique(torch.stack([lo, hi], 1), dim=0) if e.numel() else e
        parent = list(range(n))

        def find(i):
            while parent[i] != i:
                parent[i] = parent[parent[i]]
                i = parent[i]
            return i
        for i, j in e.tolist():
            parent[find(i)] = find(j)
        comps = len({find(i) for i in range(n)})
        deg = torch.bincount(e.reshape(-1), minlength=n).double()
        r = torch.cat([e[:, 0], e[:, 1], torch.arange(n)])
        c = torch.cat([e[:, 1], e[:, 0], torch.arange(n)])
        v = torch.cat([-torch.ones(2 * e.shape[0], dtype=torch.float64), deg])
        args = dict(rank=n - comps)
        args.update(model)
        return cls(y, (r, c, v), **args)

    @classmethod
    def lattice(cls, y, kappa2, alpha=1, **model):
        """The SPDE-Matern field on the (H, W) grid of y (Lindgren, Rue and Lindstrom 2011): R = (kappa2 I + G)^alpha, G
        the grid Laplacian with free boundaries (degree minus adjacency of the 4-neighbour graph).  alpha = 1 is a 5-point
        stencil, alpha = 2 the 13-point one.  Proper (rank n) for kappa2 > 0.  event_shape (H, W) when tau is fixed."""
        yt = torch.as_tensor(y)
        if yt.dim() != 2 or alpha not in (1, 2) or not (math.isfinite(float(kappa2)) and float(kappa2) > 0):
            raise ValueError('y must be an (H, W) grid, alpha 1 or 2 and kappa2 > 0, got shape %s, %r, %r'
                             % (tuple(yt.shape), alpha, kappa2))
        H, W = (int(v) for v in yt.shape)
        n = H * W
        site = torch.arange(n).reshape(H, W)
        e = torch.cat([torch.stack([site[:, :-1].reshape(-1), site[:, 1:].reshape(-1)], 1),
                       torch.stack([site[:-1, :].reshape(-1), site[1:, :].reshape(-1)], 1)])
        deg = torch.bincount(e.reshape(-1), minlength=n).double()
        r = torch.cat([e[:, 0], e[:, 1], torch.arange(n)])
        c = torch.cat([e[:, 1], e[:, 0], torch.arange(n)])
        v = torch.cat([-torch.ones(2 * e.shape[0], dtype=torch.float64), deg + float(kappa2)])
        A = torch.sparse_coo_tensor(torch.stack([r, c]), v, (n, n)).coalesce()
        trip = (A.indices()[0], A.indices()[1], A.values())
        if alpha == 2:
            trip = cls._matmul(trip, trip, n)
        args = dict(rank=n)
        if model.get('precision_prior') is None:
            args['event_shape'] = (H, W)
        args.update(model)
        return cls(yt.reshape(-1), trip, **args)

    @classmethod
    def log_gaussian_cox(cls, counts, range_cells, variance=1.0, mean=None, **model):
        """The log-Gaussian Cox process on an (H, W) grid of unit cells with the alpha = 2 SPDE-Matern field (smoothness
        1) of correlation range `range_cells` (in cells) and marginal variance `variance`: kappa = sqrt(8) / range,
        tau = 1 / (4 pi kappa^2 variance), R = (kappa^2 I + G)^2, Poisson counts with exposure 1 per cell, prior mean
        log(mean count) - variance / 2 unless given.  The variance is that of the stationary field on the infinite grid in
        the continuum limit: APPROXIMATE, and near the free boundary the marginal variance is larger (about twice at an
        edge, for a range of a few cells)."""
        c = _as_fp64(torch.as_tensor(counts))
        rg, var = float(range_cells), float(variance)
        if c.dim() != 2 or not (math.isfinite(rg) and rg > 0 and math.isfinite(var) and var > 0):
            raise ValueError('counts must be an (H, W) grid, range_cells > 0 and variance > 0, got shape %s, %r, %r'
                             % (tuple(c.shape), range_cells, variance))
        kappa2 = 8.0 / (rg * rg)
        if mean is None:
            mean = math.log(max(float(c.mean()), 1e-3)) - 0.5 * var
        args = dict(likelihood='poisson', mean=mean, weight=1.0, precision=1.0 / (4.0 * math.pi * kappa2 * var))
        args.update(model)
        return cls.lattice(c, kappa2, alpha=2, **args)

    @classmethod
    def synthetic(cls, n, structure, likelihood, seed, **model):
        """(potential, truth): a seeded problem on n sites.  `structure`: 'rw1', 'rw2' (random walks), 'ring' (the ring's
        Laplacian + 0.5 I, proper) or an explicit structure.  The field is drawn from N(m, (R + I)^-1) (the ridge makes
        an intrinsic R proper and keeps its smooth directions of order 1), tau* = 1, the observations from the
        likelihood at the field as in LatentGaussianModel.synthetic; all draws in fp64 from one CPU torch.Generator
        seeded with `seed`.  `model`: the constructor's keywords.  `truth` is the
        generating state in the object's own coordinates (d,), fp64."""
        n = int(n)
        if n < 1 or likelihood not in cls.LIKELIHOODS:
            raise ValueError('n >= 1 and a likelihood of %s, got %r, %r' % (', '.join(cls.LIKELIHOODS), n, likelihood))
        zeros = torch.zeros(n)
        if isinstance(structure, str):
            if structure in ('rw1', 'rw2'):
                def make(y):
                    return cls.random_walk(y, order=int(structure[2]), likelihood=likelihood, **model)
            elif structure == 'ring':
                j = torch.arange(n)
                e = torch.stack([j, (j + 1) % n], 1)
                ic = cls.icar(zeros, e)
                trip = (torch.cat([ic.rows, j]), torch.cat([ic.cols, j]), torch.cat([ic.values, torch.full((n,), 0.5, dtype=torch.float64)]))

                def make(y):
                    return cls(y, trip, likelihood=likelihood, **model)
            else:
                raise ValueError("structure must be 'rw1', 'rw2', 'ring' or an explicit structure, got %r" % (structure,))
        else:
            def make(y):
                return cls(y, structure, likelihood=likelihood, **model)
        proto = make(zeros)
        g = torch.Generator().manual_seed(int(seed))
        chol = torch.linalg.cholesky(proto.structure_dense() + torch.eye(n, dtype=torch.float64))
        eps = torch.randn(n, generator=g, dtype=torch.float64)
        f = proto.mean + torch.linalg.solve_triangular(chol.t(), eps[:, None], upper=True)[:, 0]
        w = proto.weight
        if likelihood == 'poisson':
            y = torch.poisson(w * torch.exp(f), generator=g)
        elif likelihood == 'binomial':
            trials = max(int(w.max()), 1)
            draws = torch.rand(trials, n, generator=g, dtype=torch.float64) < torch.sigmoid(f)
            y = (draws & (torch.arange(trials)[:, None] < w[None, :])).sum(0).to(torch.float64)
        else:
            chi2 = 2.0 * torch._standard_gamma(torch.full((n,), 0.5 * proto.dof, dtype=torch.float64), generator=g)
            y = f + proto.scale * torch.randn(n, generator=g, dtype=torch.float64) / torch.sqrt(chi2 / proto.dof)
        pot = make(y)
        return pot, pot.coordinates(f, tau=1.0 if pot.tau_unknown else None)

    # ------------------------------------------------------------------ routing
    def fused_in(self, family: str) -> bool:
        return (super().fused_in(family) and family in ('mcmc', 'flow_mh', 'neutra') and self.dim <= 1024
                and self.width <= self.MAX_WIDTH)

    # ------------------------------------------------------------------ helpers
    def _flat(self, x):
        x = torch.as_tensor(x)
        k = len(self.event_shape)
        if x.dim() >= k and tuple(x.shape[x.dim() - k:]) == self.event_shape:
            return x.reshape(x.shape[:x.dim() - k] + (self.dim,))
        if x.shape[-1:] == (self.dim,):
            return x
        raise ValueError('the states must end in the event shape %s or in d = %d, got shape %s'
                         % (self.event_shape, self.dim, tuple(x.shape)))

    def latent(self, x):
        """The field f (..., n) of the coordinates x: the first n coordinates, or m + e^(-s/2) u when scaled."""
        xf = self._flat(x)
        n = self.n_sites
        if not self.scaled:
            return xf[..., :n]
        return self.mean.to(xf) + torch.exp(-0.5 * xf[..., n:]) * xf[..., :n]

    def precision_of(self, x):
        """The field's precision multiplier (...,): `precision` when it is fixed, precision e^s when tau is a coordinate."""
        xf = self._flat(x)
        if not self.tau_unknown:
            return torch.full(xf.shape[:-1], self.precision, dtype=xf.dtype, device=xf.device)
        return self.precision * torch.exp(xf[..., self.n_sites])

    def coordinates(self, f, tau=None):
        """The coordinates x (..., d) of a field f (..., n) (or event-shaped when tau is fixed): f itself when tau is
        fixed; [f | log tau] when centred; [(f - m) sqrt(tau) | log tau] when scaled.  `tau` (a number or (...,); 1 unless
        given) is the coordinate e^s, without the factor `precision`."""
        ff = torch.as_tensor(f)
        if not self.tau_unknown:
            if tau is not None:
                raise ValueError('tau is fixed (no precision_prior): coordinates takes no tau')
            return self._flat(ff)
        if ff.shape[-1:] != (self.n_sites,):
            raise ValueError('the field must end in n = %d, got shape %s' % (self.n_sites, tuple(ff.shape)))
        t = torch.as_tensor(1.0 if tau is None else tau).to(ff).expand(ff.shape[:-1])[..., None]
        if not bool((t > 0).all()):
            raise ValueError('tau must be positive')
        head = (ff - self.mean.to(ff)) * torch.sqrt(t) if self.scaled else ff
        return torch.cat([head, torch.log(t)], dim=-1)

    def mean_response(self, x):
        """The Poisson rate w e^f, the success probability sigmoid(f), or the location f, at the coordinates x."""
        f = self.latent(x)
        if self.likelihood == 'poisson':
            return self.weight.to(f) * torch.exp(f)
        if self.likelihood == 'binomial':
            return torch.sigmoid(f)
        return f

    def _model(self):
        return dict(likelihood=self.likelihood, mean=self.mean, weight=self.weight, rank=self.rank, dof=self.dof,
                    scale=self.scale, precision_prior=(self.prior_shape, self.prior_rate) if self.tau_unknown else None)

    def reparameterized(self, parameterization):
        """The same data, prior and hyperprior in the form `parameterization` ('centered' / 'scaled'; tau must be
        unknown for 'scaled'): U_scaled(u, s) = U_centred(m + e^(-s/2) u, s) + (n/2) s, the log Jacobian."""
        if parameterization not in self.PARAMETERIZATIONS:
            raise ValueError('parameterization must be one of %s, got %r'
                             % (', '.join(self.PARAMETERIZATIONS), parameterization))
        return type(self)(self.y, (self.rows, self.cols, self.values), parameterization=parameterization,
                          event_shape=self.event_shape, **self._model())

    def to_dense(self):
        """The equivalent centred LatentGaussianModel (covariance (precision R)^-1) of a proper R with fixed tau: the
        same U up to a constant, evaluated with the dense d x d matrix."""
        if self.tau_unknown:
            raise ValueError('to_dense() needs a fixed tau: LatentGaussianModel has no hyperparameter')
        R = self.structure_dense()
        chol, info = torch.linalg.cholesky_ex(R)
        if int(info) != 0:
            raise ValueError('to_dense() needs a proper (positive definite) structure; this one is intrinsic')
        K = torch.cholesky_inverse(chol)
        return LatentGaussianModel(self.y, 0.5 * (K + K.t()), likelihood=self.likelihood, mean=self.mean, weight=self.weight,
                                   parameterization='centered', dof=self.dof, scale=self.scale, event_shape=self.event_shape)

    _lik = LatentGaussianModel._lik

    def _apply(self, v, val, col):
        """R v (..., n) of v (..., n) through the ELL slots: W gathers, no dense matrix."""
        n = self.n_sites
        out = torch.zeros_like(v)
        for k in range(self.width):
            out = out + val[k, :n] * v.index_select(-1, col[k, :n])
        return out

    def hessian_bound(self, x):
        """An UPPER bound on lambda_max of the Hessian of U at the state x (d,) (or event-shaped), in fp64, by
        Gershgorin's circles: for a site the absolute row sum of tau R plus the likelihood's curvature (e^(-s) l'' when
        scaled) plus the absolute coupling to s; for s its own second derivative plus the absolute couplings.  For
        step sizes: MALA h ~ d^(-1/3) / bound, HMC h ~ d^(-1/4) / sqrt(bound)."""
        xf = self._flat(torch.as_tensor(x).detach().to('cpu', torch.float64)).reshape(self.dim)
        n = self.n_sites
        val, col = self._ell64
        rowsum = val[:, :n].abs().sum(0)
        f = self.latent(xf)
        l2 = self._lik(f, self.y, self.weight, second=True)
        if not self.tau_unknown:
            return float((rowsum + l2).max())
        s = xf[n]
        es, b = torch.exp(s), self.prior_rate
        if not self.scaled:
            r = xf[:n] - self.mean
            Rr = self._apply(r, val, col)
            cross = es * Rr.abs()
            sites = es * rowsum + l2 + cross
            srow = 0.5 * es * (r * Rr).sum() + b * es + cross.sum()
        else:
            u, eh = xf[:n], torch.exp(-0.5 * s)
            t = f.detach().requires_grad_(True)
            (l1,) = torch.autograd.grad(self._lik(t, self.y, self.weight).sum(), t)
            cross = (0.5 * eh * (l1 + l2 * eh * u)).abs()
            sites = rowsum + eh * eh * l2 + cross
            srow = 0.25 * eh * (u * l1).sum() + 0.25 * eh * eh * (u * u * l2).sum() + b * es + cross.sum()
        return float(torch.maximum(sites.max(), srow))

    # ------------------------------------------------------------------ evaluation in torch ops
    def _copy(self, device, dtype=torch.float32):
        key = (str(device), dtype)
        if key not in self._dev:
            val, col = self._ell64
            self._dev[key] = (val.to(device, dtype).contiguous(), col.to(device).contiguous()) + tuple(
                v.to(device, dtype).contiguous() for v in (self.mean, self.y, self.weight))
        return self._dev[key]

    def __call__(self, x):
        """U (n_chains,) of states x (n_chains, ...) in differentiable torch ops; R v through W gathers."""
        xf = x.reshape(x.shape[0], -1)
        val, col, m, y, w = self._copy(xf.device, xf.dtype)
        n = self.n_sites
        if not self.tau_unknown:
            r = xf - m
            return 0.5 * torch.sum(r * self._apply(r, val, col), dim=1) + torch.sum(self._lik(xf, y, w), dim=1)
        s = xf[:, n]
        es, a, b = torch.exp(s), self.prior_shape, self.prior_rate
        if not self.scaled:
            f = xf[:, :n]
            r = f - m
            q = torch.sum(r * self._apply(r, val, col), dim=1)
            return 0.5 * es * q - (0.5 * self.rank + a) * s + torch.sum(self._lik(f, y, w), dim=1) + b * es
        u = xf[:, :n]
        f = m + torch.exp(-0.5 * s)[:, None] * u
        q = torch.sum(u * self._apply(u, val, col), dim=1)
        return 0.5 * q + torch.sum(self._lik(f, y, w), dim=1) + b * es + (0.5 * (n - self.rank) - a) * s

    # ------------------------------------------------------------------ the kernels' view
    def code(self):
        """a_scalar of the descriptor: likelihood code + 4 [tau unknown] + 8 [scaled]."""
        return float(self.LIKELIHOODS.index(self.likelihood) + (4 if self.tau_unknown else 0) + (8 if self.scaled else 0))

    def data_block(self):
        """The kernels' view (NFMC_POT_LATENT_GMRF, include/nfmc_hip.h), fp32 on the CPU: (ELL block, table).  ELL block
        (2, W, n4), n4 = 4 ceil(n / 4): the W slot rows of values, then the W slot rows of column indices as
        integer-valued floats; a padding slot is 0 at its own row.  Table: 8 floats ((nu+1)/2, 1/(nu s^2), nu s^2, nu+1, a,
        b, rho/2, (n - rho)/2), the first four zeros unless Student-t, then the rows m, y, w of n4 floats, zero past n."""
        n, n4 = self.n_sites, 4 * ((self.n_sites + 3) // 4)
        val, col = self._ell64
        block = torch.stack([val, col.to(torch.float64)]).to(torch.float32).contiguous()
        tab = torch.zeros(8 + 3 * n4, dtype=torch.float64)
        if self.likelihood == 'student_t':
            ns2 = self.dof * self.scale ** 2
            tab[:4] = torch.tensor([0.5 * (self.dof + 1.0), 1.0 / ns2, ns2, self.dof + 1.0], dtype=torch.float64)
        tab[4:8] = torch.tensor([self.prior_shape, self.prior_rate, 0.5 * self.rank, 0.5 * (n - self.rank)], dtype=torch.float64)
        for k, v in enumerate((self.mean, self.y, self.weight)):
            tab[8 + k * n4:8 + k * n4 + n] = v
        return block, tab.to(torch.float32)

    def descriptor(self, device):
        key = (str(device), 'descriptor')
        if key not in self._dev:
            block, tab = self.data_block()
            self._dev[key] = (block.to(device).contiguous(), tab.to(device).contiguous())
        block, tab = self._dev[key]
        return hip.NfmcPotential(hip.POT_LATENT_GMRF, self.width, hip.ptr(block), hip.ptr(tab), self.code(), 0.0)


class DiffusionBridge(Potential):
    """The latent path of a stochastic differential equation dX = f(X) dt + sigma dW, discretised by Euler-Maruyama and
    partially observed: T >= 2 time steps, a state X_t in R^m (m = 1, 2 or 3), the step `dt`:

        X_0 ~ N(mu0, s0^2 I),   X_t | X_{t-1} ~ N(X_{t-1} + dt f(X_{t-1}), sigma^2 dt I),   y_{t,c} ~ N(X_{t,c}, tau^2)

    `y` is (T, m) (a (T,) vector is m = 1); a NaN in y, or False in `observed`, marks an entry that is not observed.
    sigma = `innovation_scale`, tau = `observation_scale`, mu0 = `initial_mean`, s0 = `initial_scale`.  With
    `scale_prior=(l, c)` both scales are unknown, p = log sigma and q = log tau with p, q ~ N(l, c^2) (a LogNormal(l, c)
    prior on each; the Inference Gym's is (0, 2)), and `innovation_scale` / `observation_scale` are not used.  The
    coordinates are time-major, x[t m + c] = X_{t,c}, then p and q when the scales are unknown: d = T m or T m + 2.
    With e_t = X_t - X_{t-1} - dt f(X_{t-1}), om = 1 / (sigma^2 dt), rho = 1 / tau^2, S_e = sum_{t>=1} |e_t|^2, S_v the
    sum of (X - y)^2 over the N_o observed entries, constants dropped:

        U = 1/2 |X_0 - mu0|^2 / s0^2 + 1/2 om S_e + 1/2 rho S_v [ + (T-1) m p + N_o q + ((p - l)^2 + (q - l)^2) / (2 c^2) ]

    Drifts (`drift`, parameters `drift_params` as a sequence in the order given, or a dict by name):

        'cubic'            any m, componentwise f_c = alpha x_c - beta x_c^3   (alpha, beta), default (0, 0): Brownian
                           motion; alpha < 0, beta = 0: Ornstein-Uhlenbeck; alpha = beta > 0: the double well
        'fitzhugh_nagumo'  m = 2, f = (x0 - x0^3/3 - x1 + current, epsilon (x0 + a - b x1))
                           (a, b, epsilon, current), default (0.7, 0.8, 0.08, 0.5)
        'lorenz63'         m = 3, f = (s (x1 - x0), x0 (r - x2) - x1, x0 x1 - beta x2)   (s, r, beta), default (10, 28, 8/3)

    This is the centred parameterisation: the states are the coordinates.  (A non-centred one, with the innovations as
    coordinates, needs a sequential pass through time per gradient and is not offered.)  Nothing is clamped.  Validated in
    fp64 on the host: y, the scales, dt and the parameters finite in fp32 too, the scales and dt > 0, T >= 2, m fitting the
    drift.  The fused kernels evaluate it in the mcmc, flow-MH and NeuTra launch families (NeuTra on its VALU kernels,
    conditioners of at most 32 units) for d <= 1024; anything else runs on the split or composed path like any callable
    (`fused_in`).  It is never inferred from a plain callable: pass the object as the target.  N(0, I) starts sit far in
    the tails (U ~ 1e5 for the Lorenz preset): start from `prior_draws`."""

    neutra_matrix_cores = False
    DRIFTS = ('cubic', 'fitzhugh_nagumo', 'lorenz63')
    DRIFT_DIMS = {'cubic': (1, 2, 3), 'fitzhugh_nagumo': (2,), 'lorenz63': (3,)}
    DRIFT_PARAMS = {'cubic': ('alpha', 'beta'), 'fitzhugh_nagumo': ('a', 'b', 'epsilon', 'current'),
                    'lorenz63': ('s', 'r', 'beta')}
    DRIFT_DEFAULTS = {'cubic': (0.0, 0.0), 'fitzhugh_nagumo': (0.7, 0.8, 0.08, 0.5), 'lorenz63': (10.0, 28.0, 8.0 / 3.0)}

    def __init__(self, y, observed=None, drift='lorenz63', drift_params=None, dt=0.02, innovation_scale=0.1,
                 observation_scale=1.0, initial_mean=0.0, initial_scale=1.0, scale_prior=None, event_shape=None):
        if drift not in self.DRIFTS:
            raise ValueError('drift must be one of %s, got %r' % (', '.join(self.DRIFTS), drift))
        yv = _as_fp64(y)
        if yv.dim() == 1:
            yv = yv[:, None]
        if yv.dim() != 2 or yv.shape[0] < 2 or yv.shape[1] < 1:
            raise ValueError('y must be (T, m) or (T,) with T >= 2 time steps, got shape %s' % (tuple(yv.shape),))
        T, m = int(yv.shape[0]), int(yv.shape[1])
        if m not in self.DRIFT_DIMS[drift]:
            raise ValueError('drift %r needs m in %s, got m = %d' % (drift, self.DRIFT_DIMS[drift], m))
        ob = ~torch.isnan(yv)
        if observed is not None:
            o = torch.as_tensor(observed).detach().to('cpu')
            if o.dim() == 1:
                o = o[:, None]
            if o.dtype != torch.bool or tuple(o.shape) != (T, m):
                raise ValueError('observed must be a bool mask of shape %s, got %s of shape %s'
                                 % ((T, m), o.dtype, tuple(o.shape)))
            ob = ob & o
        yv = torch.where(ob, yv, torch.zeros_like(yv))          # an unobserved entry's y is never read
        if not bool(torch.isfinite(yv).all()) or not bool(torch.isfinite(yv.float()).all()):
            raise ValueError('the observed entries of y must be finite (in fp32 too: the kernels read an fp32 copy)')
        names = self.DRIFT_PARAMS[drift]
        if drift_params is None:
            par = self.DRIFT_DEFAULTS[drift]
        elif isinstance(drift_params, dict):
            if set(drift_params) - set(names):
                raise ValueError('drift %r takes the parameters %s, got %s' % (drift, names, sorted(drift_params)))
            par = tuple(drift_params.get(k, v) for k, v in zip(names, self.DRIFT_DEFAULTS[drift]))
        else:
            par = tuple(drift_params)
            if len(par) != len(names):
                raise ValueError('drift %r takes the %d parameters %s, got %d' % (drift, len(names), names, len(par)))
        self.drift_params = tuple(_finite_fp32('drift parameter %s' % k, v) for k, v in zip(names, par))
        self.dt = _positive_fp32('dt', dt)
        self.initial_mean = _finite_fp32('initial_mean', initial_mean)
        self.initial_scale = _positive_fp32('initial_scale', initial_scale)
        self.scales_unknown = scale_prior is not None
        self.prior_loc, self.prior_scale = 0.0, 1.0
        if self.scales_unknown:
            try:
                loc, sc = scale_prior
            except (TypeError, ValueError):
                raise ValueError('scale_prior must be a pair (l, c), got %r' % (scale_prior,)) from None
            self.prior_loc = _finite_fp32('the location l of scale_prior', loc)
            self.prior_scale = _positive_fp32('the scale c of scale_prior', sc)
            _positive_fp32('1 / c^2 of scale_prior', 1.0 / self.prior_scale ** 2)
            self.innovation_scale = self.observation_scale = 1.0
        else:
            self.innovation_scale = _positive_fp32('innovation_scale', innovation_scale)
            self.observation_scale = _positive_fp32('observation_scale', observation_scale)
            _positive_fp32('1 / (innovation_scale^2 dt)', 1.0 / (self.innovation_scale ** 2 * self.dt))
            _positive_fp32('1 / observation_scale^2', 1.0 / self.observation_scale ** 2)
        _positive_fp32('1 / initial_scale^2', 1.0 / self.initial_scale ** 2)
        d = T * m + (2 if self.scales_unknown else 0)
        if event_shape is None:
            event_shape = (d,)
        elif isinstance(event_shape, int):
            event_shape = (event_shape,)
        self.event_shape = tuple(int(v) for v in event_shape)
        if self.event_size != d:
            raise ValueError('event_shape %s must have d = %d elements%s'
                             % (self.event_shape, d, ' (T m states, log sigma and log tau)' if self.scales_unknown else ''))
        self.dim = d
        self.drift = drift
        self.T, self.m = T, m
        self.y = yv.contiguous()                 # fp64 masters; the kernels get fp32
        self.observed = ob.contiguous()
        self.n_observed = int(ob.sum())
        self._dev = {}

    # ------------------------------------------------------------------ presets
    @classmethod
    def synthetic(cls, n_steps, drift, seed, observed=None, **model):
        """(potential, truth): a path simulated from the model itself (X_0 ~ N(mu0, s0^2 I), Euler-Maruyama steps; with
        `scale_prior` the generating scales are the model's `innovation_scale` / `observation_scale` all the same) and
        observed with noise on the entries of the bool mask `observed` ((T, m); everything when None); all draws in
        fp64 from one CPU torch.Generator seeded with `seed`.  `model`: the constructor's keywords.  `truth` is the
        generating state in the object's coordinates (d,), fp64."""
        T = int(n_steps)
        m = int(model.pop('m', cls.DRIFT_DIMS[drift][0] if drift in cls.DRIFT_DIMS else 1))
        proto = cls(torch.zeros(max(T, 2), m), drift=drift, **model)         # validates the model
        if T < 2:
            raise ValueError('n_steps must be >= 2, got %r' % (n_steps,))
        sig = _positive_fp32('innovation_scale', model.get('innovation_scale', 0.1))
        tau = _positive_fp32('observation_scale', model.get('observation_scale', 1.0))
        g = torch.Generator().manual_seed(int(seed))
        X = torch.empty(T, m, dtype=torch.float64)
        X[0] = proto.initial_mean + proto.initial_scale * torch.randn(m, generator=g, dtype=torch.float64)
        for t in range(1, T):
            X[t] = X[t - 1] + proto.dt * proto._drift(X[t - 1]) + sig * math.sqrt(proto.dt) * torch.randn(
                m, generator=g, dtype=torch.float64)
        y = X + tau * torch.randn(T, m, generator=g, dtype=torch.float64)
        pot = cls(y, observed=observed, drift=drift, **model)
        return pot, (pot.pack(X, sig, tau) if pot.scales_unknown else pot.pack(X))

    @staticmethod
    def _preset_model(model, unknown_scales):
        model = dict(model)
        if unknown_scales:
            model.setdefault('scale_prior', (0.0, 2.0))
        return model

    @classmethod
    def brownian_motion(cls, n_steps=30, unknown_scales=False, seed=0, **model):
        """The Inference Gym's BrownianMotionMissingMiddleObservations: m = 1, zero drift, dt = 1, innovation scale 0.1
        and observation scale 0.15 unless given, the middle third of the steps not observed; data simulated with
        `seed`.  `unknown_scales`: both scales with the LogNormal(0, 2) prior.  Returns the potential."""
        T = int(n_steps)
        model = cls._preset_model(model, unknown_scales)
        model.setdefault('dt', 1.0)
        model.setdefault('innovation_scale', 0.1)
        model.setdefault('observation_scale', 0.15)
        ob = torch.ones(max(T, 2), 1, dtype=torch.bool)
        ob[T // 3:T - T // 3] = False
        return cls.synthetic(T, 'cubic', seed, observed=ob[:T], m=1, drift_params=(0.0, 0.0), **model)[0]

    @classmethod
    def lorenz_bridge(cls, n_steps=30, dt=0.02, unknown_scales=False, seed=0, **model):
        """The Inference Gym's ConvectionLorenzBridge: m = 3, the Lorenz-63 drift, innovation scale 0.1 and observation
        scale 1 unless given, the FIRST component observed on the first and the last ten steps (a third of the steps
        at each end when n_steps < 30); the path starts about the origin, X_0 ~ N(0, I) unless `initial_mean` /
        `initial_scale` are given.  Data simulated with `seed`."""
        T = int(n_steps)
        model = cls._preset_model(model, unknown_scales)
        k = 10 if T >= 30 else max(T // 3, 1)
        ob = torch.zeros(max(T, 2), 3, dtype=torch.bool)
        ob[:k, 0] = True
        ob[T - k:, 0] = True
        return cls.synthetic(T, 'lorenz63', seed, observed=ob[:T], dt=dt, **model)[0]

    @classmethod
    def double_well_path(cls, n_steps=64, unknown_scales=False, seed=0, **model):
        """The double-well transition path: m = 1, f = x - x^3 (alpha = beta = 1), only the two end points observed, at
        -1 and +1 (observation scale 0.1, innovation scale 0.7, dt = 0.1 unless given).  `seed` is not used (the data
        are the two end points); kept for a uniform signature."""
        T = int(n_steps)
        if T < 2:
            raise ValueError('n_steps must be >= 2, got %r' % (n_steps,))
        model = cls._preset_model(model, unknown_scales)
        model.setdefault('dt', 0.1)
        model.setdefault('innovation_scale', 0.7)
        model.setdefault('observation_scale', 0.1)
        model.setdefault('initial_mean', -1.0)
        y = torch.full((T,), float('nan'), dtype=torch.float64)
        y[0], y[-1] = -1.0, 1.0
        return cls(y, drift='cubic', drift_params=(1.0, 1.0), **model)

    # ------------------------------------------------------------------ routing
    def fused_in(self, family: str) -> bool:
        return super().fused_in(family) and family in ('mcmc', 'flow_mh', 'neutra') and self.dim <= 1024

    # ------------------------------------------------------------------ helpers
    _flat = LatentGMRF._flat

    def paths(self, x):
        """The states X (..., T, m) of the coordinates x."""
        xf = self._flat(x)
        return xf[..., :self.T * self.m].reshape(xf.shape[:-1] + (self.T, self.m))

    def scales(self, x):
        """(sigma, tau), each (...,): the fixed scales, or e^p and e^q of the coordinates when they are unknown."""
        xf = self._flat(x)
        if not self.scales_unknown:
            return (torch.full(xf.shape[:-1], self.innovation_scale, dtype=xf.dtype, device=xf.device),
                    torch.full(xf.shape[:-1], self.observation_scale, dtype=xf.dtype, device=xf.device))
        n = self.T * self.m
        return torch.exp(xf[..., n]), torch.exp(xf[..., n + 1])

    def pack(self, paths, innovation_scale=None, observation_scale=None):
        """The coordinates x (..., d) of paths (..., T, m) (or (..., T) when m = 1) and, when the scales are unknown,
        of sigma and tau (numbers or (...,); both needed).  Inverse of `paths` / `scales`."""
        X = torch.as_tensor(paths)
        if self.m == 1 and X.shape[-1:] == (self.T,) and X.shape[-2:] != (self.T, 1):
            X = X[..., None]
        if X.shape[-2:] != (self.T, self.m):
            raise ValueError('paths must end in (T, m) = %s, got shape %s' % ((self.T, self.m), tuple(X.shape)))
        if not X.is_floating_point():
            X = X.to(torch.get_default_dtype())
        head = X.reshape(X.shape[:-2] + (self.T * self.m,))
        if not self.scales_unknown:
            if innovation_scale is not None or observation_scale is not None:
                raise ValueError('the scales are fixed (no scale_prior): pack takes none')
            return head
        if innovation_scale is None or observation_scale is None:
            raise ValueError('the scales are coordinates: pack needs innovation_scale and observation_scale')
        sig, tau = (torch.as_tensor(v).to(head).expand(head.shape[:-1]) for v in (innovation_scale, observation_scale))
        if not bool((sig > 0).all()) or not bool((tau > 0).all()):
            raise ValueError('the scales must be positive')
        return torch.cat([head, torch.log(sig)[..., None], torch.log(tau)[..., None]], dim=-1)

    def prior_draws(self, n, seed):
        """n draws from the prior in coordinate form, (n, d) fp64 on the CPU: the scales from their LogNormal prior when
        unknown, X_0 ~ N(mu0, s0^2 I), then Euler-Maruyama steps; one CPU torch.Generator seeded with `seed`.  These
        are the starts to use: N(0, I) starts sit far in the tails of a stiff bridge."""
        n = int(n)
        if n < 1:
            raise ValueError('n must be >= 1, got %r' % (n,))
        g = torch.Generator().manual_seed(int(seed))
        if self.scales_unknown:
            ls = self.prior_loc + self.prior_scale * torch.randn(n, 2, generator=g, dtype=torch.float64)
            sig = torch.exp(ls[:, 0])
        else:
            sig = torch.full((n,), self.innovation_scale, dtype=torch.float64)
        z = torch.randn(n, self.T, self.m, generator=g, dtype=torch.float64)
        X = torch.empty(n, self.T, self.m, dtype=torch.float64)
        X[:, 0] = self.initial_mean + self.initial_scale * z[:, 0]
        for t in range(1, self.T):
            X[:, t] = X[:, t - 1] + self.dt * self._drift(X[:, t - 1]) + (sig * math.sqrt(self.dt))[:, None] * z[:, t]
        head = X.reshape(n, -1)
        return torch.cat([head, ls], dim=1) if self.scales_unknown else head

    def gaussian(self):
        """The equivalent FullRankGaussian (the same U up to a constant; a block-tridiagonal precision) when the model is
        linear and its scales are fixed: drift 'cubic' with beta = 0.  ValueError otherwise."""
        if self.drift != 'cubic' or self.drift_params[1] != 0.0 or self.scales_unknown:
            raise ValueError("gaussian() needs the drift 'cubic' with beta = 0 and fixed scales: anything else is not Gaussian")
        T, m, n = self.T, self.m, self.T * self.m
        a = 1.0 + self.dt * self.drift_params[0]
        om, rho = 1.0 / (self.innovation_scale ** 2 * self.dt), 1.0 / self.observation_scale ** 2
        P = torch.zeros(n, n, dtype=torch.float64)
        idx = torch.arange(n)
        w = self.observed.to(torch.float64).reshape(-1)
        P[idx, idx] = rho * w
        P[idx[:m], idx[:m]] += 1.0 / self.initial_scale ** 2
        P[idx[m:], idx[m:]] += om
        P[idx[:-m], idx[:-m]] += om * a * a
        P[idx[m:], idx[:-m]] -= om * a
        P[idx[:-m], idx[m:]] -= om * a
        b = rho * w * self.y.reshape(-1)
        b[:m] += self.initial_mean / self.initial_scale ** 2
        return FullRankGaussian(torch.linalg.solve(P, b), precision=P, event_shape=self.event_shape)

    # ------------------------------------------------------------------ evaluation in torch ops
    def _drift(self, X):
        """f(X) of states X (..., m), in torch ops"""
        p = self.drift_params
        if self.drift == 'cubic':
            return p[0] * X - p[1] * X ** 3
        if self.drift == 'fitzhugh_nagumo':
            x0, x1 = X[..., 0], X[..., 1]
            return torch.stack([x0 - x0 ** 3 / 3.0 - x1 + p[3], p[2] * (x0 + p[0] - p[1] * x1)], dim=-1)
        x0, x1, x2 = X[..., 0], X[..., 1], X[..., 2]
        return torch.stack([p[0] * (x1 - x0), x0 * (p[1] - x2) - x1, x0 * x1 - p[2] * x2], dim=-1)

    def _copy(self, device, dtype=torch.float32):
        key = (str(device), dtype)
        if key not in self._dev:
            self._dev[key] = (self.y.to(device, dtype).contiguous(), self.observed.to(device, dtype).contiguous())
        return self._dev[key]

    def __call__(self, x):
        """U (n_chains,) of states x (n_chains, ...) in differentiable torch ops."""
        xf = x.reshape(x.shape[0], -1)
        y, w = self._copy(xf.device, xf.dtype)
        T, m = self.T, self.m
        X = xf[:, :T * m].reshape(-1, T, m)
        e = X[:, 1:] - X[:, :-1] - self.dt * self._drift(X[:, :-1])
        se = torch.sum(e * e, dim=(1, 2))
        sv = torch.sum(w * (X - y) ** 2, dim=(1, 2))
        u0 = 0.5 * torch.sum((X[:, 0] - self.initial_mean) ** 2, dim=1) / self.initial_scale ** 2
        if not self.scales_unknown:
            return (u0 + 0.5 * se / (self.innovation_scale ** 2 * self.dt) + 0.5 * sv / self.observation_scale ** 2)
        p, q = xf[:, T * m], xf[:, T * m + 1]
        c2 = self.prior_scale ** 2
        return (u0 + 0.5 * torch.exp(-2.0 * p) * se / self.dt + 0.5 * torch.exp(-2.0 * q) * sv + (T - 1) * m * p
                + self.n_observed * q + 0.5 * ((p - self.prior_loc) ** 2 + (q - self.prior_loc) ** 2) / c2)

    # ------------------------------------------------------------------ the kernels' view
    def code(self):
        """a_scalar of the descriptor: drift code + 4 [scales unknown] + 8 (m - 1)."""
        return float(self.DRIFTS.index(self.drift) + (4 if self.scales_unknown else 0) + 8 * (self.m - 1))

    def data_block(self):
        """The kernels' view (NFMC_POT_DIFFUSION_BRIDGE, include/nfmc_hip.h), fp32 on the CPU: (header, rows).  Header: 16
        floats (dt, sigma, tau, mu0, 1/s0^2, l, 1/c^2, N_o, (T-1) m, four drift parameters, 0, 0, 0).  Rows (2, n4),
        n4 = 4 ceil(T m / 4): y and w (1 observed, 0 not), time-major, zero past T m."""
        n = self.T * self.m
        n4 = 4 * ((n + 3) // 4)
        par = self.drift_params + (0.0,) * (4 - len(self.drift_params))
        head = torch.tensor([self.dt, self.innovation_scale, self.observation_scale, self.initial_mean,
                             1.0 / self.initial_scale ** 2, self.prior_loc, 1.0 / self.prior_scale ** 2,
                             float(self.n_observed), float((self.T - 1) * self.m)] + list(par) + [0.0, 0.0, 0.0],
                            dtype=torch.float64)
        rows = torch.zeros(2, n4, dtype=torch.float64)
        rows[0, :n] = self.y.reshape(-1)
        rows[1, :n] = self.observed.to(torch.float64).reshape(-1)
        return head.to(torch.float32), rows.to(torch.float32)

    def descriptor(self, device):
        key = (str(device), 'descriptor')
        if key not in self._dev:
            head, rows = self.data_block()
            self._dev[key] = (head.to(device).contiguous(), rows.to(device).contiguous())
        head, rows = self._dev[key]
        return hip.NfmcPotential(hip.POT_DIFFUSION_BRIDGE, self.T, hip.ptr(head), hip.ptr(rows), self.code(), 0.0)


_log = logging.getLogger('nfmc_amd')
_announced = set()


def recognize(target, event_shape, rtol: float = 1e-5, x_scale: float = None) -> Optional[Potential]:
    """A QuadraticPotential that reproduces the plain callable `target` on every probe below, or None.

    This is an inference from finitely many evaluations, not a proof: a callable that is quadratic on all probed
    points and something else elsewhere (walls or modes beyond the probed radii), or one that changes between calls,
    would be sampled as the fitted Gaussian.  The probes therefore cover, besides the unit directions used for the
    fit, random points at radii 0.1 ... 100 per coordinate AND at 1x / 3x / 10x the largest |x0| of the run
    (`x_scale`), a repeated evaluation (stateful / stochastic targets differ), and the autograd gradient; any mismatch,
    non-finite value or exception -> None (the sampler then takes the split path, where an exception of the target
    surfaces unchanged).  The first time a callable is rerouted one line is logged on the `nfmc_amd` logger.  Opt out
    with `sample(..., fuse='never')` / `sampler.fuse = False`, or pass a `Potential` to be explicit."""
    if isinstance(target, Potential):
        return target
    d = int(math.prod(event_shape))
    try:
        with torch.no_grad():
            g = torch.Generator().manual_seed(0x5EED)
            z = torch.zeros(1, *event_shape, dtype=torch.float64)
            c0 = target(z).reshape(-1).double()
            eye = torch.eye(d, dtype=torch.float64).reshape(d, *event_shape)
            up = target(eye).reshape(-1).double()
            um = target(-eye).reshape(-1).double()
            if not (torch.isfinite(c0).all() and torch.isfinite(up).all() and torch.isfinite(um).all()):
                return None
            # U(t e_j) = a_j t^2 - 2 a_j b_j t + (c0)  =>  a_j = (U+ + U- - 2 c0)/2, a_j b_j = (U- - U+)/4
            a = (up + um - 2 * c0) / 2
            ab = (um - up) / 4
            b = torch.where(a > 0, ab / torch.where(a > 0, a, torch.ones_like(a)), torch.zeros_like(a))
            const = c0 - (a * b * b).sum()
            if not torch.isfinite(a).all() or not torch.isfinite(b).all() or (a < 0).any():
                return None
            scales = [0.1, 1.0, 7.0, 30.0, 100.0]
            if x_scale is not None and math.isfinite(x_scale) and x_scale > 0:
                scales += [x_scale, 3.0 * x_scale, 10.0 * x_scale]
            for scale in scales:
                x = scale * torch.randn(8, *event_shape, generator=g, dtype=torch.float64)
                want = target(x).reshape(-1).double()
                got = (a * (x.reshape(8, -1) - b) ** 2).sum(-1) + const
                if not torch.allclose(got, want, rtol=rtol, atol=rtol * (1 + want.abs().max())):
                    return None
            if not torch.equal(target(x).reshape(-1).double(), want):   # same input, same answer
                return None
        # gradient check through autograd (catches targets that detach / are piecewise)
        with torch.enable_grad():
            x = torch.randn(4, *event_shape, generator=g, dtype=torch.float64).requires_grad_(True)
            gr, = torch.autograd.grad(target(x).sum(), x)
        want_g = (2 * a * (x.detach().reshape(4, -1) - b)).reshape(x.shape)
        if not torch.allclose(gr, want_g, rtol=rtol, atol=rtol * (1 + want_g.abs().max())):
            return None
    except Exception:
        return None

    def simplify(v):
        return float(v[0]) if bool((v == v[0]).all()) else v.float()

    key = getattr(target, '__qualname__', None) or type(target).__name__
    if key not in _announced:
        _announced.add(key)
        _log.warning('nfmc_amd: target %r reproduces U(x) = sum_j a_j (x_j - b_j)^2 + c on every probe (radii up to %.3g); '
                     'it is evaluated in closed form inside the HIP kernels.  Pass fuse="never" to sample() to keep '
                     'calling the Python callable.', key, max(scales))
    return QuadraticPotential(tuple(event_shape), simplify(a), simplify(b))
