"""The full-rank Gaussian (csrc/pot_fullrank.hpp)."""
import torch

from .. import hip
from ._base import VALU_FAMILIES, Potential, _check_finite, _event_shape, _spd, _spd_inverse


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
    fused_families = VALU_FAMILIES
    SYMMETRY_RTOL = 1e-6

    def __init__(self, mu, covariance=None, precision=None, event_shape=None):
        if (covariance is None) == (precision is None):
            raise ValueError('give exactly one of covariance / precision')
        name = 'covariance' if covariance is not None else 'precision'
        m = torch.as_tensor(covariance if covariance is not None else precision).detach().to('cpu', torch.float64)
        m, chol = _spd(name, m, self.SYMMETRY_RTOL)
        d = int(m.shape[0])
        mu = torch.as_tensor(mu).detach().to('cpu', torch.float64).reshape(-1)
        if mu.numel() != d:
            raise ValueError('mu must have d = %d entries, got %d' % (d, mu.numel()))
        if not bool(torch.isfinite(mu).all()):
            raise ValueError('mu must be finite')
        self.event_shape = _event_shape(event_shape, d)
        lam = _spd_inverse(chol) if covariance is not None else m
        _check_finite(lam, 'the precision matrix must be finite in fp32 too (the kernels read an fp32 copy)')
        self.dim = d
        self.mean = mu.contiguous()          # fp64 masters; the kernels get fp32
        self.precision = lam.contiguous()
        self._dev = {}

    def _copy(self, device):
        """The fp32 (Lambda, mu) of `device`, made once per device (every shard of a sharded run gets its own)."""
        return self._cached(str(device), lambda: (self.precision.float().to(device).contiguous(),
                                                  self.mean.float().to(device).contiguous()))

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
