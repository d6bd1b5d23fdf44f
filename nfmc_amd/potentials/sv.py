"""The stochastic-volatility model (csrc/pot_sv.hpp)."""
import math

import torch

from .. import hip
from ._base import VALU_FAMILIES, Potential, _check_finite, _pair, _positive_fp32


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
    fused_families = VALU_FAMILIES

    def __init__(self, y, mu_scale=10.0, sigma_scale=5.0, phi_prior=(1.0, 1.0)):
        y = y if torch.is_tensor(y) else torch.as_tensor(y, dtype=torch.float64)
        if y.dim() != 1 or y.shape[0] < 1:
            raise ValueError('y must be a 1-D series of T >= 1 returns, got shape %s' % (tuple(y.shape),))
        y = y.detach().to('cpu', torch.float64)
        _check_finite(y, 'y must be finite, in fp32 too (the kernels read an fp32 copy)')
        alpha, beta = _pair(phi_prior, 'phi_prior', '(alpha, beta)', sized=True)
        self.mu_scale = _positive_fp32('mu_scale', mu_scale)
        self.sigma_scale = _positive_fp32('sigma_scale', sigma_scale)
        self.alpha = _positive_fp32('phi_prior alpha', alpha)
        self.beta = _positive_fp32('phi_prior beta', beta)
        self.y = y.contiguous()          # fp64 master; the kernels get fp32
        self.T = int(y.shape[0])
        self.event_shape = (self.T + 3,)
        self._dev = {}

    def _tables(self, device, dtype):
        """(y (T,), y^2 (T,), (alpha, beta) (2,)) of `device` in `dtype`, made once per (device, dtype)"""
        def make():
            y = self.y.to(device, dtype).contiguous()
            ab = torch.tensor([self.alpha, self.beta], dtype=torch.float64).to(device, dtype).contiguous()
            return y, (self.y * self.y).to(device, dtype), ab
        return self._cached((str(device), dtype), make)

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
        x = self._event_states(x)
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
