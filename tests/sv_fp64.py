"""fp64 restatement of the stochastic-volatility target (potentials.StochasticVolatility), for the host and GPU tests: U
written as an explicit loop over t, its autograd gradient, the diagonal of its Hessian (step sizes) and a seeded
simulator of (y, h) from the model."""
import math

import torch


def _softplus(z):
    return torch.clamp(z, min=0) + torch.log1p(torch.exp(-z.abs()))


class SVU64:
    """U(x) of the stochastic-volatility model in fp64, x = (mu, s = log sigma, r = atanh phi, h_0 .. h_{T-1}):

        U = log1p((mu/c_mu)^2) + softplus(2(s - log c_sigma)) - s + (alpha + 1/2) softplus(-2r) + (beta + 1/2) softplus(2r)
          + 1/2 q w delta_0^2 + s + sum_{t>=1} [1/2 w e_t^2 + s] + sum_{t>=0} 1/2 [h_t + y_t^2 e^{-h_t}]

    term by term as the model's negative log densities give it (the Jacobian -s of sigma and the +s of h_0's normaliser
    kept apart), one loop iteration per t.  Callable on (n, ...) tensors of any dtype; works under autograd."""

    def __init__(self, y, mu_scale=10.0, sigma_scale=5.0, alpha=1.0, beta=1.0):
        self.y = torch.as_tensor(y, dtype=torch.float64).reshape(-1)
        self.T = int(self.y.shape[0])
        self.d = self.T + 3
        self.cm, self.cs, self.alpha, self.beta = float(mu_scale), float(sigma_scale), float(alpha), float(beta)

    def __call__(self, x):
        x = x.reshape(x.shape[0], -1).double()
        mu, s, r = x[:, 0], x[:, 1], x[:, 2]
        w = torch.exp(-2 * s)
        phi = torch.tanh(r)
        q = 4 * torch.sigmoid(2 * r) * torch.sigmoid(-2 * r)
        u = (torch.log1p((mu / self.cm) ** 2) + _softplus(2 * (s - math.log(self.cs))) - s
             + (self.alpha + 0.5) * _softplus(-2 * r) + (self.beta + 0.5) * _softplus(2 * r))
        for t in range(self.T):
            h = x[:, 3 + t]
            if t == 0:
                u = u + 0.5 * q * w * (h - mu) ** 2 + s
            else:
                e = h - mu - phi * (x[:, 2 + t] - mu)
                u = u + 0.5 * w * e ** 2 + s
            u = u + 0.5 * (h + self.y[t] ** 2 * torch.exp(-h))
        return u

    def grad(self, x):
        t = x.reshape(x.shape[0], -1).double().detach().requires_grad_(True)
        (g,) = torch.autograd.grad(self(t).sum(), t)
        return g

    def hess_diag(self, x):
        """d^2 U / dx_c^2 per coordinate: mu, s, r by double backward; h_t in closed form,
        1/2 y_t^2 e^{-h_t} + [t = 0] q w + [t >= 1] w + [t + 1 < T] phi^2 w."""
        x = x.reshape(x.shape[0], -1).double().detach()
        t = x.clone().requires_grad_(True)
        (g,) = torch.autograd.grad(self(t).sum(), t, create_graph=True)
        hd = torch.empty_like(x)
        for c in range(3):
            (hc,) = torch.autograd.grad(g[:, c].sum(), t, retain_graph=True)
            hd[:, c] = hc[:, c]
        s, r = x[:, 1], x[:, 2]
        w, phi = torch.exp(-2 * s), torch.tanh(r)
        q = 1 - phi ** 2
        for k in range(self.T):
            v = 0.5 * self.y[k] ** 2 * torch.exp(-x[:, 3 + k]) + (q * w if k == 0 else w)
            if k + 1 < self.T:
                v = v + phi ** 2 * w
            hd[:, 3 + k] = v
        return hd


def constrained_u64(x, y, mu_scale=10.0, sigma_scale=5.0, alpha=1.0, beta=1.0):
    """The model's negative log joint, summed from torch.distributions in fp64, plus the log-Jacobians of s = log sigma
    and r = atanh phi: U of SVU64 up to one constant.  Argument validation is off, so a state whose sigma or phi
    overflows gives a non-finite U for its own row (as the kernels do) instead of an error for the whole batch."""
    D = torch.distributions
    mu_scale, sigma_scale, alpha, beta = (torch.tensor(float(v), dtype=torch.float64)
                                          for v in (mu_scale, sigma_scale, alpha, beta))
    x = x.reshape(x.shape[0], -1).double()
    y = torch.as_tensor(y, dtype=torch.float64)
    mu, s, r, h = x[:, 0], x[:, 1], x[:, 2], x[:, 3:]
    sigma, phi = torch.exp(s), torch.tanh(r)
    lp = D.Cauchy(torch.zeros_like(mu_scale), mu_scale, validate_args=False).log_prob(mu)
    lp = lp + D.HalfCauchy(sigma_scale, validate_args=False).log_prob(sigma) + s                          # + log |d sigma / d s|
    lp = lp + D.Beta(alpha, beta, validate_args=False).log_prob((phi + 1) / 2) + torch.log((1 - phi ** 2) / 2)   # + log |d u / d r|
    lp = lp + D.Normal(mu, sigma / torch.sqrt(1 - phi ** 2), validate_args=False).log_prob(h[:, 0])
    if h.shape[1] > 1:
        m = mu[:, None] + phi[:, None] * (h[:, :-1] - mu[:, None])
        lp = lp + D.Normal(m, sigma[:, None], validate_args=False).log_prob(h[:, 1:]).sum(1)
    lp = lp + D.Normal(torch.zeros_like(h), torch.exp(h / 2), validate_args=False).log_prob(y).sum(1)
    return -lp


def simulate(T, mu=-1.0, sigma=0.25, phi=0.95, seed=0):
    """(y, h), both (T,) fp64, drawn from the model at the given parameters: h_0 from the stationary law."""
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(2, T, generator=gen, dtype=torch.float64)
    h = torch.empty(T, dtype=torch.float64)
    h[0] = mu + sigma / math.sqrt(1 - phi * phi) * z[0, 0]
    for t in range(1, T):
        h[t] = mu + phi * (h[t - 1] - mu) + sigma * z[0, t]
    return torch.exp(h / 2) * z[1], h


def start_states(T, n, seed, mu=-1.0, sigma=0.25, phi=0.95, spread=0.05):
    """n fp64 states near the simulating parameters and a simulated path: (y, x0 (n, T + 3), h).  Each chain's
    (mu, s, r) are jittered by `spread` and its h by spread * sigma around the path."""
    y, h = simulate(T, mu, sigma, phi, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    z = torch.randn(n, T + 3, generator=gen, dtype=torch.float64)
    x = torch.empty(n, T + 3, dtype=torch.float64)
    x[:, 0] = mu + spread * z[:, 0]
    x[:, 1] = math.log(sigma) + spread * z[:, 1]
    x[:, 2] = math.atanh(phi) + spread * z[:, 2]
    x[:, 3:] = h + spread * sigma * z[:, 3:]
    return y, x, h
