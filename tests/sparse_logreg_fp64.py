"""fp64 restatement of the sparse logistic-regression target (potentials.SparseLogisticRegression), for the host and GPU
tests: U written as loops over the coefficients and the rows, its autograd gradient, the model's log densities from
torch.distributions, the diagonal of its Hessian (step sizes), a seeded synthetic data set drawn from the model, and start
states."""
import math

import torch


class SLRU64:
    """U(x) in fp64, x = (w_0, l_0, w_1, l_1, .., w_{D-1}, l_{D-1}, s), beta_j = e^{s + l_j} w_j, z = X beta:

        U = sum_i [log(1 + e^{z_i}) - y_i z_i] + sum_j [w_j^2 / 2 + b e^{l_j} - a l_j] + b e^s - a s

    log(1 + e^z) written as logaddexp(0, z), one loop iteration per coefficient and one per row.  Callable on (n, ...)
    tensors of any dtype; works under autograd."""

    def __init__(self, X, y, a=0.5, b=0.5):
        self.X = torch.as_tensor(X).double()
        self.y = torch.as_tensor(y).double()
        self.N, self.D = (int(v) for v in self.X.shape)
        self.d = 2 * self.D + 1
        self.a, self.b = float(a), float(b)

    def beta(self, x):
        x = x.reshape(x.shape[0], -1).double()
        s = x[:, 2 * self.D]
        return torch.stack([torch.exp(s + x[:, 2 * j + 1]) * x[:, 2 * j] for j in range(self.D)], dim=1)

    def __call__(self, x):
        x = x.reshape(x.shape[0], -1).double()
        s = x[:, 2 * self.D]
        u = self.b * torch.exp(s) - self.a * s
        for j in range(self.D):
            w, l = x[:, 2 * j], x[:, 2 * j + 1]
            u = u + 0.5 * w * w + self.b * torch.exp(l) - self.a * l
        z = self.beta(x) @ self.X.t()
        for i in range(self.N):
            u = u + torch.logaddexp(torch.zeros_like(z[:, i]), z[:, i]) - self.y[i] * z[:, i]
        return u

    def grad(self, x):
        t = x.reshape(x.shape[0], -1).double().detach().requires_grad_(True)
        (g,) = torch.autograd.grad(self(t).sum(), t)
        return g

    def hess_diag(self, x):
        """d^2 U / dx_c^2 in closed form, with v_i = p_i (1 - p_i), p = sigmoid(z), r = p - y, g = X^T r:
        w_j: e^{2(s + l_j)} sum_i X_ij^2 v_i + 1;  l_j: beta_j^2 sum_i X_ij^2 v_i + beta_j g_j + b e^{l_j};
        s: sum_i z_i^2 v_i + sum_j beta_j g_j + b e^s."""
        x = x.reshape(x.shape[0], -1).double()
        D = self.D
        w, l, s = x[:, 0:2 * D:2], x[:, 1:2 * D:2], x[:, 2 * D]
        e = torch.exp(s[:, None] + l)
        bt = e * w
        z = bt @ self.X.t()
        p = torch.sigmoid(z)
        v = p * (1 - p)
        g = (p - self.y) @ self.X
        xv = v @ (self.X * self.X)                     # sum_i X_ij^2 v_i
        hd = torch.empty_like(x)
        hd[:, 0:2 * D:2] = e * e * xv + 1
        hd[:, 1:2 * D:2] = bt * bt * xv + bt * g + self.b * torch.exp(l)
        hd[:, 2 * D] = (z * z * v).sum(1) + (bt * g).sum(1) + self.b * torch.exp(s)
        return hd


def model_u64(x, X, y, a=0.5, b=0.5):
    """The model's negative log joint from torch.distributions in fp64 -- Gamma(a, b) for tau and every lambda_j, N(0, 1)
    for w, Bernoulli(logits = z) for y -- plus the log-Jacobians s and l_j of tau = e^s and lambda_j = e^{l_j}: U of
    SLRU64 up to one constant.  Argument validation is off, so a state whose scales overflow gives a non-finite U for its
    own row (as the kernels do) instead of an error for the whole batch."""
    dist = torch.distributions
    x = x.reshape(x.shape[0], -1).double()
    X = torch.as_tensor(X, dtype=torch.float64)
    y = torch.as_tensor(y, dtype=torch.float64)
    D = (x.shape[1] - 1) // 2
    w, l, s = x[:, 0:2 * D:2], x[:, 1:2 * D:2], x[:, 2 * D]
    gam = dist.Gamma(torch.tensor(float(a), dtype=torch.float64), torch.tensor(float(b), dtype=torch.float64),
                     validate_args=False)
    lp = gam.log_prob(torch.exp(s)) + s + (gam.log_prob(torch.exp(l)) + l).sum(1)
    lp = lp + dist.Normal(torch.zeros_like(w), torch.ones_like(w), validate_args=False).log_prob(w).sum(1)
    z = (torch.exp(s)[:, None] * torch.exp(l) * w) @ X.t()
    lp = lp + dist.Bernoulli(logits=z, validate_args=False).log_prob(y.expand_as(z)).sum(1)
    return -lp


def synthetic(N, D, seed, n_nonzero=3, scale=1.0):
    """(X fp32 (N, D), y fp32 (N,), true beta fp64 (D,)) with a fixed seed: columns of X standardised (N >= 2) and then
    multiplied by `scale`; beta zero but for min(n_nonzero, D) coefficients of magnitude 1 .. 2 and alternating sign;
    y ~ Bernoulli(sigmoid(X beta))."""
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, D, generator=g, dtype=torch.float64)
    if N >= 2:
        X = (X - X.mean(0)) / X.std(0).clamp_min(1e-12)
    X = scale * X
    beta = torch.zeros(D, dtype=torch.float64)
    k = min(n_nonzero, D)
    idx = torch.randperm(D, generator=g)[:k]
    mag = 1.0 + torch.rand(k, generator=g, dtype=torch.float64)
    beta[idx] = mag * torch.tensor([(-1.0) ** i for i in range(k)], dtype=torch.float64)
    y = (torch.rand(N, generator=g, dtype=torch.float64) < torch.sigmoid(X @ beta)).double()
    return X.float(), y.float(), beta


def start_states(D, n, seed, spread=1.0):
    """n fp64 states (n, 2 D + 1): w_j ~ N(0, (0.5 spread)^2), l_j and s ~ N(0, (0.3 spread)^2)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.empty(n, 2 * D + 1, dtype=torch.float64)
    x[:, 0:2 * D:2] = 0.5 * spread * torch.randn(n, D, generator=g, dtype=torch.float64)
    x[:, 1:2 * D:2] = 0.3 * spread * torch.randn(n, D, generator=g, dtype=torch.float64)
    x[:, 2 * D] = 0.3 * spread * torch.randn(n, generator=g, dtype=torch.float64)
    return x


def prior_draws(D, n, a, b, seed):
    """n exact draws (n, 2 D + 1) of the prior (the posterior when X = 0): w ~ N(0, 1), lambda_j, tau ~ Gamma(a, b),
    logged.  log of a Gamma(a, b) draw has mean digamma(a) - log b and variance trigamma(a)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.empty(n, 2 * D + 1, dtype=torch.float64)
    x[:, 0:2 * D:2] = torch.randn(n, D, generator=g, dtype=torch.float64)
    gam = torch.distributions.Gamma(torch.full((n, D + 1), float(a), dtype=torch.float64),
                                    torch.full((n, D + 1), float(b), dtype=torch.float64))
    with torch.random.fork_rng(devices=[]):          # Gamma draws come from the global generator: seed a private copy
        torch.manual_seed(int(torch.randint(0, 2 ** 31 - 1, (1,), generator=g)))
        lg = torch.log(gam.sample())
    x[:, 1:2 * D:2] = lg[:, :D]
    x[:, 2 * D] = lg[:, D]
    return x


def log_gamma_moments(a, b):
    """mean and variance of log G, G ~ Gamma(a, b)"""
    a = torch.tensor(float(a), dtype=torch.float64)
    return float(torch.digamma(a)) - math.log(b), float(torch.polygamma(1, a))
