"""fp64 restatement of the blocked Rosenbrock target (potentials.Rosenbrock), for the host and GPU tests: U and its
autograd gradient, the analytic diagonal of its Hessian (step sizes), an exact ancestral sampler and the closed-form
moments of the block-2 target."""
import math

import torch


class RosenbrockU64:
    """U(x) = sum_{heads c} a (x_c - mu)^2 + sum_{non-heads c} b (x_c - x_{c-1}^2)^2 in fp64, c a head when
    c % block == 0.  Written as an explicit loop over the coordinates, not the class's vectorised torch.where.  Callable
    on (n, ...) tensors of any dtype; works under autograd."""

    def __init__(self, d, mu=1.0, a=0.05, b=5.0, block=2):
        self.d, self.mu, self.a, self.b, self.block = int(d), float(mu), float(a), float(b), int(block)

    def __call__(self, x):
        x = x.reshape(x.shape[0], -1).double()
        u = torch.zeros(x.shape[0], dtype=torch.float64)
        for c in range(self.d):
            if c % self.block == 0:
                u = u + self.a * (x[:, c] - self.mu) ** 2
            else:
                u = u + self.b * (x[:, c] - x[:, c - 1] ** 2) ** 2
        return u

    def grad(self, x):
        t = x.reshape(x.shape[0], -1).double().detach().requires_grad_(True)
        (g,) = torch.autograd.grad(self(t).sum(), t)
        return g

    def hess_diag(self, x):
        """d^2 U / dx_c^2 per coordinate: [head] 2a + [non-head] 2b + [c+1 < d non-head] (12 b x_c^2 - 4 b x_{c+1})."""
        x = x.reshape(x.shape[0], -1).double()
        h = torch.empty_like(x)
        for c in range(self.d):
            v = 2 * self.a if c % self.block == 0 else 2 * self.b
            if c + 1 < self.d and (c + 1) % self.block != 0:
                v = v + 12 * self.b * x[:, c] ** 2 - 4 * self.b * x[:, c + 1]
            h[:, c] = v
        return h

    def draw(self, n, seed):
        """n exact fp64 draws by ancestral sampling: x_head ~ N(mu, 1/(2a)), x_c | x_{c-1} ~ N(x_{c-1}^2, 1/(2b))."""
        z = torch.randn(n, self.d, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
        x = torch.empty_like(z)
        sa, sb = math.sqrt(0.5 / self.a), math.sqrt(0.5 / self.b)
        for c in range(self.d):
            if c % self.block == 0:
                x[:, c] = self.mu + sa * z[:, c]
            else:
                x[:, c] = x[:, c - 1] ** 2 + sb * z[:, c]
        return x

    def block2_moments(self):
        """Closed-form means and variances (d,) of the block-2 target, s2 = 1/(2a): heads mean mu, variance s2;
        non-heads mean mu^2 + s2, variance 4 mu^2 s2 + 2 s2^2 + 1/(2b)."""
        assert self.block == 2
        s2 = 0.5 / self.a
        mean = torch.empty(self.d, dtype=torch.float64)
        var = torch.empty(self.d, dtype=torch.float64)
        mean[0::2], var[0::2] = self.mu, s2
        mean[1::2] = self.mu ** 2 + s2
        var[1::2] = 4 * self.mu ** 2 * s2 + 2 * s2 ** 2 + 0.5 / self.b
        return mean, var
