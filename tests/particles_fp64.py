"""fp64 restatement of the interacting-particle target (NFMC_POT_PARTICLES) for the tests: U from explicit pair sums
over the upper-triangle index pairs (i < j), independent of ParticleSystem's own chunked pair-matrix code path; the
gradient by autograd; the diagonal Hessian in closed form (checked against autograd in tests/test_host_particles.py);
the lattice start states built site by site.

    U(x) = beta [ k/2 sum_i |r_i|^2 + sum_{i<j} phi(r_ij) ]
    Lennard-Jones  phi(r) = eps [ (r_m / r)^12 - 2 (r_m / r)^6 ]
    double well    phi(r) = a (r - r0) + b (r - r0)^2 + c (r - r0)^4
    d^2 U / d x_{ic}^2 = beta [ k + sum_{j != i} ( phi''(r) (dx_c / r)^2 + (phi'(r) / r) (1 - (dx_c / r)^2) ) ]
"""
import itertools

import torch


class Particles64:
    """U (n,) fp64 of states x (n, P D), particle-major; `grad`, `hess_diag`."""

    def __init__(self, n_particles, n_dims=3, pair='lennard_jones', trap=1.0, temperature=1.0, epsilon=1.0, r_min=1.0,
                 a=0.0, b=-4.0, c=0.9, r0=4.0):
        assert pair in ('lennard_jones', 'double_well')
        self.P, self.D, self.pair = int(n_particles), int(n_dims), pair
        self.d = self.P * self.D
        self.k, self.beta = float(trap), 1.0 / float(temperature)
        self.eps, self.rm = float(epsilon), float(r_min)
        self.a, self.b, self.c, self.r0 = float(a), float(b), float(c), float(r0)
        idx = [(i, j) for i in range(self.P) for j in range(i + 1, self.P)]
        self.i = torch.tensor([p[0] for p in idx], dtype=torch.int64)
        self.j = torch.tensor([p[1] for p in idx], dtype=torch.int64)

    def phi(self, r):
        """(phi, phi', phi'') at distances r"""
        if self.pair == 'lennard_jones':
            q = (self.rm / r) ** 6
            return (self.eps * (q * q - 2.0 * q), self.eps * (-12.0 * q * q + 12.0 * q) / r,
                    self.eps * (156.0 * q * q - 84.0 * q) / (r * r))
        u = r - self.r0
        return (self.a * u + self.b * u ** 2 + self.c * u ** 4, self.a + 2.0 * self.b * u + 4.0 * self.c * u ** 3,
                2.0 * self.b + 12.0 * self.c * u ** 2)

    def u(self, x):
        """U in the dtype of x"""
        n = x.shape[0]
        r = x.reshape(n, self.P, self.D)
        dist = torch.sqrt(((r[:, self.i] - r[:, self.j]) ** 2).sum(-1))     # (n, P (P - 1) / 2)
        return self.beta * (0.5 * self.k * (r ** 2).sum(dim=(1, 2)) + self.phi(dist)[0].sum(1))

    def __call__(self, x):
        return self.u(x.to(torch.float64))

    def u32(self, x):
        """The same sums in fp32: the restatement's own rounding error is u32(x) against __call__(x)."""
        return self.u(x.to(torch.float32))

    def grad(self, x):
        t = x.detach().to(torch.float64).clone().requires_grad_(True)
        (g,) = torch.autograd.grad(self(t).sum(), t)
        return g

    def hess_diag(self, x):
        x = x.detach().to(torch.float64)
        n = x.shape[0]
        r = x.reshape(n, self.P, self.D)
        dx = r[:, self.i] - r[:, self.j]                                    # (n, M, D)
        dist = torch.sqrt((dx ** 2).sum(-1, keepdim=True))
        _, p1, p2 = self.phi(dist)
        c2 = (dx / dist) ** 2
        h = p2 * c2 + (p1 / dist) * (1.0 - c2)                              # the same for both ends of a pair
        out = torch.full((n, self.P, self.D), self.k, dtype=torch.float64)
        out.index_add_(1, self.i, h)
        out.index_add_(1, self.j, h)
        return self.beta * out.reshape(n, self.d)


def lattice_sites(P, D, spacing):
    """The first P sites, row-major, of the simple lattice with ceil(P^(1/D)) sites per axis and the given spacing, moved
    so that their mean is the origin: (P, D) fp64, built site by site."""
    m = 1
    while m ** D < P:
        m += 1
    sites = [list(s) for s in itertools.islice(itertools.product(range(m), repeat=D), P)]
    t = torch.tensor(sites, dtype=torch.float64) * float(spacing)
    return t - t.sum(0) / P


def start_states(P, D, spacing, n, seed, jitter):
    """(n, P D) fp64: lattice_sites plus N(0, jitter^2) noise, one CPU generator seeded with `seed` (the draw of
    ParticleSystem.start_states: one randn of shape (n, P, D) in fp64)."""
    g = torch.Generator().manual_seed(int(seed))
    noise = torch.randn(n, P, D, generator=g, dtype=torch.float64)
    return (lattice_sites(P, D, spacing)[None] + float(jitter) * noise).reshape(n, P * D)


def min_pair_distance(x, P, D):
    """the smallest pair distance of each state: (n,)"""
    r = x.to(torch.float64).reshape(x.shape[0], P, D)
    return torch.pdist(r[0]).min().reshape(1) if x.shape[0] == 1 else torch.stack([torch.pdist(v).min() for v in r])
