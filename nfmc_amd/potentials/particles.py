"""Interacting particles in a harmonic trap (csrc/pot_particles.hpp)."""
import math

import torch

from .. import hip
from ._base import VALU_FAMILIES, Potential, _finite_fp32, _positive_fp32


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
    fused_families, fused_max_dim = VALU_FAMILIES, 1024
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
        x = self._event_states(x)
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
        par = self._cached(str(device), lambda: self.data_block().to(device).contiguous())
        return hip.NfmcPotential(hip.POT_PARTICLES, self.n_particles, hip.ptr(par), None, 0.0, 0.0)
