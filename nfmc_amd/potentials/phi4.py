"""The phi^4 lattice field (csrc/pot_phi4.hpp)."""
import torch

from .. import hip
from ._base import VALU_FAMILIES, Potential, _finite_fp32


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
    fused_families, fused_max_dim = VALU_FAMILIES, 1024
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
        return super().fused_in(family) and self.event_shape[-1] % 4 == 0

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
        def make():
            # one row with the zero boundary on both axes, shape (1, W): the kernels' 1-D lattice with the two vertical
            # boundary bonds of every site, 1/2 kappa 2 x^2, folded into the mass term
            fold = self.boundary == 'zero' and len(self.event_shape) == 2 and self.event_shape[0] == 1
            m2 = _finite_fp32('m2 + 2 kappa', self.m2 + 2.0 * self.kappa) if fold else self.m2
            return torch.tensor([m2, self.lam, self.kappa, float(self.BOUNDARIES.index(self.boundary))],
                                dtype=torch.float64).to(device, torch.float32).contiguous()
        par = self._cached(str(device), make)
        return hip.NfmcPotential(hip.POT_LATTICE_PHI4, self.event_shape[-1], hip.ptr(par), None, 0.0, 0.0)
