"""fp64 restatement of the phi^4 lattice field (potentials.LatticePhi4), for the host and GPU tests: U, its gradient,
the diagonal of its Hessian and the precision matrix of the lam = 0 model, all written as explicit loops over the sites
and bonds of the lattice, not the roll / pad arithmetic of the class.  The loops list the bonds and the neighbours once
per object; U and the gradient then sum along those lists."""
import itertools

import torch


class Phi4U64:
    """U(x) = sum_c [1/2 m2 x_c^2 + 1/4 lam x_c^4] + 1/2 kappa sum_bonds (x_c' - x_c)^2 in fp64 on a lattice of `shape`
    ((L,) or (H, W), flattened row-major).  'periodic': one forward bond per site and axis, wrapping round (none on an
    axis of length 1).  'zero': the field is 0 outside, an axis of length n has n + 1 bonds.  Callable on (n, ...)
    tensors of any dtype; works under autograd."""

    def __init__(self, shape, m2=-1.0, lam=1.0, kappa=1.0, boundary='periodic'):
        self.shape = tuple(int(v) for v in shape)
        assert boundary in ('periodic', 'zero')
        self.m2, self.lam, self.kappa, self.boundary = float(m2), float(lam), float(kappa), boundary
        self.ndim = len(self.shape)
        self.d = 1
        for v in self.shape:
            self.d *= v
        self.sites = list(itertools.product(*[range(v) for v in self.shape]))
        # the loops below run once, here; the evaluations gather along their index lists (index d: the zero outside)
        pad = lambda c: self.d if c is None else c   # noqa: E731
        self._a = torch.tensor([pad(a) for a, _ in self.bonds()], dtype=torch.long)
        self._b = torch.tensor([pad(b) for _, b in self.bonds()], dtype=torch.long)
        self._nb = [torch.tensor([pad(self.neighbours(s)[k]) for s in self.sites], dtype=torch.long)
                    for k in range(len(self.neighbours(self.sites[0])))]

    def index(self, site):
        c = 0
        for v, n in zip(site, self.shape):
            c = c * n + v
        return c

    def bonds(self):
        """(c, c') pairs of flat indices, None for the zero field outside the lattice; a bond appears once per time it
        is counted"""
        out = []
        for site in self.sites:
            for ax, n in enumerate(self.shape):
                nxt = list(site)
                nxt[ax] += 1
                if self.boundary == 'periodic':
                    if n == 1:
                        continue
                    nxt[ax] %= n
                    out.append((self.index(site), self.index(nxt)))
                else:
                    if site[ax] == 0:
                        out.append((None, self.index(site)))
                    out.append((self.index(site), self.index(nxt) if nxt[ax] < n else None))
        return out

    def neighbours(self, site):
        """flat indices of the 2 ndim neighbours of `site`, None where the zero boundary leaves one out; a periodic axis
        of length 1 has none"""
        out = []
        for ax, n in enumerate(self.shape):
            for step in (-1, 1):
                nb = list(site)
                nb[ax] += step
                if self.boundary == 'periodic':
                    if n == 1:
                        continue
                    nb[ax] %= n
                    out.append(self.index(nb))
                else:
                    out.append(self.index(nb) if 0 <= nb[ax] < n else None)
        return out

    def _padded(self, x):
        x = x.reshape(x.shape[0], -1).double()
        return x, torch.cat([x, torch.zeros_like(x[:, :1])], dim=1)

    def __call__(self, x):
        """site terms plus 1/2 kappa (x_c' - x_c)^2 over the list of bonds()"""
        x, xz = self._padded(x)
        u = torch.sum(0.5 * self.m2 * x ** 2 + 0.25 * self.lam * x ** 4, dim=1)
        if len(self._a):
            u = u + 0.5 * self.kappa * torch.sum((xz[:, self._b] - xz[:, self._a]) ** 2, dim=1)
        return u

    def grad(self, x):
        """m2 x_c + lam x_c^3 + kappa sum_{neighbours c'} (x_c - x_c') over the lists of neighbours(), a missing
        neighbour reading as 0"""
        x, xz = self._padded(x)
        g = self.m2 * x + self.lam * x ** 3
        for nb in self._nb:
            g = g + self.kappa * (x - xz[:, nb])
        return g

    def hess_diag(self, x):
        """m2 + 3 lam x_c^2 + 2 ndim kappa (every site has two neighbour terms per axis; a periodic axis of length 1
        has none, so there this is an upper bound)"""
        x = x.reshape(x.shape[0], -1).double()
        return self.m2 + 3.0 * self.lam * x * x + 2.0 * self.ndim * self.kappa

    def precision(self):
        """(d, d): m2 I + kappa sum_bonds (e_c' - e_c)(e_c' - e_c)^T"""
        p = self.m2 * torch.eye(self.d, dtype=torch.float64)
        for a, b in self.bonds():
            for i, si in ((a, -1.0), (b, 1.0)):
                for j, sj in ((a, -1.0), (b, 1.0)):
                    if i is not None and j is not None:
                        p[i, j] += self.kappa * si * sj
        return p
