"""The latent Gaussian Markov random field, a sparse prior precision (csrc/pot_gmrf.hpp)."""
import math
import numbers

import torch

from .. import hip
from ._base import VALU_FAMILIES, Potential, _as_fp64, _check_finite, _event_shape, _one_of, _pair, _positive_fp32, _spd_inverse
from ._observations import SiteObservations
from .lgm import LatentGaussianModel


class LatentGMRF(SiteObservations, Potential):
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
    fused_families, fused_max_dim = VALU_FAMILIES, 1024
    PARAMETERIZATIONS = ('centered', 'scaled')
    SYMMETRY_RTOL = 1e-6
    MAX_WIDTH = 32           # ELL slots the kernels run (check_gmrf, csrc/pot_kinds.hpp)

    def __init__(self, y, structure, likelihood='poisson', mean=0.0, weight=None, observed=None, precision=1.0,
                 precision_prior=None, parameterization='centered', rank=None, dof=4.0, scale=1.0, event_shape=None):
        _one_of('likelihood', likelihood, self.LIKELIHOODS)
        _one_of('parameterization', parameterization, self.PARAMETERIZATIONS)
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
        _check_finite(self.values, 'precision * structure must be finite in fp32 too (the kernels read an fp32 copy)')
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
            a, b = _pair(precision_prior, 'precision_prior', '(a, b) = (shape, rate)')
            self.prior_shape = _positive_fp32('the shape a of precision_prior', a)
            self.prior_rate = _positive_fp32('the rate b of precision_prior', b)
        self._set_observations(yv, n, 'n', likelihood, mean, weight, observed, dof, scale)
        d = n + 1 if self.tau_unknown else n
        self.event_shape = _event_shape(event_shape, d, ' (n sites and log tau)' if self.tau_unknown else '')
        self.dim = d
        self.parameterization = parameterization
        self.scaled = parameterization == 'scaled'
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
        return super().fused_in(family) and self.width <= self.MAX_WIDTH

    # ------------------------------------------------------------------ helpers
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

    def _model(self):
        return dict(likelihood=self.likelihood, mean=self.mean, weight=self.weight, rank=self.rank, dof=self.dof,
                    scale=self.scale, precision_prior=(self.prior_shape, self.prior_rate) if self.tau_unknown else None)

    def reparameterized(self, parameterization):
        """The same data, prior and hyperprior in the form `parameterization` ('centered' / 'scaled'; tau must be
        unknown for 'scaled'): U_scaled(u, s) = U_centred(m + e^(-s/2) u, s) + (n/2) s, the log Jacobian."""
        _one_of('parameterization', parameterization, self.PARAMETERIZATIONS)
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
        return LatentGaussianModel(self.y, _spd_inverse(chol), likelihood=self.likelihood, mean=self.mean, weight=self.weight,
                                   parameterization='centered', dof=self.dof, scale=self.scale, event_shape=self.event_shape)

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
        def make():
            val, col = self._ell64
            return (val.to(device, dtype).contiguous(), col.to(device).contiguous()) + tuple(
                v.to(device, dtype).contiguous() for v in (self.mean, self.y, self.weight))
        return self._cached((str(device), dtype), make)

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
        n = self.n_sites
        val, col = self._ell64
        block = torch.stack([val, col.to(torch.float64)]).to(torch.float32).contiguous()
        tab = self._table(n)
        tab[4:8] = torch.tensor([self.prior_shape, self.prior_rate, 0.5 * self.rank, 0.5 * (n - self.rank)], dtype=torch.float64)
        return block, tab.to(torch.float32)

    def descriptor(self, device):
        block, tab = self._descriptor_blocks(device)
        return hip.NfmcPotential(hip.POT_LATENT_GMRF, self.width, hip.ptr(block), hip.ptr(tab), self.code(), 0.0)
