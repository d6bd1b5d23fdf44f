"""fp64 restatement of the latent Gaussian Markov random field (potentials.LatentGMRF), for the host and GPU tests, and
the seeded problems both use.  Written differently from the class: the structure matrix is DENSE and the quadratic form
goes through torch.einsum (the class gathers through ELL slots), tau = exp(s) and f = m + u / sqrt(tau) are explicit,
the three likelihoods come from torch.nn.functional / torch.log where the class uses logaddexp / log1p, the unobserved
sites are left out by an index list instead of a select, and the gradient is autograd's."""
import torch
import torch.nn.functional as F

LIKELIHOODS = ('poisson', 'binomial', 'student_t')
MODES = ('fixed', 'centered', 'scaled')
COMBOS = [(lik, mode) for lik in LIKELIHOODS for mode in MODES]
NU, SCALE = 4.0, 0.5
PRIOR = (2.0, 2.0)                     # tau ~ Gamma(2, 2)


class LatentGMRF64:
    """U of the GMRF model in fp64 (constants dropped), callable on (N, ...) tensors of any dtype, works under autograd.
    R dense (n, n); rho its rank; (a, b) the Gamma prior of tau.
      fixed:    U = 1/2 r^T R r + sum l_j(x_j)
      centered: U = 1/2 tau r^T R r - rho/2 s + sum l_j(x_j) + b tau - a s,          x = [f | s], tau = e^s
      scaled:   U = 1/2 u^T R u + sum l_j(m_j + u_j / sqrt(tau)) + b tau - a s + (n - rho)/2 s,   x = [u | s]"""

    def __init__(self, y, R, likelihood, mean, weight, mode, prior=PRIOR, rank=None, dof=NU, scale=SCALE):
        assert likelihood in LIKELIHOODS and mode in MODES
        self.R = torch.as_tensor(R).double()
        self.n = int(self.R.shape[0])
        self.d = self.n + (mode != 'fixed')
        self.y = torch.as_tensor(y).double().reshape(-1)
        self.m = torch.as_tensor(mean).double().expand(self.n).clone()
        self.w = torch.as_tensor(weight).double().expand(self.n).clone()
        self.on = torch.nonzero(self.w > 0).reshape(-1)
        self.likelihood, self.mode = likelihood, mode
        self.a, self.b = (float(v) for v in prior)
        self.rho = float(self.n if rank is None else rank)
        self.dof, self.scale = float(dof), float(scale)

    def split(self, x):
        x = x.reshape(x.shape[0], -1).double()
        if self.mode == 'fixed':
            return x, None
        return x[:, :self.n], x[:, self.n]

    def latent(self, x):
        head, s = self.split(x)
        if self.mode != 'scaled':
            return head
        return self.m[None, :] + head / torch.sqrt(s.exp())[:, None]

    def data_term(self, f):
        f, y, w = f[:, self.on], self.y[self.on], self.w[self.on]
        if self.likelihood == 'poisson':
            l = w * torch.exp(f) - y * f
        elif self.likelihood == 'binomial':
            l = w * F.softplus(f, beta=1.0, threshold=1e9) - y * f
        else:
            l = w * 0.5 * (self.dof + 1.0) * torch.log(1.0 + (y - f) ** 2 / (self.dof * self.scale ** 2))
        return l.sum(dim=1)

    def __call__(self, x):
        head, s = self.split(x)
        data = self.data_term(self.latent(x))
        if self.mode == 'fixed':
            r = head - self.m
            return 0.5 * torch.einsum('ni,ij,nj->n', r, self.R, r) + data
        tau = s.exp()
        hyper = self.b * tau - self.a * s
        if self.mode == 'centered':
            r = head - self.m
            return 0.5 * tau * torch.einsum('ni,ij,nj->n', r, self.R, r) - 0.5 * self.rho * s + data + hyper
        return 0.5 * torch.einsum('ni,ij,nj->n', head, self.R, head) + data + hyper + 0.5 * (self.n - self.rho) * s

    def grad(self, x):
        t = x.reshape(x.shape[0], -1).double().detach().requires_grad_(True)
        (g,) = torch.autograd.grad(self(t).sum(), t)
        return g

    def hessian_lmax(self, x):
        """lambda_max of the autograd Hessian of U at one state x (d,)."""
        H = torch.autograd.functional.hessian(lambda t: self(t[None])[0], x.double().reshape(-1), vectorize=True)
        return float(torch.linalg.eigvalsh(0.5 * (H + H.t())).max())


def graph_edges(n):
    """The seeded graph: the ring j ~ j + 1 (mod n) and the chord (j, (7 j + 3) mod n) for every j divisible by 3;
    duplicates merged, self loops dropped.  A sorted list of pairs (i < j)."""
    pairs = set()
    for j in range(n):
        for k in [(j + 1) % n] + ([(7 * j + 3) % n] if j % 3 == 0 else []):
            if k != j:
                pairs.add((min(j, k), max(j, k)))
    return sorted(pairs)


def laplacian(n, edges):
    L = torch.zeros(n, n, dtype=torch.float64)
    for i, j in edges:
        L[i, j] -= 1.0
        L[j, i] -= 1.0
        L[i, i] += 1.0
        L[j, j] += 1.0
    return L


def lattice_structure(H, W, kappa2, alpha):
    """(kappa2 I + G)^alpha dense, G the Laplacian of the (H, W) grid's 4-neighbour graph with free boundaries."""
    edges = [(i * W + j, i * W + j + 1) for i in range(H) for j in range(W - 1)]
    edges += [(i * W + j, (i + 1) * W + j) for i in range(H - 1) for j in range(W)]
    A = laplacian(H * W, edges) + kappa2 * torch.eye(H * W, dtype=torch.float64)
    return torch.linalg.matrix_power(A, alpha)


def observations(f, likelihood, g):
    """Weights and observations drawn at the field f as latent_gaussian_fp64.problem_data draws them, and its seeded 20 %
    of unobserved sites: (weight, y, observed)."""
    n = f.numel()
    if likelihood == 'poisson':
        w = 0.5 + torch.rand(n, generator=g, dtype=torch.float64)
        y = torch.poisson(w * torch.exp(f), generator=g)
    elif likelihood == 'binomial':
        w = torch.randint(1, 6, (n,), generator=g).double()
        hits = torch.rand(5, n, generator=g, dtype=torch.float64) < torch.sigmoid(f)
        y = (hits & (torch.arange(5)[:, None] < w[None, :])).sum(0).double()
    else:
        w = torch.ones(n, dtype=torch.float64)
        noise = SCALE * torch.randn(n, generator=g, dtype=torch.float64)
        out = torch.rand(n, generator=g, dtype=torch.float64) < 0.10
        sign = torch.where(torch.rand(n, generator=g, dtype=torch.float64) < 0.5, -1.0, 1.0).double()
        y = f + torch.where(out, 5.0 * SCALE * sign, noise)
    observed = torch.rand(n, generator=g, dtype=torch.float64) >= 0.20
    return w, y, observed


def problem_data(n, likelihood, seed, structure=None):
    """The seeded problem on n sites, independent of the mode: R = Laplacian(graph_edges(n)) + 0.5 I unless a dense
    `structure` is given (proper), m = 1 (Poisson) or 0, the generating field f* = m + L^-T eps with R = L L^T, s* = 0,
    and `observations` at f*.  Returns a dict."""
    g = torch.Generator().manual_seed(int(seed))
    edges = graph_edges(n)
    R = laplacian(n, edges) + 0.5 * torch.eye(n, dtype=torch.float64) if structure is None else torch.as_tensor(structure).double()
    L = torch.linalg.cholesky(R)
    m = torch.full((n,), 1.0 if likelihood == 'poisson' else 0.0, dtype=torch.float64)
    eps = torch.randn(n, generator=g, dtype=torch.float64)
    fs = m + torch.linalg.solve(L.t(), eps)
    w, y, observed = observations(fs, likelihood, g)
    return dict(n=n, edges=edges, R=R, mean=m, f_star=fs, weight=w, y=y, observed=observed, likelihood=likelihood)


def n_of(d, mode):
    """sites of a problem with d coordinates"""
    return d if mode == 'fixed' else d - 1


def make_pair(data, mode, event_shape=None, intrinsic=False):
    """(package potential, fp64 restatement) of problem_data's dict in one mode.  intrinsic: the ICAR model on the same
    graph (R = D - A, rank n - 1: the ring connects the graph) in place of the proper R."""
    from nfmc_amd.potentials import LatentGMRF
    lik, n = data['likelihood'], data['n']
    model = dict(likelihood=lik, mean=data['mean'], weight=data['weight'], observed=data['observed'], dof=NU, scale=SCALE,
                 event_shape=event_shape)
    if mode != 'fixed':
        model.update(precision_prior=PRIOR, parameterization=mode)
    if intrinsic:
        pot = LatentGMRF.icar(data['y'], torch.tensor(data['edges']).reshape(-1, 2), **model)
        R, rank = laplacian(n, data['edges']), n - 1
    else:
        pot = LatentGMRF(data['y'], data['R'], **model)
        R, rank = data['R'], n
    w = torch.where(data['observed'], data['weight'], torch.zeros_like(data['weight']))
    return pot, LatentGMRF64(data['y'], R, lik, data['mean'], w, mode, PRIOR, rank, NU, SCALE)


def truth(data, ref):
    """The generating state (tau* = 1) in the coordinates of `ref`, (d,) fp64."""
    if ref.mode == 'fixed':
        return data['f_star'].clone()
    head = data['f_star'] if ref.mode == 'centered' else data['f_star'] - data['mean']
    return torch.cat([head, torch.zeros(1, dtype=torch.float64)])


def starts(data, ref, n_chains, seed, spread=0.3):
    """n_chains fp32 starts in the coordinates of `ref`: the generating state + spread eps, rounded to fp32."""
    g = torch.Generator().manual_seed(int(seed))
    t = truth(data, ref)
    return (t[None, :] + spread * torch.randn(n_chains, t.numel(), generator=g, dtype=torch.float64)).float()


def step_lambda(data, ref, x0):
    """lambda of the step-size rule: the largest autograd-Hessian lambda_max over the generating state and the first 8
    starts."""
    states = [truth(data, ref)] + [x.double() for x in x0[:8]]
    return max(ref.hessian_lmax(x) for x in states)
