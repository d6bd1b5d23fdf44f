"""fp64 restatement of the diffusion-bridge target (potentials.DiffusionBridge), for the host and GPU tests: U written as
a plain loop over t with the three drifts restated here (nothing of the package class is used), its autograd gradient,
the closed-form diagonal of its Hessian (step sizes), the model's log density summed from torch.distributions, and a
seeded simulator."""
import math

import torch

DRIFT_M = {'cubic': (1, 2, 3), 'fitzhugh_nagumo': (2,), 'lorenz63': (3,)}
DEFAULT_PARAMS = {'cubic': (0.0, 0.0), 'fitzhugh_nagumo': (0.7, 0.8, 0.08, 0.5), 'lorenz63': (10.0, 28.0, 8.0 / 3.0)}


def drift64(name, X, par):
    """f(X) for states X (..., m): a list of the m components"""
    if name == 'cubic':
        alpha, beta = par
        return [alpha * X[..., c] - beta * X[..., c] * X[..., c] * X[..., c] for c in range(X.shape[-1])]
    if name == 'fitzhugh_nagumo':
        a, b, eps, cur = par
        v, w = X[..., 0], X[..., 1]
        return [v - v * v * v / 3 - w + cur, eps * (v + a - b * w)]
    if name == 'lorenz63':
        s, r, beta = par
        x, y, z = X[..., 0], X[..., 1], X[..., 2]
        return [s * (y - x), x * (r - z) - y, x * y - beta * z]
    raise ValueError(name)


class DiffusionU64:
    """U(x) of the diffusion bridge in fp64, one loop iteration per time step, term by term as the model's negative log
    densities give it (constants dropped).  x = (X_0 .. X_{T-1} time-major [, p = log sigma, q = log tau]).  `scale_prior`
    = (l, c) makes the scales coordinates.  Callable on (n, ...) tensors of any dtype; works under autograd."""

    def __init__(self, y, observed, drift, par, dt, sigma, tau, mu0, s0, scale_prior=None):
        self.y = torch.as_tensor(y, dtype=torch.float64)
        self.w = torch.as_tensor(observed).to(torch.float64)
        self.T, self.m = int(self.y.shape[0]), int(self.y.shape[1])
        self.drift, self.par = drift, tuple(float(v) for v in par)
        self.dt, self.sigma, self.tau, self.mu0, self.s0 = float(dt), float(sigma), float(tau), float(mu0), float(s0)
        self.prior = None if scale_prior is None else (float(scale_prior[0]), float(scale_prior[1]))
        self.d = self.T * self.m + (2 if self.prior else 0)
        self.dtype = torch.float64

    def cast(self, dtype):
        """The same loop evaluated in `dtype` (states, data and every intermediate): fp32 gives the size of what fp32
        rounding does to U at a state, from the reference alone."""
        import copy
        other = copy.copy(self)
        other.dtype = dtype
        other.y, other.w = self.y.to(dtype), self.w.to(dtype)
        return other

    def __call__(self, x):
        x = x.reshape(x.shape[0], -1).to(self.dtype)
        T, m = self.T, self.m
        if self.prior:
            p, q = x[:, T * m], x[:, T * m + 1]
            sig2, tau2 = torch.exp(2 * p), torch.exp(2 * q)
            loc, c = self.prior
            u = (p - loc) ** 2 / (2 * c * c) + (q - loc) ** 2 / (2 * c * c)
        else:
            p = q = torch.zeros(x.shape[0], dtype=self.dtype)
            sig2 = torch.full_like(p, self.sigma ** 2)
            tau2 = torch.full_like(p, self.tau ** 2)
            u = torch.zeros_like(p)
        prev = None
        for t in range(T):
            X = x[:, t * m:(t + 1) * m]
            if t == 0:
                u = u + ((X - self.mu0) ** 2).sum(1) / (2 * self.s0 ** 2)
            else:
                f = drift64(self.drift, prev, self.par)
                for c in range(m):
                    e = X[:, c] - prev[:, c] - self.dt * f[c]
                    u = u + e * e / (2 * sig2 * self.dt) + (p if self.prior else 0.0)
            for c in range(m):
                if self.w[t, c] != 0:
                    u = u + (X[:, c] - self.y[t, c]) ** 2 / (2 * tau2) + (q if self.prior else 0.0)
            prev = X
        return u

    def grad(self, x):
        t = x.reshape(x.shape[0], -1).double().detach().requires_grad_(True)
        (g,) = torch.autograd.grad(self(t).sum(), t)
        return g

    def hess_diag(self, x):
        """d^2 U / dx_c^2 per coordinate (n, d) in closed form: for X_{t,c}
        [t = 0] / s0^2 + [t >= 1] om + [t < T-1] om (sum_k (delta_kc + dt J_kc(X_t))^2 - dt sum_k e_{t+1,k} d^2 f_k / dx_c^2)
        + rho w_{t,c}; 2 om S_e + 1/c^2 for p and 2 rho S_v + 1/c^2 for q."""
        x = x.reshape(x.shape[0], -1).double().detach()
        n, T, m, dt = x.shape[0], self.T, self.m, self.dt
        if self.prior:
            om = torch.exp(-2 * x[:, T * m]) / dt
            rho = torch.exp(-2 * x[:, T * m + 1])
        else:
            om = torch.full((n,), 1.0 / (self.sigma ** 2 * dt), dtype=torch.float64)
            rho = torch.full((n,), 1.0 / self.tau ** 2, dtype=torch.float64)
        X = x[:, :T * m].reshape(n, T, m)
        hd = torch.zeros_like(x)
        se = torch.zeros(n, dtype=torch.float64)
        for t in range(T):
            Xt = X[:, t]
            for c in range(m):
                v = rho * self.w[t, c] + (om if t >= 1 else 1.0 / self.s0 ** 2)
                hd[:, t * m + c] = v
            if t + 1 < T:
                f = drift64(self.drift, Xt, self.par)
                e = [X[:, t + 1, k] - Xt[:, k] - dt * f[k] for k in range(m)]
                se = se + sum(ek * ek for ek in e)
                J, H2 = self._jac(Xt)
                for c in range(m):
                    col = sum(((1.0 if k == c else 0.0) + dt * J[k][c]) ** 2 for k in range(m))
                    curv = sum(e[k] * H2[k][c] for k in range(m))
                    hd[:, t * m + c] += om * (col - dt * curv)
        if self.prior:
            sv = (self.w * (X - self.y) ** 2).sum((1, 2))
            hd[:, T * m] = 2 * om * se + 1.0 / self.prior[1] ** 2
            hd[:, T * m + 1] = 2 * rho * sv + 1.0 / self.prior[1] ** 2
        return hd

    def _jac(self, X):
        """(J[k][c] = df_k/dx_c, H2[k][c] = d^2 f_k / dx_c^2) at states X (n, m), entries (n,) tensors or numbers"""
        m = self.m
        zero = torch.zeros(X.shape[0], dtype=torch.float64)
        J = [[zero for _ in range(m)] for _ in range(m)]
        H2 = [[zero for _ in range(m)] for _ in range(m)]
        if self.drift == 'cubic':
            alpha, beta = self.par
            for c in range(m):
                J[c][c] = alpha - 3 * beta * X[:, c] ** 2
                H2[c][c] = -6 * beta * X[:, c]
        elif self.drift == 'fitzhugh_nagumo':
            a, b, eps, _cur = self.par
            J[0][0], J[0][1] = 1 - X[:, 0] ** 2, zero - 1
            J[1][0], J[1][1] = zero + eps, zero - eps * b
            H2[0][0] = -2 * X[:, 0]
        else:
            s, r, beta = self.par
            J[0][0], J[0][1] = zero - s, zero + s
            J[1][0], J[1][1], J[1][2] = r - X[:, 2], zero - 1, -X[:, 0]
            J[2][0], J[2][1], J[2][2] = X[:, 1], X[:, 0], zero - beta
        return J, H2


def model_log_density(ref, x):
    """The model's log joint density summed from torch.distributions in fp64, plus the log-Jacobians of p = log sigma and
    q = log tau when the scales are unknown: -U of DiffusionU64 up to one constant."""
    D = torch.distributions
    x = x.reshape(x.shape[0], -1).double()
    T, m = ref.T, ref.m
    X = x[:, :T * m].reshape(-1, T, m)
    one = torch.ones(x.shape[0], dtype=torch.float64)
    lp = torch.zeros_like(one)
    if ref.prior:
        p, q = x[:, T * m], x[:, T * m + 1]
        sigma, tau = torch.exp(p), torch.exp(q)
        ln = D.LogNormal(torch.tensor(ref.prior[0], dtype=torch.float64), torch.tensor(ref.prior[1], dtype=torch.float64))
        lp = lp + ln.log_prob(sigma) + p + ln.log_prob(tau) + q                  # + log |d sigma / dp|, log |d tau / dq|
    else:
        sigma, tau = ref.sigma * one, ref.tau * one
    lp = lp + D.Normal(ref.mu0 * one[:, None], ref.s0 * one[:, None]).log_prob(X[:, 0]).sum(1)
    for t in range(1, T):
        f = torch.stack(drift64(ref.drift, X[:, t - 1], ref.par), dim=-1)
        lp = lp + D.Normal(X[:, t - 1] + ref.dt * f, (sigma * math.sqrt(ref.dt))[:, None]).log_prob(X[:, t]).sum(1)
    obs = D.Normal(X, tau[:, None, None]).log_prob(ref.y[None])
    return lp + (obs * ref.w[None]).sum((1, 2))


def simulate(T, m, drift, par, dt, sigma, tau, mu0, s0, seed):
    """(y (T, m), X (T, m)) fp64 drawn from the model: X_0 ~ N(mu0, s0^2 I), Euler-Maruyama steps, y = X + tau eps."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(2, T, m, generator=g, dtype=torch.float64)
    X = torch.empty(T, m, dtype=torch.float64)
    X[0] = mu0 + s0 * z[0, 0]
    for t in range(1, T):
        f = torch.stack(drift64(drift, X[t - 1], par))
        X[t] = X[t - 1] + dt * f + sigma * math.sqrt(dt) * z[0, t]
    return X + tau * z[1], X


# ------------------------------------------------------------------------------------------------ the tests' problems
# per drift: parameters, dt, sigma, tau, mu0, s0.  The Lorenz problem is the Inference Gym's bridge (om = 1 / (sigma^2 dt)
# = 5000); the cubic one is the double well; FitzHugh-Nagumo at its textbook parameters.
MODELS = {
    'cubic': dict(par=(1.0, 1.0), dt=0.1, sigma=0.7, tau=0.3, mu0=-1.0, s0=0.5),
    'brownian': dict(par=(0.0, 0.0), dt=1.0, sigma=0.1, tau=0.15, mu0=0.0, s0=1.0),
    'ou': dict(par=(-0.5, 0.0), dt=0.2, sigma=0.5, tau=0.4, mu0=0.3, s0=0.8),
    'fitzhugh_nagumo': dict(par=DEFAULT_PARAMS['fitzhugh_nagumo'], dt=0.1, sigma=0.3, tau=0.2, mu0=0.0, s0=1.0),
    'lorenz63': dict(par=DEFAULT_PARAMS['lorenz63'], dt=0.02, sigma=0.1, tau=1.0, mu0=0.0, s0=1.0),
}
SCALE_PRIOR = (-1.0, 0.25)       # of the unknown-scale problems: sigma, tau about 0.37, a quarter either way
COMBOS = [('lorenz63', 3), ('cubic', 1), ('fitzhugh_nagumo', 2), ('cubic', 3), ('ou', 2), ('brownian', 1)]


def drift_name(model):
    return model if model in DRIFT_M else 'cubic'


def problem_data(T, m, model, seed, unknown):
    """A simulated series with about a third of the entries not observed (seeded; the first component of the first step
    always observed, the whole last step never): a dict of what the class and the oracle take."""
    mod = MODELS[model]
    y, X = simulate(T, m, drift_name(model), mod['par'], mod['dt'], mod['sigma'], mod['tau'], mod['mu0'], mod['s0'], seed)
    g = torch.Generator().manual_seed(seed + 1)
    ob = torch.rand(T, m, generator=g) > 0.35
    ob[0, 0] = True
    ob[T - 1] = False
    return dict(y=y, X=X, observed=ob, model=model, unknown=bool(unknown), T=T, m=m)


def make_pair(data, event_shape=None):
    """(package potential, fp64 oracle) of one problem"""
    from nfmc_amd.potentials import DiffusionBridge
    mod = MODELS[data['model']]
    prior = SCALE_PRIOR if data['unknown'] else None
    y = data['y'].clone()
    y[~data['observed']] = float('nan')
    pot = DiffusionBridge(y, drift=drift_name(data['model']), drift_params=mod['par'], dt=mod['dt'],
                          innovation_scale=mod['sigma'], observation_scale=mod['tau'], initial_mean=mod['mu0'],
                          initial_scale=mod['s0'], scale_prior=prior, event_shape=event_shape)
    ref = DiffusionU64(torch.where(data['observed'], data['y'], torch.zeros_like(data['y'])), data['observed'],
                       drift_name(data['model']), mod['par'], mod['dt'], mod['sigma'], mod['tau'], mod['mu0'], mod['s0'], prior)
    return pot, ref


def starts_near_truth(data, pot, n, seed, spread=0.5):
    """n fp64 states about the generating path: X + spread sigma sqrt(dt) eps, and the generating scales times
    e^(0.05 eps) when they are coordinates.  For the long series, where a prior draw wanders far from the data (a
    Brownian path of 1022 steps against observations of scale 0.15) and U is 1e5 and more."""
    mod = MODELS[data['model']]
    g = torch.Generator().manual_seed(seed)
    X = data['X'] + spread * mod['sigma'] * math.sqrt(mod['dt']) * torch.randn((n,) + tuple(data['X'].shape), generator=g,
                                                                               dtype=torch.float64)
    if not data['unknown']:
        return pot.pack(X)
    z = 0.05 * torch.randn(n, 2, generator=g, dtype=torch.float64)
    return pot.pack(X, mod['sigma'] * torch.exp(z[:, 0]), mod['tau'] * torch.exp(z[:, 1]))


def shape_of(d, m, unknown):
    """T of a problem with d coordinates"""
    n = d - (2 if unknown else 0)
    assert n % m == 0 and n // m >= 2, (d, m, unknown)
    return n // m


def step_lambda(ref, x0):
    """the largest entry of the Hessian's diagonal over the starts"""
    return float(ref.hess_diag(x0.double()).abs().max())


def fp32_figure(ref, states):
    """The worst |U(fp32(x)) - U(x)| over the states (k, d) fp64, both in fp64: what rounding the STATE to fp32 does to U,
    whatever the arithmetic behind it.  A kernel that keeps its state in fp32 cannot know U closer than this; measured
    from the reference alone.  (The oracle's loop itself run in fp32, `cast`, is no bound for a kernel: its serial sum
    over t loses 10 to 100 times more than the kernels' lane-parallel sums do.)"""
    x = states.reshape(-1, ref.d).double()
    with torch.no_grad():
        diff = (ref(x.float().double()) - ref(x)).abs()
    return float(diff[torch.isfinite(diff)].max())
