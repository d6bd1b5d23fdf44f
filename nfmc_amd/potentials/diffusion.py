"""The partially observed, discretised diffusion (csrc/pot_diffusion.hpp)."""
import math

import torch

from .. import hip
from ._base import VALU_FAMILIES, Potential, _as_fp64, _check_finite, _event_shape, _finite_fp32, _one_of, _pair, _positive_fp32
from .fullrank import FullRankGaussian


class DiffusionBridge(Potential):
    """The latent path of a stochastic differential equation dX = f(X) dt + sigma dW, discretised by Euler-Maruyama and
    partially observed: T >= 2 time steps, a state X_t in R^m (m = 1, 2 or 3), the step `dt`:

        X_0 ~ N(mu0, s0^2 I),   X_t | X_{t-1} ~ N(X_{t-1} + dt f(X_{t-1}), sigma^2 dt I),   y_{t,c} ~ N(X_{t,c}, tau^2)

    `y` is (T, m) (a (T,) vector is m = 1); a NaN in y, or False in `observed`, marks an entry that is not observed.
    sigma = `innovation_scale`, tau = `observation_scale`, mu0 = `initial_mean`, s0 = `initial_scale`.  With
    `scale_prior=(l, c)` both scales are unknown, p = log sigma and q = log tau with p, q ~ N(l, c^2) (a LogNormal(l, c)
    prior on each; the Inference Gym's is (0, 2)), and `innovation_scale` / `observation_scale` are not used.  The
    coordinates are time-major, x[t m + c] = X_{t,c}, then p and q when the scales are unknown: d = T m or T m + 2.
    With e_t = X_t - X_{t-1} - dt f(X_{t-1}), om = 1 / (sigma^2 dt), rho = 1 / tau^2, S_e = sum_{t>=1} |e_t|^2, S_v the
    sum of (X - y)^2 over the N_o observed entries, constants dropped:

        U = 1/2 |X_0 - mu0|^2 / s0^2 + 1/2 om S_e + 1/2 rho S_v [ + (T-1) m p + N_o q + ((p - l)^2 + (q - l)^2) / (2 c^2) ]

    Drifts (`drift`, parameters `drift_params` as a sequence in the order given, or a dict by name):

        'cubic'            any m, componentwise f_c = alpha x_c - beta x_c^3   (alpha, beta), default (0, 0): Brownian
                           motion; alpha < 0, beta = 0: Ornstein-Uhlenbeck; alpha = beta > 0: the double well
        'fitzhugh_nagumo'  m = 2, f = (x0 - x0^3/3 - x1 + current, epsilon (x0 + a - b x1))
                           (a, b, epsilon, current), default (0.7, 0.8, 0.08, 0.5)
        'lorenz63'         m = 3, f = (s (x1 - x0), x0 (r - x2) - x1, x0 x1 - beta x2)   (s, r, beta), default (10, 28, 8/3)

    This is the centred parameterisation: the states are the coordinates.  (A non-centred one, with the innovations as
    coordinates, needs a sequential pass through time per gradient and is not offered.)  Nothing is clamped.  Validated in
    fp64 on the host: y, the scales, dt and the parameters finite in fp32 too, the scales and dt > 0, T >= 2, m fitting the
    drift.  The fused kernels evaluate it in the mcmc, flow-MH and NeuTra launch families (NeuTra on its VALU kernels,
    conditioners of at most 32 units) for d <= 1024; anything else runs on the split or composed path like any callable
    (`fused_in`).  It is never inferred from a plain callable: pass the object as the target.  N(0, I) starts sit far in
    the tails (U ~ 1e5 for the Lorenz preset): start from `prior_draws`."""

    neutra_matrix_cores = False
    fused_families, fused_max_dim = VALU_FAMILIES, 1024
    DRIFTS = ('cubic', 'fitzhugh_nagumo', 'lorenz63')
    DRIFT_DIMS = {'cubic': (1, 2, 3), 'fitzhugh_nagumo': (2,), 'lorenz63': (3,)}
    DRIFT_PARAMS = {'cubic': ('alpha', 'beta'), 'fitzhugh_nagumo': ('a', 'b', 'epsilon', 'current'),
                    'lorenz63': ('s', 'r', 'beta')}
    DRIFT_DEFAULTS = {'cubic': (0.0, 0.0), 'fitzhugh_nagumo': (0.7, 0.8, 0.08, 0.5), 'lorenz63': (10.0, 28.0, 8.0 / 3.0)}

    def __init__(self, y, observed=None, drift='lorenz63', drift_params=None, dt=0.02, innovation_scale=0.1,
                 observation_scale=1.0, initial_mean=0.0, initial_scale=1.0, scale_prior=None, event_shape=None):
        _one_of('drift', drift, self.DRIFTS)
        yv = _as_fp64(y)
        if yv.dim() == 1:
            yv = yv[:, None]
        if yv.dim() != 2 or yv.shape[0] < 2 or yv.shape[1] < 1:
            raise ValueError('y must be (T, m) or (T,) with T >= 2 time steps, got shape %s' % (tuple(yv.shape),))
        T, m = int(yv.shape[0]), int(yv.shape[1])
        if m not in self.DRIFT_DIMS[drift]:
            raise ValueError('drift %r needs m in %s, got m = %d' % (drift, self.DRIFT_DIMS[drift], m))
        ob = ~torch.isnan(yv)
        if observed is not None:
            o = torch.as_tensor(observed).detach().to('cpu')
            if o.dim() == 1:
                o = o[:, None]
            if o.dtype != torch.bool or tuple(o.shape) != (T, m):
                raise ValueError('observed must be a bool mask of shape %s, got %s of shape %s'
                                 % ((T, m), o.dtype, tuple(o.shape)))
            ob = ob & o
        yv = torch.where(ob, yv, torch.zeros_like(yv))          # an unobserved entry's y is never read
        _check_finite(yv, 'the observed entries of y must be finite (in fp32 too: the kernels read an fp32 copy)')
        names = self.DRIFT_PARAMS[drift]
        if drift_params is None:
            par = self.DRIFT_DEFAULTS[drift]
        elif isinstance(drift_params, dict):
            if set(drift_params) - set(names):
                raise ValueError('drift %r takes the parameters %s, got %s' % (drift, names, sorted(drift_params)))
            par = tuple(drift_params.get(k, v) for k, v in zip(names, self.DRIFT_DEFAULTS[drift]))
        else:
            par = tuple(drift_params)
            if len(par) != len(names):
                raise ValueError('drift %r takes the %d parameters %s, got %d' % (drift, len(names), names, len(par)))
        self.drift_params = tuple(_finite_fp32('drift parameter %s' % k, v) for k, v in zip(names, par))
        self.dt = _positive_fp32('dt', dt)
        self.initial_mean = _finite_fp32('initial_mean', initial_mean)
        self.initial_scale = _positive_fp32('initial_scale', initial_scale)
        self.scales_unknown = scale_prior is not None
        self.prior_loc, self.prior_scale = 0.0, 1.0
        if self.scales_unknown:
            loc, sc = _pair(scale_prior, 'scale_prior', '(l, c)')
            self.prior_loc = _finite_fp32('the location l of scale_prior', loc)
            self.prior_scale = _positive_fp32('the scale c of scale_prior', sc)
            _positive_fp32('1 / c^2 of scale_prior', 1.0 / self.prior_scale ** 2)
            self.innovation_scale = self.observation_scale = 1.0
        else:
            self.innovation_scale = _positive_fp32('innovation_scale', innovation_scale)
            self.observation_scale = _positive_fp32('observation_scale', observation_scale)
            _positive_fp32('1 / (innovation_scale^2 dt)', 1.0 / (self.innovation_scale ** 2 * self.dt))
            _positive_fp32('1 / observation_scale^2', 1.0 / self.observation_scale ** 2)
        _positive_fp32('1 / initial_scale^2', 1.0 / self.initial_scale ** 2)
        d = T * m + (2 if self.scales_unknown else 0)
        self.event_shape = _event_shape(event_shape, d, ' (T m states, log sigma and log tau)' if self.scales_unknown else '')
        self.dim = d
        self.drift = drift
        self.T, self.m = T, m
        self.y = yv.contiguous()                 # fp64 masters; the kernels get fp32
        self.observed = ob.contiguous()
        self.n_observed = int(ob.sum())
        self._dev = {}

    # ------------------------------------------------------------------ presets
    @classmethod
    def synthetic(cls, n_steps, drift, seed, observed=None, **model):
        """(potential, truth): a path simulated from the model itself (X_0 ~ N(mu0, s0^2 I), Euler-Maruyama steps; with
        `scale_prior` the generating scales are the model's `innovation_scale` / `observation_scale` all the same) and
        observed with noise on the entries of the bool mask `observed` ((T, m); everything when None); all draws in
        fp64 from one CPU torch.Generator seeded with `seed`.  `model`: the constructor's keywords.  `truth` is the
        generating state in the object's coordinates (d,), fp64."""
        T = int(n_steps)
        m = int(model.pop('m', cls.DRIFT_DIMS[drift][0] if drift in cls.DRIFT_DIMS else 1))
        proto = cls(torch.zeros(max(T, 2), m), drift=drift, **model)         # validates the model
        if T < 2:
            raise ValueError('n_steps must be >= 2, got %r' % (n_steps,))
        sig = _positive_fp32('innovation_scale', model.get('innovation_scale', 0.1))
        tau = _positive_fp32('observation_scale', model.get('observation_scale', 1.0))
        g = torch.Generator().manual_seed(int(seed))
        X = torch.empty(T, m, dtype=torch.float64)
        X[0] = proto.initial_mean + proto.initial_scale * torch.randn(m, generator=g, dtype=torch.float64)
        for t in range(1, T):
            X[t] = X[t - 1] + proto.dt * proto._drift(X[t - 1]) + sig * math.sqrt(proto.dt) * torch.randn(
                m, generator=g, dtype=torch.float64)
        y = X + tau * torch.randn(T, m, generator=g, dtype=torch.float64)
        pot = cls(y, observed=observed, drift=drift, **model)
        return pot, (pot.pack(X, sig, tau) if pot.scales_unknown else pot.pack(X))

    @staticmethod
    def _preset_model(model, unknown_scales):
        model = dict(model)
        if unknown_scales:
            model.setdefault('scale_prior', (0.0, 2.0))
        return model

    @classmethod
    def brownian_motion(cls, n_steps=30, unknown_scales=False, seed=0, **model):
        """The Inference Gym's BrownianMotionMissingMiddleObservations: m = 1, zero drift, dt = 1, innovation scale 0.1
        and observation scale 0.15 unless given, the middle third of the steps not observed; data simulated with
        `seed`.  `unknown_scales`: both scales with the LogNormal(0, 2) prior.  Returns the potential."""
        T = int(n_steps)
        model = cls._preset_model(model, unknown_scales)
        model.setdefault('dt', 1.0)
        model.setdefault('innovation_scale', 0.1)
        model.setdefault('observation_scale', 0.15)
        ob = torch.ones(max(T, 2), 1, dtype=torch.bool)
        ob[T // 3:T - T // 3] = False
        return cls.synthetic(T, 'cubic', seed, observed=ob[:T], m=1, drift_params=(0.0, 0.0), **model)[0]

    @classmethod
    def lorenz_bridge(cls, n_steps=30, dt=0.02, unknown_scales=False, seed=0, **model):
        """The Inference Gym's ConvectionLorenzBridge: m = 3, the Lorenz-63 drift, innovation scale 0.1 and observation
        scale 1 unless given, the FIRST component observed on the first and the last ten steps (a third of the steps
        at each end when n_steps < 30); the path starts about the origin, X_0 ~ N(0, I) unless `initial_mean` /
        `initial_scale` are given.  Data simulated with `seed`."""
        T = int(n_steps)
        model = cls._preset_model(model, unknown_scales)
        k = 10 if T >= 30 else max(T // 3, 1)
        ob = torch.zeros(max(T, 2), 3, dtype=torch.bool)
        ob[:k, 0] = True
        ob[T - k:, 0] = True
        return cls.synthetic(T, 'lorenz63', seed, observed=ob[:T], dt=dt, **model)[0]

    @classmethod
    def double_well_path(cls, n_steps=64, unknown_scales=False, seed=0, **model):
        """The double-well transition path: m = 1, f = x - x^3 (alpha = beta = 1), only the two end points observed, at
        -1 and +1 (observation scale 0.1, innovation scale 0.7, dt = 0.1 unless given).  `seed` is not used (the data
        are the two end points); kept for a uniform signature."""
        T = int(n_steps)
        if T < 2:
            raise ValueError('n_steps must be >= 2, got %r' % (n_steps,))
        model = cls._preset_model(model, unknown_scales)
        model.setdefault('dt', 0.1)
        model.setdefault('innovation_scale', 0.7)
        model.setdefault('observation_scale', 0.1)
        model.setdefault('initial_mean', -1.0)
        y = torch.full((T,), float('nan'), dtype=torch.float64)
        y[0], y[-1] = -1.0, 1.0
        return cls(y, drift='cubic', drift_params=(1.0, 1.0), **model)

    # ------------------------------------------------------------------ helpers
    def paths(self, x):
        """The states X (..., T, m) of the coordinates x."""
        xf = self._flat(x)
        return xf[..., :self.T * self.m].reshape(xf.shape[:-1] + (self.T, self.m))

    def scales(self, x):
        """(sigma, tau), each (...,): the fixed scales, or e^p and e^q of the coordinates when they are unknown."""
        xf = self._flat(x)
        if not self.scales_unknown:
            return (torch.full(xf.shape[:-1], self.innovation_scale, dtype=xf.dtype, device=xf.device),
                    torch.full(xf.shape[:-1], self.observation_scale, dtype=xf.dtype, device=xf.device))
        n = self.T * self.m
        return torch.exp(xf[..., n]), torch.exp(xf[..., n + 1])

    def pack(self, paths, innovation_scale=None, observation_scale=None):
        """The coordinates x (..., d) of paths (..., T, m) (or (..., T) when m = 1) and, when the scales are unknown,
        of sigma and tau (numbers or (...,); both needed).  Inverse of `paths` / `scales`."""
        X = torch.as_tensor(paths)
        if self.m == 1 and X.shape[-1:] == (self.T,) and X.shape[-2:] != (self.T, 1):
            X = X[..., None]
        if X.shape[-2:] != (self.T, self.m):
            raise ValueError('paths must end in (T, m) = %s, got shape %s' % ((self.T, self.m), tuple(X.shape)))
        if not X.is_floating_point():
            X = X.to(torch.get_default_dtype())
        head = X.reshape(X.shape[:-2] + (self.T * self.m,))
        if not self.scales_unknown:
            if innovation_scale is not None or observation_scale is not None:
                raise ValueError('the scales are fixed (no scale_prior): pack takes none')
            return head
        if innovation_scale is None or observation_scale is None:
            raise ValueError('the scales are coordinates: pack needs innovation_scale and observation_scale')
        sig, tau = (torch.as_tensor(v).to(head).expand(head.shape[:-1]) for v in (innovation_scale, observation_scale))
        if not bool((sig > 0).all()) or not bool((tau > 0).all()):
            raise ValueError('the scales must be positive')
        return torch.cat([head, torch.log(sig)[..., None], torch.log(tau)[..., None]], dim=-1)

    def prior_draws(self, n, seed):
        """n draws from the prior in coordinate form, (n, d) fp64 on the CPU: the scales from their LogNormal prior when
        unknown, X_0 ~ N(mu0, s0^2 I), then Euler-Maruyama steps; one CPU torch.Generator seeded with `seed`.  These
        are the starts to use: N(0, I) starts sit far in the tails of a stiff bridge."""
        n = int(n)
        if n < 1:
            raise ValueError('n must be >= 1, got %r' % (n,))
        g = torch.Generator().manual_seed(int(seed))
        if self.scales_unknown:
            ls = self.prior_loc + self.prior_scale * torch.randn(n, 2, generator=g, dtype=torch.float64)
            sig = torch.exp(ls[:, 0])
        else:
            sig = torch.full((n,), self.innovation_scale, dtype=torch.float64)
        z = torch.randn(n, self.T, self.m, generator=g, dtype=torch.float64)
        X = torch.empty(n, self.T, self.m, dtype=torch.float64)
        X[:, 0] = self.initial_mean + self.initial_scale * z[:, 0]
        for t in range(1, self.T):
            X[:, t] = X[:, t - 1] + self.dt * self._drift(X[:, t - 1]) + (sig * math.sqrt(self.dt))[:, None] * z[:, t]
        head = X.reshape(n, -1)
        return torch.cat([head, ls], dim=1) if self.scales_unknown else head

    def gaussian(self):
        """The equivalent FullRankGaussian (the same U up to a constant; a block-tridiagonal precision) when the model is
        linear and its scales are fixed: drift 'cubic' with beta = 0.  ValueError otherwise."""
        if self.drift != 'cubic' or self.drift_params[1] != 0.0 or self.scales_unknown:
            raise ValueError("gaussian() needs the drift 'cubic' with beta = 0 and fixed scales: anything else is not Gaussian")
        T, m, n = self.T, self.m, self.T * self.m
        a = 1.0 + self.dt * self.drift_params[0]
        om, rho = 1.0 / (self.innovation_scale ** 2 * self.dt), 1.0 / self.observation_scale ** 2
        P = torch.zeros(n, n, dtype=torch.float64)
        idx = torch.arange(n)
        w = self.observed.to(torch.float64).reshape(-1)
        P[idx, idx] = rho * w
        P[idx[:m], idx[:m]] += 1.0 / self.initial_scale ** 2
        P[idx[m:], idx[m:]] += om
        P[idx[:-m], idx[:-m]] += om * a * a
        P[idx[m:], idx[:-m]] -= om * a
        P[idx[:-m], idx[m:]] -= om * a
        b = rho * w * self.y.reshape(-1)
        b[:m] += self.initial_mean / self.initial_scale ** 2
        return FullRankGaussian(torch.linalg.solve(P, b), precision=P, event_shape=self.event_shape)

    # ------------------------------------------------------------------ evaluation in torch ops
    def _drift(self, X):
        """f(X) of states X (..., m), in torch ops"""
        p = self.drift_params
        if self.drift == 'cubic':
            return p[0] * X - p[1] * X ** 3
        if self.drift == 'fitzhugh_nagumo':
            x0, x1 = X[..., 0], X[..., 1]
            return torch.stack([x0 - x0 ** 3 / 3.0 - x1 + p[3], p[2] * (x0 + p[0] - p[1] * x1)], dim=-1)
        x0, x1, x2 = X[..., 0], X[..., 1], X[..., 2]
        return torch.stack([p[0] * (x1 - x0), x0 * (p[1] - x2) - x1, x0 * x1 - p[2] * x2], dim=-1)

    def _copy(self, device, dtype=torch.float32):
        return self._cached((str(device), dtype), lambda: (self.y.to(device, dtype).contiguous(),
                                                           self.observed.to(device, dtype).contiguous()))

    def __call__(self, x):
        """U (n_chains,) of states x (n_chains, ...) in differentiable torch ops."""
        xf = x.reshape(x.shape[0], -1)
        y, w = self._copy(xf.device, xf.dtype)
        T, m = self.T, self.m
        X = xf[:, :T * m].reshape(-1, T, m)
        e = X[:, 1:] - X[:, :-1] - self.dt * self._drift(X[:, :-1])
        se = torch.sum(e * e, dim=(1, 2))
        sv = torch.sum(w * (X - y) ** 2, dim=(1, 2))
        u0 = 0.5 * torch.sum((X[:, 0] - self.initial_mean) ** 2, dim=1) / self.initial_scale ** 2
        if not self.scales_unknown:
            return (u0 + 0.5 * se / (self.innovation_scale ** 2 * self.dt) + 0.5 * sv / self.observation_scale ** 2)
        p, q = xf[:, T * m], xf[:, T * m + 1]
        c2 = self.prior_scale ** 2
        return (u0 + 0.5 * torch.exp(-2.0 * p) * se / self.dt + 0.5 * torch.exp(-2.0 * q) * sv + (T - 1) * m * p
                + self.n_observed * q + 0.5 * ((p - self.prior_loc) ** 2 + (q - self.prior_loc) ** 2) / c2)

    # ------------------------------------------------------------------ the kernels' view
    def code(self):
        """a_scalar of the descriptor: drift code + 4 [scales unknown] + 8 (m - 1)."""
        return float(self.DRIFTS.index(self.drift) + (4 if self.scales_unknown else 0) + 8 * (self.m - 1))

    def data_block(self):
        """The kernels' view (NFMC_POT_DIFFUSION_BRIDGE, include/nfmc_hip.h), fp32 on the CPU: (header, rows).  Header: 16
        floats (dt, sigma, tau, mu0, 1/s0^2, l, 1/c^2, N_o, (T-1) m, four drift parameters, 0, 0, 0).  Rows (2, n4),
        n4 = 4 ceil(T m / 4): y and w (1 observed, 0 not), time-major, zero past T m."""
        n = self.T * self.m
        n4 = 4 * ((n + 3) // 4)
        par = self.drift_params + (0.0,) * (4 - len(self.drift_params))
        head = torch.tensor([self.dt, self.innovation_scale, self.observation_scale, self.initial_mean,
                             1.0 / self.initial_scale ** 2, self.prior_loc, 1.0 / self.prior_scale ** 2,
                             float(self.n_observed), float((self.T - 1) * self.m)] + list(par) + [0.0, 0.0, 0.0],
                            dtype=torch.float64)
        rows = torch.zeros(2, n4, dtype=torch.float64)
        rows[0, :n] = self.y.reshape(-1)
        rows[1, :n] = self.observed.to(torch.float64).reshape(-1)
        return head.to(torch.float32), rows.to(torch.float32)

    def descriptor(self, device):
        head, rows = self._descriptor_blocks(device)
        return hip.NfmcPotential(hip.POT_DIFFUSION_BRIDGE, self.T, hip.ptr(head), hip.ptr(rows), self.code(), 0.0)
