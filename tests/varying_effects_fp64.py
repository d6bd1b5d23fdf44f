"""fp64 restatement of the varying-effects regression (potentials.VaryingEffectsRegression), for the host and GPU tests.
Everything here works on the raw observations (y_i, x_i, g_i, sigma_i), never on the per-group sufficient statistics the
class and the kernels use, and nothing here uses the class: the model's log densities from torch.distributions
(`model_u64`), a fast U and gradient for the oracle samplers (`VFX64`), a diagonal Hessian for the mass diagonals and
start states.

Coordinates (the public layout): the group block -- [a_0, b_0, a_1, b_1, ...] when both sides vary, [v_0 .. v_{C-1}] when
one does -- then the globals that exist: mu_a, s_a or a; mu_b, s_b or b; s_y."""
import torch


class VFX64:
    """U(x) in fp64 over the observations, constants dropped.  y, group (and x unless slopes == 'none') are (N,);
    noise_scale None (unknown noise) or a scalar or (N,) of known scales."""

    def __init__(self, y, group, x=None, intercepts='varying', slopes='none', noise_scale=None, centered=True,
                 location_scale=10.0, scale_scale=1.0):
        self.y = torch.as_tensor(y).double().reshape(-1)
        self.g = torch.as_tensor(group).long().reshape(-1)
        self.N = self.y.numel()
        self.C = int(self.g.max()) + 1
        self.x = torch.zeros_like(self.y) if slopes == 'none' else torch.as_tensor(x).double().reshape(-1)
        self.ia, self.sl, self.centered = intercepts, slopes, bool(centered)
        self.known = noise_scale is not None
        self.sig = torch.as_tensor(noise_scale).double().expand(self.N).clone() if self.known else None
        self.m, self.h = float(location_scale), float(scale_scale)
        self.both = intercepts == 'varying' and slopes == 'varying'
        self.gb = 2 * self.C if self.both else self.C
        self.names = ((['mu_a', 's_a'] if intercepts == 'varying' else ['a'])
                      + {'varying': ['mu_b', 's_b'], 'shared': ['b'], 'none': []}[slopes] + ([] if self.known else ['s_y']))
        self.d = self.gb + len(self.names)

    def parts(self, x):
        """dict: the raw group coordinates 'a' / 'b' (n, C) of the varying sides and every global (n,)"""
        x = x.reshape(x.shape[0], -1).double()
        out = {}
        if self.both:
            out['a'], out['b'] = x[:, 0:self.gb:2], x[:, 1:self.gb:2]
        else:
            out['a' if self.ia == 'varying' else 'b'] = x[:, :self.gb]
        for k, name in enumerate(self.names):
            out[name] = x[:, self.gb + k]
        return out

    def natural(self, p):
        """(a, b) each (n, C) on the natural scale"""
        n = next(iter(p.values())).shape[0]
        res = []
        for side, mode in (('a', self.ia), ('b', self.sl)):
            if mode == 'varying':
                v = p[side]
                res.append(v if self.centered else p['mu_' + side][:, None] + torch.exp(p['s_' + side])[:, None] * v)
            elif mode == 'shared':
                res.append(p[side][:, None].expand(n, self.C))
            else:
                res.append(torch.zeros(n, self.C, dtype=torch.float64))
        return res

    def _omega(self, p):
        """(n, N) or (1, N) observation weights 1 / sigma_i^2"""
        if self.known:
            return (self.sig ** -2)[None, :]
        return torch.exp(-2 * p['s_y'])[:, None].expand(-1, self.N)

    def __call__(self, x):
        p = self.parts(x)
        a, b = self.natural(p)
        res = self.y[None, :] - a[:, self.g] - b[:, self.g] * self.x[None, :]
        u = 0.5 * (self._omega(p) * res * res).sum(1)
        P, Hh = self.m ** -2, self.h ** -2
        if not self.known:
            sy = p['s_y']
            u = u + self.N * sy + 0.5 * Hh * torch.exp(2 * sy) - sy
        for side, mode in (('a', self.ia), ('b', self.sl)):
            if mode == 'varying':
                mu, s, v = p['mu_' + side], p['s_' + side], p[side]
                if self.centered:
                    u = u + self.C * s + 0.5 * torch.exp(-2 * s) * ((v - mu[:, None]) ** 2).sum(1)
                else:
                    u = u + 0.5 * (v * v).sum(1)
                u = u + 0.5 * P * mu * mu + 0.5 * Hh * torch.exp(2 * s) - s
            elif mode == 'shared':
                u = u + 0.5 * P * p[side] ** 2
        return u

    def _put(self, out, name, val):
        if name in ('a', 'b') and val.dim() == 2:
            if self.both:
                out[:, (0 if name == 'a' else 1):self.gb:2] = val
            else:
                out[:, :self.gb] = val
        else:
            out[:, self.gb + self.names.index(name)] = val

    def grad(self, x):
        """dU/dx written out over the observations (no autograd)"""
        x = x.reshape(x.shape[0], -1).double()
        n = x.shape[0]
        p = self.parts(x)
        a, b = self.natural(p)
        om = self._omega(p)
        res = self.y[None, :] - a[:, self.g] - b[:, self.g] * self.x[None, :]
        zero = torch.zeros(n, self.C, dtype=torch.float64)
        gnat = {'a': zero.index_add(1, self.g, (-om * res).expand(n, -1)),
                'b': zero.index_add(1, self.g, (-om * res * self.x[None, :]).expand(n, -1))}
        P, Hh = self.m ** -2, self.h ** -2
        out = torch.zeros_like(x)
        if not self.known:
            sy = p['s_y']
            self._put(out, 's_y', self.N - (om * res * res).sum(1) + Hh * torch.exp(2 * sy) - 1)
        for side, mode in (('a', self.ia), ('b', self.sl)):
            gv = gnat[side]
            if mode == 'varying':
                mu, s, v = p['mu_' + side], p['s_' + side], p[side]
                if self.centered:
                    w, r = torch.exp(-2 * s), v - mu[:, None]
                    self._put(out, side, gv + w[:, None] * r)
                    self._put(out, 'mu_' + side, P * mu - w * r.sum(1))
                    self._put(out, 's_' + side, self.C - w * (r * r).sum(1) + Hh * torch.exp(2 * s) - 1)
                else:
                    es = torch.exp(s)
                    self._put(out, side, es[:, None] * gv + v)
                    self._put(out, 'mu_' + side, P * mu + gv.sum(1))
                    self._put(out, 's_' + side, es * (gv * v).sum(1) + Hh * torch.exp(2 * s) - 1)
            elif mode == 'shared':
                self._put(out, side, P * p[side] + gv.sum(1))
        return out

    def hess_diag(self, x):
        """A positive diagonal for the mass matrices: d^2 U / dx_c^2 with the one indefinite term dropped (for a
        non-centered log scale, e^s sum_c gV_c t_c, which has either sign)."""
        x = x.reshape(x.shape[0], -1).double()
        n = x.shape[0]
        p = self.parts(x)
        a, b = self.natural(p)
        om = self._omega(p)
        res = self.y[None, :] - a[:, self.g] - b[:, self.g] * self.x[None, :]
        zero = torch.zeros(n, self.C, dtype=torch.float64)
        hnat = {'a': zero.index_add(1, self.g, om.expand(n, -1)),
                'b': zero.index_add(1, self.g, (om * self.x[None, :] ** 2).expand(n, -1))}
        P, Hh = self.m ** -2, self.h ** -2
        out = torch.zeros_like(x)
        if not self.known:
            self._put(out, 's_y', 2 * (om * res * res).sum(1) + 2 * Hh * torch.exp(2 * p['s_y']))
        for side, mode in (('a', self.ia), ('b', self.sl)):
            hv = hnat[side]
            if mode == 'varying':
                mu, s, v = p['mu_' + side], p['s_' + side], p[side]
                if self.centered:
                    w, r = torch.exp(-2 * s), v - mu[:, None]
                    self._put(out, side, hv + w[:, None])
                    self._put(out, 'mu_' + side, P + self.C * w)
                    self._put(out, 's_' + side, 2 * w * (r * r).sum(1) + 2 * Hh * torch.exp(2 * s))
                else:
                    e2 = torch.exp(2 * s)
                    self._put(out, side, e2[:, None] * hv + 1)
                    self._put(out, 'mu_' + side, P + hv.sum(1))
                    self._put(out, 's_' + side, e2 * (hv * v * v).sum(1) + 2 * Hh * e2)
            elif mode == 'shared':
                self._put(out, side, P + hv.sum(1))
        return out


def model_u64(x, y, group, xcov=None, intercepts='varying', slopes='none', noise_scale=None, centered=True,
              location_scale=10.0, scale_scale=1.0):
    """The model's negative log joint from torch.distributions in fp64 over the raw observations: Normal and HalfNormal
    priors (a scale's log is the coordinate: + s for the Jacobian), Normal likelihood.  U up to one constant.  Argument
    validation is off, so a non-finite state gives a non-finite U for its own row instead of an error for the batch."""
    dist = torch.distributions
    ref = VFX64(y, group, xcov, intercepts, slopes, noise_scale, centered, location_scale, scale_scale)
    p = ref.parts(x)
    n = x.shape[0]
    m, h = float(location_scale), float(scale_scale)

    def normal(v, mean, scale):
        return dist.Normal(mean, scale, validate_args=False).log_prob(v)

    def half_normal_log(s):   # log density of s = log sigma, sigma ~ HalfNormal(h)
        return dist.HalfNormal(torch.full_like(s, h), validate_args=False).log_prob(torch.exp(s)) + s
    lp = torch.zeros(n, dtype=torch.float64)
    nat = {}
    for side, mode in (('a', intercepts), ('b', slopes)):
        if mode == 'varying':
            mu, s, v = p['mu_' + side], p['s_' + side], p[side]
            lp = lp + normal(mu, torch.zeros_like(mu), torch.full_like(mu, m)) + half_normal_log(s)
            if centered:
                lp = lp + normal(v, mu[:, None].expand_as(v), torch.exp(s)[:, None].expand_as(v)).sum(1)
                nat[side] = v
            else:
                lp = lp + normal(v, torch.zeros_like(v), torch.ones_like(v)).sum(1)
                nat[side] = mu[:, None] + torch.exp(s)[:, None] * v
        elif mode == 'shared':
            v = p[side]
            lp = lp + normal(v, torch.zeros_like(v), torch.full_like(v, m))
            nat[side] = v[:, None].expand(n, ref.C)
        else:
            nat[side] = torch.zeros(n, ref.C, dtype=torch.float64)
    if noise_scale is None:
        lp = lp + half_normal_log(p['s_y'])
        sig = torch.exp(p['s_y'])[:, None].expand(n, ref.N)
    else:
        sig = ref.sig[None, :].expand(n, ref.N)
    mean = nat['a'][:, ref.g] + nat['b'][:, ref.g] * ref.x[None, :]
    lp = lp + normal(ref.y[None, :].expand(n, ref.N), mean, sig).sum(1)
    return -lp


def start_states(ref, truth, n, seed):
    """n fp64 states (n, d): the generating state plus N(0, 1) / sqrt(hess_diag(truth)) per coordinate -- about one
    posterior standard deviation around it -- rounded through fp32.  `ref` is a VFX64."""
    g = torch.Generator().manual_seed(seed)
    truth = torch.as_tensor(truth).double().reshape(1, -1)
    sd = 1 / torch.sqrt(ref.hess_diag(truth))
    x = truth + torch.randn(n, truth.shape[1], generator=g, dtype=torch.float64) * sd
    return x.float().double()
