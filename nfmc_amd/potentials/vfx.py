"""Gaussian regression with varying (group-level) effects (csrc/pot_vfx.hpp)."""
import torch

from .. import hip
from ._base import VALU_FAMILIES, Potential, _check_finite, _positive_fp32


class VaryingEffectsRegression(Potential):
    """Gaussian regression with group-level (varying) effects: the radon models (varying intercepts, varying slopes,
    both) and eight schools, the textbook funnel between a group-level scale and its group effects.  Observation i has a
    response y_i, an optional covariate x_i and a group g_i in 0 .. C-1 (`group`, integers, no empty group):

        y_i ~ N(a[g_i] + b[g_i] x_i, sigma_i^2)

    `intercepts` is 'varying' (a_c ~ N(mu_a, sigma_a^2), mu_a ~ N(0, m^2), sigma_a ~ HalfNormal(h)) or 'shared' (one
    a ~ N(0, m^2)); `slopes` is 'varying', 'shared' or 'none' (b = 0, x unused); at least one side varies.
    `noise_scale=None` is the unknown noise sigma_i = sigma_y ~ HalfNormal(h); a positive scalar or (N,) array gives known
    scales and no noise coordinate.  m = `location_scale`, h = `scale_scale`.  Scales are sampled as logs s = log sigma,
    Jacobian included.  `centered=True`: the group coordinates are a_c, b_c themselves; `centered=False`: standardised
    t_c ~ N(0, 1) with a_c = mu_a + e^{s_a} t_c (`effects` gives the natural scale in either case).

    Coordinates (`unpack` / `pack` convert): the group block, [a_0, b_0, a_1, b_1, ...] when both sides vary and
    [v_0 .. v_{C-1}] when one does; then the globals that exist, in this order: mu_a, s_a or a; mu_b, s_b or b; s_y.
    d = 2 C + 5 for radon "both", C + 4 for "intercepts" or "slopes", C + 2 for eight schools.

    The likelihood enters through six statistics per group, formed in fp64 with weights omega_i = 1 / sigma_i^2 (1 when
    the noise is unknown): n_c = sum omega, the weighted means xbar_c, ybar_c and the centred weighted sums Sxx_c, Sxy_c,
    Syy_c, so an evaluation costs O(d), not O(N).  With P = 1 / m^2, Hh = 1 / h^2, w_y = e^{-2 s_y} (1 when known) and
    e_c = ybar_c - a_c - b_c xbar_c, constants dropped:

        Q_c = n_c e_c^2 + Syy_c - 2 b_c Sxy_c + b_c^2 Sxx_c
        U = 1/2 w_y sum_c Q_c  [+ N s_y + 1/2 Hh e^{2 s_y} - s_y]
            + per varying side:  centered      C s + 1/2 e^{-2s} sum (v_c - mu)^2 + 1/2 P mu^2 + 1/2 Hh e^{2s} - s
                                 non-centered  1/2 sum t_c^2 + 1/2 P mu^2 + 1/2 Hh e^{2s} - s
            + per shared side:   1/2 P v^2

    Validated in fp64 on the host (ValueError): y, group, x 1-D of equal length N >= 1 and finite; group integers
    0 .. C-1 with no empty group; x required unless slopes='none'; one side varying; noise_scale positive; both scales and
    their inverse squares positive and finite in fp32; the table finite in fp32.  d is not capped: the fused kernels
    evaluate the model in the mcmc, flow-MH and NeuTra launch families (NeuTra on its VALU kernels, conditioners of at
    most 32 units) for d <= 1024, and a larger model, and every other family, runs on the split or composed path like
    any callable (`fused_in`).  It is never inferred from a plain callable: pass the object as the target."""

    neutra_matrix_cores = False
    fused_families, fused_max_dim = VALU_FAMILIES, 1024
    MODES = {'none': 0, 'shared': 1, 'varying': 2}

    def __init__(self, y, group, x=None, intercepts='varying', slopes='none', noise_scale=None, centered=True,
                 location_scale=10.0, scale_scale=1.0):
        if intercepts not in ('varying', 'shared'):
            raise ValueError("intercepts must be 'varying' or 'shared', got %r" % (intercepts,))
        if slopes not in ('varying', 'shared', 'none'):
            raise ValueError("slopes must be 'varying', 'shared' or 'none', got %r" % (slopes,))
        if intercepts != 'varying' and slopes != 'varying':
            raise ValueError('at least one of intercepts and slopes must be varying')
        if not isinstance(centered, bool):
            raise ValueError('centered must be a bool, got %r' % (centered,))
        yv = torch.as_tensor(y).detach().to('cpu', torch.float64)
        if yv.dim() != 1 or yv.numel() < 1:
            raise ValueError('y must be 1-D with N >= 1 entries, got shape %s' % (tuple(yv.shape),))
        N = yv.numel()
        gv = torch.as_tensor(group).detach().to('cpu')
        if gv.dim() != 1 or gv.numel() != N:
            raise ValueError('group must be 1-D with N = %d entries, got shape %s' % (N, tuple(gv.shape)))
        if gv.dtype == torch.bool or gv.is_complex():
            raise ValueError('group must hold integers, got %s' % gv.dtype)
        if gv.is_floating_point():
            if not bool(torch.isfinite(gv).all()) or not bool((gv == gv.round()).all()):
                raise ValueError('group must hold integers')
        gv = gv.to(torch.int64)
        if int(gv.min()) < 0:
            raise ValueError('group must hold integers 0 .. C-1, got %d' % int(gv.min()))
        C = int(gv.max()) + 1
        counts = torch.bincount(gv, minlength=C)
        if not bool((counts > 0).all()):
            raise ValueError('group must use every label 0 .. C-1 = %d: group %d is empty' % (C - 1, int((counts == 0).nonzero()[0])))
        if slopes == 'none':
            xv = torch.zeros_like(yv)
        else:
            if x is None:
                raise ValueError("x is required unless slopes='none'")
            xv = torch.as_tensor(x).detach().to('cpu', torch.float64)
            if xv.dim() != 1 or xv.numel() != N:
                raise ValueError('x must be 1-D with N = %d entries, got shape %s' % (N, tuple(xv.shape)))
        if not bool(torch.isfinite(yv).all()) or not bool(torch.isfinite(xv).all()):
            raise ValueError('y and x must be finite')
        if noise_scale is None:
            sig = None
            om = torch.ones_like(yv)
        else:
            sig = torch.as_tensor(noise_scale).detach().to('cpu', torch.float64)
            if sig.dim() == 0:
                sig = sig.expand(N)
            if sig.dim() != 1 or sig.numel() != N:
                raise ValueError('noise_scale must be a scalar or have N = %d entries, got shape %s' % (N, tuple(sig.shape)))
            if not bool((torch.isfinite(sig) & (sig > 0)).all()):
                raise ValueError('noise_scale must be > 0 and finite')
            sig = sig.contiguous()
            om = sig ** -2
        self.location_scale = _positive_fp32('location_scale', location_scale)
        self.scale_scale = _positive_fp32('scale_scale', scale_scale)
        self.P = _positive_fp32('1 / location_scale^2', self.location_scale ** -2)
        self.Hh = _positive_fp32('1 / scale_scale^2', self.scale_scale ** -2)
        self.intercepts, self.slopes, self.centered = intercepts, slopes, centered
        self.known_noise = sig is not None
        self.n_groups, self.n_obs = C, N
        self.y, self.x, self.group, self.noise_scale = yv.contiguous(), xv.contiguous(), gv.contiguous(), sig
        # the sufficient statistics, fp64, centred before they are squared
        zero = torch.zeros(C, dtype=torch.float64)
        n = zero.index_add(0, gv, om)
        xb = zero.index_add(0, gv, om * xv) / n
        yb = zero.index_add(0, gv, om * yv) / n
        dx, dy = xv - xb[gv], yv - yb[gv]
        self.stats = torch.stack([n, xb, yb, zero.index_add(0, gv, om * dx * dx), zero.index_add(0, gv, om * dx * dy),
                                  zero.index_add(0, gv, om * dy * dy)], dim=1).contiguous()   # (C, 6)
        _check_finite(self.stats, 'the group statistics (n, xbar, ybar, Sxx, Sxy, Syy) must be finite in fp32')
        self.both = intercepts == 'varying' and slopes == 'varying'
        self.group_block = 2 * C if self.both else C
        self.names = ((['mu_a', 's_a'] if intercepts == 'varying' else ['a'])
                      + {'varying': ['mu_b', 's_b'], 'shared': ['b'], 'none': []}[slopes]
                      + ([] if self.known_noise else ['s_y']))
        self.event_shape = (self.group_block + len(self.names),)
        self.code = (self.MODES[intercepts] + 4 * self.MODES[slopes] + 16 * int(self.known_noise)
                     + 32 * int(not centered))
        self._dev = {}

    @classmethod
    def synthetic(cls, n_groups, n_obs, seed, **model):
        """(potential, truth): a data set of `n_obs` observations in `n_groups` groups drawn from the model that `model`
        (the constructor's keywords other than y, group and x) describes; every group gets one observation and the rest
        are assigned at random.  The group-level means are drawn from N(0, 1) and the group-level and noise scales from
        HalfNormal(1) + 0.25, not from the wide priors, so that the data are of order one; x ~ N(0, 1); a known
        `noise_scale` is used as given.  All draws in fp64 from one CPU torch.Generator seeded with `seed`.  `truth` is
        the packed generating state (d,), fp64, in the model's own parameterisation."""
        C, N = int(n_groups), int(n_obs)
        if C < 1 or N < C:
            raise ValueError('n_groups >= 1 and n_obs >= n_groups, got %r, %r' % (n_groups, n_obs))
        g = torch.Generator().manual_seed(int(seed))
        rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)   # noqa: E731
        group = torch.cat([torch.arange(C), torch.randint(0, C, (N - C,), generator=g)])
        group = group[torch.randperm(N, generator=g)]
        x = rn(N)
        ia, sl = model.get('intercepts', 'varying'), model.get('slopes', 'none')
        parts, eff = {}, {}
        for side, mode in (('a', ia), ('b', sl)):
            if mode == 'varying':
                mu, sg, t = rn(()), rn(()).abs() + 0.25, rn(C)
                parts['mu_' + side], parts['s_' + side], eff[side] = mu, sg.log(), mu + sg * t
                parts[side] = eff[side] if model.get('centered', True) else t
            elif mode == 'shared':
                parts[side] = rn(())
                eff[side] = parts[side].expand(C)
            else:
                eff[side] = torch.zeros(C, dtype=torch.float64)
        ns = model.get('noise_scale')
        if ns is None:
            sy = rn(()).abs() + 0.25
            parts['s_y'] = sy.log()
            sig = sy.expand(N)
        else:
            sig = torch.as_tensor(ns, dtype=torch.float64).expand(N)
        y = eff['a'][group] + eff['b'][group] * x + sig * rn(N)
        pot = cls(y, group, None if sl == 'none' else x, **model)
        return pot, pot.pack(**parts)

    @classmethod
    def eight_schools(cls, **model):
        """Rubin's eight schools: one observation per group with known standard errors, varying intercepts, no slope
        (d = 10: theta_0 .. theta_7, mu, log tau).  `model` may set centered, location_scale and scale_scale."""
        y = [28.0, 8.0, -3.0, 7.0, -1.0, 1.0, 18.0, 12.0]
        sigma = [15.0, 10.0, 16.0, 11.0, 9.0, 11.0, 10.0, 18.0]
        return cls(torch.tensor(y, dtype=torch.float64), torch.arange(8), None, intercepts='varying', slopes='none',
                   noise_scale=torch.tensor(sigma, dtype=torch.float64), **model)

    def unpack(self, x):
        """dict of the parts of states x (..., d) that exist: 'a' (..., C) or (...) and 'b' likewise (the group
        coordinates of a varying side, as sampled; the value of a shared side), 'mu_a', 's_a', 'mu_b', 's_b', 's_y'."""
        x = self._event_states(x)
        gb, out = self.group_block, {}
        if self.both:
            out['a'], out['b'] = x[..., 0:gb:2], x[..., 1:gb:2]
        else:
            out['a' if self.intercepts == 'varying' else 'b'] = x[..., :gb]
        for k, name in enumerate(self.names):
            out[name] = x[..., gb + k]
        return out

    def pack(self, **parts):
        """The state x (..., d) of the parts `unpack` names (all of them, and no others); the leading shapes
        broadcast.  Inverse of `unpack`."""
        vary = [s for s, m in (('a', self.intercepts), ('b', self.slopes)) if m == 'varying']
        want = set(vary) | set(self.names)
        if set(parts) != want:
            raise ValueError('pack needs exactly the parts %s, got %s' % (sorted(want), sorted(parts)))
        first = torch.as_tensor(parts[vary[0]])
        dt = first.dtype if first.is_floating_point() else torch.get_default_dtype()
        t = {k: torch.as_tensor(v, dtype=dt, device=first.device) for k, v in parts.items()}
        C = self.n_groups
        for s in vary:
            if t[s].dim() < 1 or t[s].shape[-1] != C:
                raise ValueError('%s must end in C = %d entries, got shape %s' % (s, C, tuple(t[s].shape)))
        lead = torch.broadcast_shapes(*[t[k].shape[:-1] if k in vary else t[k].shape for k in t])
        if self.both:
            blk = torch.stack([t['a'].expand(lead + (C,)), t['b'].expand(lead + (C,))], dim=-1).reshape(lead + (2 * C,))
        else:
            blk = t[vary[0]].expand(lead + (C,))
        return torch.cat([blk] + [t[name].expand(lead)[..., None] for name in self.names], dim=-1)

    def effects(self, x):
        """(a_c, b_c), each (..., C), on the natural scale in either parameterisation (a shared side repeated over the
        groups, b = 0 for slopes='none')."""
        p = self.unpack(x)
        out = []
        for side, mode in (('a', self.intercepts), ('b', self.slopes)):
            if mode == 'varying':
                v = p[side]
                out.append(v if self.centered else p['mu_' + side][..., None] + torch.exp(p['s_' + side])[..., None] * v)
            elif mode == 'shared':
                out.append(p[side][..., None].expand(p[side].shape + (self.n_groups,)))
            else:
                ref = out[0]
                out.append(torch.zeros_like(ref))
        return out[0], out[1]

    def _stats(self, device, dtype):
        return self._cached((str(device), dtype), lambda: self.stats.to(device, dtype).contiguous())

    def __call__(self, x):
        n = x.shape[0]
        xf = x.reshape(n, -1)
        st = self._stats(xf.device, xf.dtype)
        nn, xb, yb, sxx, sxy, syy = (st[:, k] for k in range(6))
        p = self.unpack(xf)
        a, b = self.effects(xf)
        C, P, Hh = self.n_groups, self.P, self.Hh
        e = yb - a - b * xb
        q = torch.sum(nn * e * e + syy - 2.0 * b * sxy + b * b * sxx, dim=1)
        if self.known_noise:
            u = 0.5 * q
        else:
            sy = p['s_y']
            u = 0.5 * torch.exp(-2.0 * sy) * q + self.n_obs * sy + 0.5 * Hh * torch.exp(2.0 * sy) - sy
        for side, mode in (('a', self.intercepts), ('b', self.slopes)):
            if mode == 'varying':
                mu, s, v = p['mu_' + side], p['s_' + side], p[side]
                if self.centered:
                    r = v - mu[:, None]
                    u = u + C * s + 0.5 * torch.exp(-2.0 * s) * torch.sum(r * r, dim=1)
                else:
                    u = u + 0.5 * torch.sum(v * v, dim=1)
                u = u + 0.5 * P * mu * mu + 0.5 * Hh * torch.exp(2.0 * s) - s
            elif mode == 'shared':
                u = u + 0.5 * P * p[side] * p[side]
        return u

    def data_block(self):
        """The kernels' group table (NFMC_POT_VARYING_EFFECTS, include/nfmc_hip.h): (C, 8) fp32 on the CPU, rows
        (n, xbar, ybar, Sxx, Sxy, Syy, 0, 0)."""
        T = torch.zeros(self.n_groups, 8, dtype=torch.float32)
        T[:, :6] = self.stats.float()
        return T

    def descriptor(self, device):
        def make():
            par = torch.tensor([self.P, self.Hh], dtype=torch.float64)
            return self.data_block().to(device).contiguous(), par.to(device, torch.float32).contiguous()
        T, par = self._cached((str(device), 'descriptor'), make)
        return hip.NfmcPotential(hip.POT_VARYING_EFFECTS, self.n_groups, hip.ptr(T), hip.ptr(par), float(self.code),
                                 0.0 if self.known_noise else float(self.n_obs))
