"""The observation model the two latent-Gaussian kinds share (lgm.py, gmrf.py; csrc/pot_shared.hpp holds its device
side): one of three likelihoods on every site of a latent field, with an observation y_j, a prior mean m_j and a weight
w_j >= 0 per site, w_j = 0 meaning "not observed"."""
import torch

from ._base import _as_fp64, _check_finite, _positive_fp32


class SiteObservations:
    """Mix-in of a Potential with a `latent(x)`: validates and holds y, mean, weight, dof and scale, evaluates the
    likelihood in torch ops and writes the kernels' table of them."""

    LIKELIHOODS = ('poisson', 'binomial', 'student_t')

    def _set_observations(self, yv, n, sites, likelihood, mean, weight, observed, dof, scale):
        """Validates the observations against `n` sites (`sites` is the letter the messages give that count; `yv` is
        fp64 with n entries already) and sets likelihood, y, mean, weight (fp64 masters, (n,)), dof and scale."""
        m = _as_fp64(mean)
        m = m.expand(n).clone() if m.numel() == 1 else m.reshape(-1)
        if m.numel() != n:
            raise ValueError('mean must be a number or have %s = %d entries, got %d' % (sites, n, m.numel()))
        w = torch.ones(n, dtype=torch.float64) if weight is None else _as_fp64(weight)
        w = w.expand(n).clone() if w.numel() == 1 else w.reshape(-1)
        if w.numel() != n:
            raise ValueError('weight must be a number or have %s = %d entries, got %d' % (sites, n, w.numel()))
        if observed is not None:
            ob = torch.as_tensor(observed).detach().to('cpu').reshape(-1)
            if ob.dtype != torch.bool or ob.numel() != n:
                raise ValueError('observed must be a bool mask of %s = %d entries, got %s of %d'
                                 % (sites, n, ob.dtype, ob.numel()))
            w = torch.where(ob, w, torch.zeros_like(w))
        if not bool(torch.isfinite(w).all()) or not bool((w >= 0).all()):
            raise ValueError('weight must be finite and >= 0')
        yv = torch.where(w > 0, yv, torch.zeros_like(yv))      # an unobserved site's y is never read
        for name, v in (('y', yv), ('mean', m), ('weight', w)):
            _check_finite(v, '%s must be finite (in fp32 too: the kernels read an fp32 copy)' % name)
        if likelihood in ('poisson', 'binomial'):
            if not bool(((yv >= 0) & (yv == yv.round())).all()):
                raise ValueError('the counts y of the %s family must be non-negative integers' % likelihood)
        if likelihood == 'binomial':
            if not bool((w == w.round()).all()):
                raise ValueError('the trials (weight) of the binomial family must be integers')
            if not bool((yv <= w).all()):
                raise ValueError('the binomial family needs 0 <= y <= trials (weight)')
        self.dof = _positive_fp32('dof', dof)
        self.scale = _positive_fp32('scale', scale)
        if likelihood == 'student_t':
            for name, v in (('(dof + 1) / 2', 0.5 * (self.dof + 1.0)), ('1 / (dof scale^2)', 1.0 / (self.dof * self.scale ** 2)),
                            ('dof scale^2', self.dof * self.scale ** 2)):
                _positive_fp32(name, v)
        self.likelihood = likelihood
        self.y = yv.contiguous()               # fp64 masters; the kernels get fp32
        self.weight = w.contiguous()
        self.mean = m.contiguous()

    def mean_response(self, x):
        """The Poisson rate w e^f, the success probability sigmoid(f), or the location f, at the coordinates x."""
        f = self.latent(x)
        if self.likelihood == 'poisson':
            return self.weight.to(f) * torch.exp(f)
        if self.likelihood == 'binomial':
            return torch.sigmoid(f)
        return f

    def _lik(self, f, y, w, second=False):
        """sum-free l_j(f_j) (..., d) in the dtype of f; with `second` its second derivative instead."""
        on = w > 0
        f = torch.where(on, f, torch.zeros_like(f))   # no 0 * inf in autograd where an unobserved e^f overflows
        if self.likelihood == 'poisson':
            e = w * torch.exp(f)
            out = e if second else e - y * f
        elif self.likelihood == 'binomial':
            if second:
                sg = torch.sigmoid(f)
                out = w * sg * (1.0 - sg)
            else:
                out = w * torch.logaddexp(f.new_zeros(()), f) - y * f
        else:
            t = y - f
            q = t * t
            ns2 = self.dof * self.scale ** 2
            if second:
                out = w * (self.dof + 1.0) * (ns2 - q) / (ns2 + q) ** 2
            else:
                out = w * (0.5 * (self.dof + 1.0)) * torch.log1p(q / ns2)
        return torch.where(on, out, torch.zeros_like(out))

    def _table(self, n):
        """The kernels' table in fp64 (the caller rounds it to fp32).  A head of 8 floats: ((nu+1)/2, 1/(nu s^2), nu s^2,
        nu+1), zeros unless Student-t, and four zeros that are the caller's; then the rows m, y, w of n4 = 4 ceil(n / 4)
        floats each, zero past n."""
        n4 = 4 * ((n + 3) // 4)
        tab = torch.zeros(8 + 3 * n4, dtype=torch.float64)
        if self.likelihood == 'student_t':
            ns2 = self.dof * self.scale ** 2
            tab[:4] = torch.tensor([0.5 * (self.dof + 1.0), 1.0 / ns2, ns2, self.dof + 1.0], dtype=torch.float64)
        for k, v in enumerate((self.mean, self.y, self.weight)):
            tab[8 + k * n4:8 + k * n4 + n] = v
        return tab
