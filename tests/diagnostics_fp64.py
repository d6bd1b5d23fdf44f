"""fp64 numpy restatement of the convergence diagnostics, straight from the raw kept states
x (K draws, n chains, d coordinates): `direct` evaluates the definitions as written, `sums` builds the additive
per-coordinate sums in the layout of nfmc_chain_diagnostics_f32.  Neither shares code with nfmc_amd.diagnostics."""
import math

import numpy as np


def chain_moments(x, max_lag):
    """m (n, d), a (L + 1, n, d) biased autocovariances about the chain's own mean, s2 (n, d); L = min(K - 1, max_lag)."""
    x = np.asarray(x, dtype=np.float64)
    K = x.shape[0]
    L = min(K - 1, int(max_lag))
    m = x.mean(axis=0)
    c = x - m
    a = np.stack([(c[:K - l] * c[l:]).sum(axis=0) / K for l in range(L + 1)])
    return m, a, a[0] * K / (K - 1)


def halves(x):
    """The 2 n half-chains: draws [0, h) and [K - h, K) of every chain -> (h, 2 n, d)."""
    x = np.asarray(x, dtype=np.float64)
    h = x.shape[0] // 2
    return np.concatenate([x[:h], x[x.shape[0] - h:]], axis=1)


def _div(a, b):
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(b > 0, a / np.where(b > 0, b, 1.0), np.nan)


def direct(x, max_lag, group=None):
    """dict of per-coordinate results from the definitions."""
    x = np.asarray(x, dtype=np.float64)
    K, n, d = x.shape
    if K < 4:
        raise ValueError('K < 4')
    if group is not None and (group < 1 or n % group):
        raise ValueError('group does not divide n')
    m, a, s2 = chain_moments(x, max_lag)
    L = a.shape[0] - 1

    hx = halves(x)
    h = hx.shape[0]
    ws = hx.var(axis=0, ddof=1).mean(axis=0)
    bs = hx.mean(axis=0).var(axis=0, ddof=1)
    rhat = np.sqrt(_div((h - 1) / h * ws + bs, ws))

    w = s2.mean(axis=0)
    varp = (K - 1) / K * w + (m.var(axis=0, ddof=1) if n > 1 else 0.0)
    rho = np.stack([1 - _div(w - a[l].mean(axis=0) * K / (K - 1), varp) for l in range(L + 1)])
    rho[0] = np.where(w > 0, 1.0, np.nan)
    rho = np.where(w > 0, rho, np.nan)
    ess = np.full(d, np.nan)
    truncated = np.zeros(d, dtype=bool)
    for c in range(d):
        if not w[c] > 0:
            continue
        total, prev, ran_out = 0.0, math.inf, True
        for k in range((L + 1) // 2):
            p = rho[2 * k, c] + rho[2 * k + 1, c]
            if p < 0:
                ran_out = False
                break
            prev = min(p, prev)
            total += prev
        tau = max(-1 + 2 * total, 1 / math.log10(n * K))
        ess[c] = n * K / tau
        truncated[c] = ran_out
    out = {'rhat': rhat, 'ess': ess, 'truncated': truncated, 'mean': m.mean(axis=0), 'sd': np.sqrt(varp),
           'mcse_mean': np.sqrt(_div(varp, ess)), 'autocorrelation': rho, 'max_lag': L}
    if group is not None:
        G = n // group
        if G < 2:
            out['nested_rhat'] = np.full(d, np.nan)
        else:
            mg, sg = m.reshape(G, group, d), s2.reshape(G, group, d)
            bt = mg.var(axis=1, ddof=1) if group > 1 else np.zeros((G, d))
            wn = (bt + sg.mean(axis=1)).mean(axis=0)
            bn = mg.mean(axis=1).var(axis=0, ddof=1)
            out['nested_rhat'] = np.sqrt(1 + _div(bn, wn))
    return out


def sums(x, max_lag, group=1):
    """The additive sums in the kernel's layout: dict of (d,) arrays + 'acov' (max_lag + 1, d); lags >= K are empty sums."""
    x = np.asarray(x, dtype=np.float64)
    K, n, d = x.shape
    m, a, _ = chain_moments(x, max_lag)
    acov = np.zeros((int(max_lag) + 1, d))
    acov[:a.shape[0]] = a.sum(axis=1)
    hx = halves(x)
    mh, s2h = hx.mean(axis=0), hx.var(axis=0, ddof=1)
    mg = m.reshape(n // group, group, d)
    mu = mg.mean(axis=1)
    bt = mg.var(axis=1, ddof=1) if group > 1 else np.zeros_like(mu)
    return {'sum_m': m.sum(axis=0), 'sum_m2': (m * m).sum(axis=0), 'sum_mh': mh.sum(axis=0), 'sum_mh2': (mh * mh).sum(axis=0),
            'sum_s2h': s2h.sum(axis=0), 'sum_mu': mu.sum(axis=0), 'sum_mu2': (mu * mu).sum(axis=0), 'sum_bt': bt.sum(axis=0),
            'acov': acov}


def ar1(rng, K, n, d, phi, mean=0.0, sd=1.0):
    """Stationary AR(1) chains with marginal N(mean, sd^2), fp32."""
    z = rng.standard_normal((K, n, d))
    x = np.empty_like(z)
    x[0] = z[0]
    for t in range(1, K):
        x[t] = phi * x[t - 1] + math.sqrt(1 - phi * phi) * z[t]
    return (mean + sd * x).astype(np.float32)
