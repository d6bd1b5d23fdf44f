"""numpy / standard-library restatement of the rank transform of the rank-normalised diagnostics (DESIGN.md 3.5,
include/nfmc_hip.h: nfmc_rank_series_f32), straight from the definitions: average ranks of the pooled fp32 values of a
coordinate by np.unique, the normal quantile by statistics.NormalDist, the order statistics by np.sort.  `direct` feeds the
four series to diagnostics_fp64.direct.  Shares no code with nfmc_amd."""
import functools
import statistics

import numpy as np

import diagnostics_fp64

KINDS = ('bulk', 'folded', 'tail_low', 'tail_high')
_INV_CDF = statistics.NormalDist().inv_cdf


def canonical(v):
    """fp32 values with -0.0 turned into +0.0 (equality is numeric)."""
    return np.asarray(v, dtype=np.float32) + np.float32(0.0)


def average_ranks(v):
    """r_i = #{v < v_i} + (#{v = v_i} + 1) / 2 of a 1-D fp32 array, fp64 (exact: multiples of 1/2)."""
    _, inv, cnt = np.unique(canonical(v), return_inverse=True, return_counts=True)
    less = np.cumsum(cnt) - cnt
    return less[inv.reshape(-1)] + (cnt[inv.reshape(-1)] + 1) / 2.0


@functools.lru_cache(maxsize=32)
def _score_table(S):
    """z of every possible average rank of S values: entry h is the rank h / 2, h = 2 .. 2 S."""
    return np.array([np.nan, np.nan] + [_INV_CDF((h / 2.0 - 0.375) / (S + 0.25)) for h in range(2, 2 * S + 1)])


def scores(r, S):
    """z = Phi^-1((r - 3/8) / (S + 1/4)) in fp64 (the ranks are multiples of 1/2: one inv_cdf each, kept per S)."""
    return _score_table(int(S))[np.rint(2 * np.asarray(r)).astype(np.int64)]


def threshold_indices(S):
    """Indices into the sorted values: low tail, the two middle ones, high tail (integer arithmetic)."""
    return (S - 1) // 20, (S - 1) // 2, -((-(S - 1)) // 2), -((-19 * (S - 1)) // 20)


def order_stats(x):
    """(d, 4) fp64: x_(lo), the two middle order statistics, x_(hi) of every coordinate (NaN rows where it is not finite)."""
    K, n, d = x.shape
    v = np.sort(canonical(x).reshape(K * n, d).astype(np.float64), axis=0)
    out = v[list(threshold_indices(K * n))].T.copy()
    out[~np.isfinite(x.reshape(K * n, d)).all(axis=0)] = np.nan
    return out


def nonfinite(x):
    return (~np.isfinite(x.reshape(-1, x.shape[-1]))).sum(axis=0)


def folded_values(x):
    """f = fl32(|fp64(v) - med|), (S, d) fp32; med exact in fp64."""
    K, n, d = x.shape
    os_ = order_stats(x)
    med = (os_[:, 1] + os_[:, 2]) / 2
    with np.errstate(over='ignore', invalid='ignore'):
        return np.abs(x.reshape(K * n, d).astype(np.float64) - med).astype(np.float32)


def series64(x, kind):
    """The series in fp64 before its one rounding to fp32 (the indicators are exact either way), (K, n, d)."""
    x = np.asarray(x, dtype=np.float32)
    K, n, d = x.shape
    S = K * n
    v = x.reshape(S, d)
    bad = nonfinite(x) > 0
    out = np.full((S, d), np.nan)
    os_ = order_stats(x)
    src = folded_values(x) if kind == 'folded' else v
    for c in np.flatnonzero(~bad):
        if kind in ('bulk', 'folded'):
            out[:, c] = scores(average_ranks(src[:, c]), S)
        elif kind == 'tail_low':
            out[:, c] = v[:, c].astype(np.float64) <= os_[c, 0]
        elif kind == 'tail_high':
            out[:, c] = v[:, c].astype(np.float64) >= os_[c, 3]
        else:
            raise ValueError(kind)
    return out.reshape(K, n, d)


def series(x, kind):
    return series64(x, kind).astype(np.float32)


def from_series(s, max_lag, group=None):
    """The reported fields from the four series (dict kind -> (K, n, d) array), each through diagnostics_fp64.direct."""
    r = {k: diagnostics_fp64.direct(np.asarray(s[k], dtype=np.float64), max_lag, group) for k in KINDS}
    out = {'rhat_bulk': r['bulk']['rhat'], 'rhat_tail': r['folded']['rhat'],
           'rhat_rank': np.maximum(r['bulk']['rhat'], r['folded']['rhat']),
           'ess_bulk': r['bulk']['ess'], 'ess_tail': np.minimum(r['tail_low']['ess'], r['tail_high']['ess']),
           'ess_tail_low': r['tail_low']['ess'], 'ess_tail_high': r['tail_high']['ess'],
           'truncated_bulk': r['bulk']['truncated'], 'truncated_tail': r['tail_low']['truncated'] | r['tail_high']['truncated']}
    if group is not None:
        out['nested_rhat_bulk'] = r['bulk']['nested_rhat']
    return out


def direct(x, max_lag, group=None):
    x = np.asarray(x, dtype=np.float32)
    out = from_series({k: series(x, k) for k in KINDS}, max_lag, group)
    out['n_nonfinite'] = nonfinite(x)
    return out
