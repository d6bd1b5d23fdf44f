"""Convergence diagnostics of a run's kept states: split R-hat, nested R-hat (Margossian et al.) and the effective
sample size of Stan / Vehtari et al. 2021, per coordinate; on request also their rank-normalised forms (bulk and
folded R-hat, bulk and tail ESS), which are the same definitions applied to four rank series of the states that a
second HIP call produces on the device (nfmc_rank_series_f32, csrc/rank_kernels.hpp).

The heavy part -- per-chain means, half-chain moments and lagged autocovariances of the n x d series -- is one HIP call
over the device-resident slab (nfmc_chain_diagnostics_f32, csrc/diagnostics.hpp).  It returns per-coordinate fp64 sums
that are additive over chains; everything reported here is a closed-form function of those sums and of
(n_draws, n_chains, superchain size), evaluated on the host in fp64 (`from_sums`), so chains sharded over GPUs combine
by one all-reduce of the sums.  DESIGN.md 3.5 has the definitions.
"""
import ctypes as C
import math
from dataclasses import dataclass
from typing import Dict, Optional

import torch

from . import hip

DEFAULT_MAX_LAG = hip.DIAG_MAX_LAG


@dataclass
class Diagnostics:
    """Per-coordinate diagnostics; every tensor is fp64 on the host with the run's event shape."""
    rhat: torch.Tensor                   # split R-hat over the 2 n half-chains
    nested_rhat: Optional[torch.Tensor]  # None unless superchains were asked for; NaN with fewer than two superchains
    ess: torch.Tensor                    # effective sample size, in units of kept draws
    mcse_mean: torch.Tensor              # Monte Carlo standard error of `mean`
    mean: torch.Tensor                   # mean over all kept draws of all chains
    sd: torch.Tensor                     # sqrt of the pooled variance estimate varp
    truncated: torch.Tensor              # bool: the lags ran out before a negative Geyer pair, `ess` is an upper estimate
    autocorrelation: torch.Tensor        # (max_lag + 1, *event): rho_l
    n_draws: int
    n_chains: int
    max_lag: int
    # rank-normalised (Vehtari et al. 2021), None unless asked for: the definitions above applied to the rank series
    rhat_bulk: Optional[torch.Tensor] = None         # split R-hat of the normal scores of the pooled ranks
    rhat_tail: Optional[torch.Tensor] = None         # split R-hat of the scores of the ranks of |x - median|
    rhat_rank: Optional[torch.Tensor] = None         # max of the two: the paper's R-hat
    ess_bulk: Optional[torch.Tensor] = None          # `ess` of the scores (unsplit chains, as `ess`)
    ess_tail: Optional[torch.Tensor] = None          # min of `ess` of the indicators x <= q05 and x >= q95
    truncated_bulk: Optional[torch.Tensor] = None
    truncated_tail: Optional[torch.Tensor] = None    # of either indicator
    nested_rhat_bulk: Optional[torch.Tensor] = None  # with superchains: nested R-hat of the scores
    n_nonfinite: Optional[torch.Tensor] = None       # int64: NaN / Inf values per coordinate (its rank fields are NaN)

    def summary(self) -> Dict[str, float]:
        def worst(t, fn):
            ok = t[~torch.isnan(t)]
            return float(fn(ok)) if ok.numel() else math.nan
        out = {'max_rhat': worst(self.rhat, torch.max), 'min_ess': worst(self.ess, torch.min),
               'n_truncated': int(self.truncated.sum()), 'n_nan': int(torch.isnan(self.rhat).sum()),
               'n_draws': self.n_draws, 'n_chains': self.n_chains, 'max_lag': self.max_lag}
        if self.nested_rhat is not None:
            out['max_nested_rhat'] = worst(self.nested_rhat, torch.max)
        if self.rhat_rank is not None:
            out['max_rhat_rank'] = worst(self.rhat_rank, torch.max)
        if self.ess_bulk is not None:
            out['min_ess_bulk'] = worst(self.ess_bulk, torch.min)
        if self.ess_tail is not None:
            out['min_ess_tail'] = worst(self.ess_tail, torch.min)
        if self.n_nonfinite is not None:
            out['n_nonfinite'] = int((self.n_nonfinite > 0).sum())
        return out


def _check_counts(n_draws, n_chains, group):
    if n_draws < 4:
        raise ValueError('diagnostics need at least 4 kept draws per chain, got %d' % n_draws)
    if n_chains < 1:
        raise ValueError('diagnostics need at least one chain')
    if group < 1 or n_chains % group != 0:
        raise ValueError('superchains of %d chains do not divide %d chains' % (group, n_chains))


def chain_sums(x: torch.Tensor, max_lag: int, group: int = 1) -> Dict[str, torch.Tensor]:
    """The kernel's sums for kept states x (n_draws, n_chains, *event), a contiguous fp32 CUDA tensor: fp64 CPU tensors
    `sum_m`, `sum_m2` (chain means), `sum_mh`, `sum_mh2`, `sum_s2h` (half-chains), `sum_mu`, `sum_mu2`, `sum_bt`
    (superchains of `group` chains), each (d,), and `acov` (max_lag + 1, d) = sum_j a_{j,l}.  One kernel call, one
    device-to-host copy."""
    if x.dim() < 2:
        raise ValueError('expected (n_draws, n_chains, *event), got %s' % (tuple(x.shape),))
    K, n = int(x.shape[0]), int(x.shape[1])
    d = int(math.prod(x.shape[2:]))
    _check_counts(K, n, int(group))
    lib = hip.lib()
    count = int(lib.nfmc_diag_sums_doubles(d, int(max_lag)))
    nbytes = int(lib.nfmc_diag_work_bytes(n, d, int(max_lag)))
    if count <= 0 or nbytes <= 0:
        raise hip.NfmcArgumentError('diagnostics: event size %d (<= 1024) or max_lag %d (0 .. %d) outside the kernel\'s range'
                                    % (d, max_lag, hip.DIAG_MAX_LAG), hip.ESHAPE)
    sums = torch.empty(count, dtype=torch.float64, device=x.device)
    work = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
    args = hip.NfmcDiagArgs(hip.ptr(x), K, n, d, int(max_lag), int(group), 0, hip.ptr(sums, torch.float64),
                            hip.ptr(work, torch.float64), nbytes)
    with torch.cuda.device(x.device):
        hip.check(lib.nfmc_chain_diagnostics_f32(C.byref(args), hip.stream()), 'nfmc_chain_diagnostics_f32')
    return unpack_sums(sums.cpu(), d)


class _RankTransform:
    """The buffers of nfmc_rank_series_f32 for one slab x (n_draws, n_chains, d): `run(series)` fills the one output slab
    `out`, `nonfinite` (d,) int32 and `order_stats` (d, 4) fp64 and returns `out`."""

    def __init__(self, x: torch.Tensor):
        K, n, d = (int(v) for v in x.shape)
        _check_counts(K, n, 1)
        self.lib = hip.lib()
        nbytes = int(self.lib.nfmc_rank_work_bytes(K, n, d))
        if nbytes <= 0:
            raise hip.NfmcArgumentError('rank transform: event size %d (<= 1024) or %d x %d pooled draws (< 2^31) outside '
                                        'the kernel\'s range' % (d, K, n), hip.ESHAPE)
        self.x = x
        self.out = torch.empty_like(x)
        self.nonfinite = torch.empty(d, dtype=torch.int32, device=x.device)
        self.order_stats = torch.empty(d, 4, dtype=torch.float64, device=x.device)
        self.work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=x.device)
        self.args = hip.NfmcRankArgs(hip.ptr(x), K, n, d, 0, hip.ptr(self.out), hip.ptr(self.order_stats, torch.float64),
                                     hip.ptr(self.nonfinite, torch.int32), hip.ptr(self.work, torch.float64), nbytes)

    def run(self, series) -> torch.Tensor:
        if series not in hip.RANK_SERIES:
            raise ValueError('series must be one of %s, got %r' % (sorted(hip.RANK_SERIES), series))
        self.args.series = hip.RANK_SERIES[series]
        with torch.cuda.device(self.x.device):
            hip.check(self.lib.nfmc_rank_series_f32(C.byref(self.args), hip.stream()), 'nfmc_rank_series_f32')
        return self.out


def _device_slab(x: torch.Tensor) -> torch.Tensor:
    if not x.is_cuda:
        x = x.to(hip.require_gpu())
    return x.detach().to(torch.float32).contiguous()


def rank_series(x: torch.Tensor, series: str) -> torch.Tensor:
    """One series of the rank-normalised diagnostics of kept states x (n_draws, n_chains, *event), as a device slab of
    x's shape (nfmc_rank_series_f32, include/nfmc_hip.h).  Per coordinate the n_draws * n_chains values are pooled and
    ranked with average ranks for ties: 'bulk' = the normal scores Phi^-1((r - 3/8) / (S + 1/4)) of the ranks, 'folded' =
    the scores of the ranks of |x - median|, 'tail_low' / 'tail_high' = the 0 / 1 indicators of x <= its 5 % and x >= its
    95 % quantile.  A coordinate holding a NaN or Inf is NaN throughout."""
    if x.dim() < 2:
        raise ValueError('expected (n_draws, n_chains, *event), got %s' % (tuple(x.shape),))
    x = _device_slab(x)
    K, n = int(x.shape[0]), int(x.shape[1])
    out = _RankTransform(x.reshape(K, n, int(math.prod(x.shape[2:])))).run(series)
    return out.reshape(x.shape)


def unpack_sums(flat: torch.Tensor, d: int) -> Dict[str, torch.Tensor]:
    """Name the rows of the kernel's `sums` (include/nfmc_hip.h: NFMC_DIAG_*)."""
    rows = flat.reshape(-1, d)
    out = {name: rows[i] for i, name in enumerate(hip.DIAG_ROWS)}
    out['acov'] = rows[hip.DIAG_ACOV:]
    return out


def pack_sums(sums: Dict[str, torch.Tensor]) -> torch.Tensor:
    return torch.cat([sums[name].reshape(1, -1) for name in hip.DIAG_ROWS] + [sums['acov']]).reshape(-1)


def _var_from_sums(s1, s2, count):
    """Unbiased variance of `count` values from their sum and sum of squares (0 for a single value)."""
    if count < 2:
        return torch.zeros_like(s1)
    return ((s2 - s1 * s1 / count) / (count - 1)).clamp_min(0.0)


def from_sums(sums: Dict[str, torch.Tensor], n_draws: int, n_chains: int, group: Optional[int] = None,
              event_shape=None) -> Diagnostics:
    """Host fp64: the diagnostics from the additive sums (of all chains, after any all-reduce).  `group` = chains per
    superchain, None for no nested R-hat.  A coordinate without within-chain variance gets NaN, never an error."""
    K, n = int(n_draws), int(n_chains)
    _check_counts(K, n, 1 if group is None else int(group))
    s = {k: v.to(torch.float64) for k, v in sums.items()}
    L = min(int(s['acov'].shape[0]) - 1, K - 1)
    unb = K / (K - 1.0)
    nan = torch.full_like(s['sum_m'], math.nan)

    # split R-hat over the 2 n half-chains of h = K // 2 draws
    h = K // 2
    ws = s['sum_s2h'] / (2 * n)
    bs = _var_from_sums(s['sum_mh'], s['sum_mh2'], 2 * n)
    rhat = torch.where(ws > 0, torch.sqrt(((h - 1.0) / h * ws + bs) / ws), nan)

    # ESS: Geyer's initial monotone sequence on the multi-chain autocorrelation
    acov = s['acov'][:L + 1] / n                       # mean_j a_{j,l}
    w = acov[0] * unb
    varp = (K - 1.0) / K * w + _var_from_sums(s['sum_m'], s['sum_m2'], n)
    rho = torch.where(w > 0, 1.0 - (w - acov * unb) / varp, nan.expand_as(acov)).clone()
    rho[0] = torch.where(w > 0, torch.ones_like(w), nan)
    alive = torch.ones_like(w, dtype=torch.bool)
    prev = torch.full_like(w, math.inf)
    total = torch.zeros_like(w)
    for k in range((L + 1) // 2):
        pair = rho[2 * k] + rho[2 * k + 1]
        alive = alive & ~(pair < 0)
        pair = torch.minimum(pair, prev)
        total = total + torch.where(alive, pair, torch.zeros_like(pair))
        prev = torch.where(alive, pair, prev)
    tau = torch.clamp_min(-1.0 + 2.0 * total, 1.0 / math.log10(n * K))
    ess = torch.where(w > 0, n * K / tau, nan)
    mcse = torch.sqrt(varp / ess)

    nested = None
    if group is not None:
        M = int(group)
        G = n // M
        if G < 2:
            nested = nan.clone()
        else:
            wn = (s['sum_bt'] + acov[0] * n * unb / M) / G      # mean_k (Bt_k + Wt_k)
            bn = _var_from_sums(s['sum_mu'], s['sum_mu2'], G)
            nested = torch.where(wn > 0, torch.sqrt(1.0 + bn / wn), nan)

    shape = tuple(event_shape) if event_shape is not None else tuple(s['sum_m'].shape)
    def ev(t):
        return t.reshape(shape)
    return Diagnostics(rhat=ev(rhat), nested_rhat=None if nested is None else ev(nested), ess=ev(ess), mcse_mean=ev(mcse),
                       mean=ev(s['sum_m'] / n), sd=ev(torch.sqrt(varp)), truncated=ev(alive & (w > 0)),
                       autocorrelation=rho.reshape((L + 1,) + shape), n_draws=K, n_chains=n, max_lag=L)


def _rank_fields(x: torch.Tensor, max_lag: int, group: Optional[int], event_shape) -> Dict[str, torch.Tensor]:
    """The rank-normalised fields of `Diagnostics` for the slab x (n_draws, n_chains, d): the four series one after
    another through one output slab, each through `chain_sums` / `from_sums`."""
    K, n = int(x.shape[0]), int(x.shape[1])
    rt = _RankTransform(x)
    M = 1 if group is None else int(group)
    res = {s: from_sums(chain_sums(rt.run(s), max_lag, M), K, n, group, event_shape)
           for s in ('bulk', 'folded', 'tail_low', 'tail_high')}
    count = rt.nonfinite.cpu().to(torch.int64).reshape(res['bulk'].rhat.shape)
    bad = count > 0

    def clean(t):
        return torch.where(bad, torch.full_like(t, math.nan), t)
    bulk, folded, low, high = res['bulk'], res['folded'], res['tail_low'], res['tail_high']
    return dict(rhat_bulk=clean(bulk.rhat), rhat_tail=clean(folded.rhat),
                rhat_rank=clean(torch.maximum(bulk.rhat, folded.rhat)),   # NaN in either is NaN in the max
                ess_bulk=clean(bulk.ess), ess_tail=clean(torch.minimum(low.ess, high.ess)),
                truncated_bulk=bulk.truncated & ~bad, truncated_tail=(low.truncated | high.truncated) & ~bad,
                nested_rhat_bulk=None if group is None else clean(bulk.nested_rhat), n_nonfinite=count)


def diagnose(x: torch.Tensor, max_lag: Optional[int] = None, superchains: Optional[int] = None, shard=None,
             rank_normalized: bool = False) -> Diagnostics:
    """Diagnostics of kept states x (n_draws, n_chains, *event), fp32; host-resident states are moved to the device first.
    `max_lag` defaults to min(n_draws - 1, 127) and is clipped to n_draws - 1.  `superchains` = M consecutive chains
    per superchain turns the nested R-hat on; M must divide the local chain count (no superchain straddles a shard).
    With a `dist.Shard` of more than one rank the sums are all-reduced and the result describes all chains, on every
    rank.

    `rank_normalized=True` adds the rank-normalised diagnostics of Vehtari et al. 2021 (`rhat_bulk`, `rhat_tail`,
    `rhat_rank`, `ess_bulk`, `ess_tail`, ...): the same definitions applied to the four series of `rank_series`, whose
    ranks pool all chains, so it raises ValueError with a shard of more than one rank.  `ess_bulk` / `ess_tail` use
    unsplit chains, as `ess` does; the `posterior` package splits the chains for its ESS as well, so its figures differ."""
    if x.dim() < 2:
        raise ValueError('expected (n_draws, n_chains, *event), got %s' % (tuple(x.shape),))
    K, n = int(x.shape[0]), int(x.shape[1])
    event_shape = tuple(int(v) for v in x.shape[2:])
    M = 1 if superchains is None else int(superchains)
    _check_counts(K, n, M)
    L = min(K - 1, DEFAULT_MAX_LAG if max_lag is None else int(max_lag))
    if L < 0:
        raise ValueError('max_lag must not be negative')
    if rank_normalized and shard is not None and shard.world > 1:
        raise ValueError('rank_normalized diagnostics rank the values of all chains together; they are not available '
                         'across a shard of %d ranks' % shard.world)
    x = _device_slab(x)
    d = int(math.prod(event_shape))
    group = None if superchains is None else M
    sums = chain_sums(x.reshape(K, n, d), L, M)
    if shard is not None and shard.world > 1:
        pack = torch.cat([pack_sums(sums), torch.tensor([float(n)], dtype=torch.float64)])
        pack = pack.to(x.device)   # Shard moves it to the host itself under a gloo group
        shard.all_reduce_sum_(pack)
        pack = pack.cpu()
        n = int(round(float(pack[-1])))
        sums = unpack_sums(pack[:-1], d)
    out = from_sums(sums, K, n, group, event_shape)
    if rank_normalized:   # a single rank here: the local chains are all of them
        for name, value in _rank_fields(x.reshape(K, n, d), L, group, event_shape).items():
            setattr(out, name, value)
    return out


class RunningDiagnostics:
    """The accumulator of a run that keeps no states (include/nfmc_hip.h: nfmc_diag_stream_*): device
    state of about (2 max_lag + 11) n d floats that is fed each kept draw once, in blocks from a staging ring (`update`),
    and yields the sums of `chain_sums` for the draws seen so far at any time (`sums`, which only reads the state).
    `n_draws_planned` fixes the half-chains of the split R-hat before the run."""

    def __init__(self, n, d, device, max_lag, n_draws_planned):
        self.n, self.d, self.max_lag, self.planned = int(n), int(d), int(max_lag), int(n_draws_planned)
        self.device = device
        self.lib = hip.lib()
        nbytes = int(self.lib.nfmc_diag_stream_state_bytes(self.n, self.d, self.max_lag))
        if nbytes <= 0:
            raise hip.NfmcArgumentError('running diagnostics: event size %d (<= 1024) or max_lag %d (0 .. %d) outside the '
                                        'kernel\'s range' % (self.d, self.max_lag, hip.DIAG_MAX_LAG), hip.ESHAPE)
        self.state = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
        self.desc = hip.NfmcDiagStream(hip.ptr(self.state, torch.float64), nbytes, self.n, self.d, self.max_lag,
                                       self.planned, 0)
        with torch.cuda.device(device):
            hip.check(self.lib.nfmc_diag_stream_reset_f32(C.byref(self.desc), hip.stream()), 'nfmc_diag_stream_reset_f32')

    @property
    def n_seen(self) -> int:
        return int(self.desc.n_seen)

    def update(self, ring: torch.Tensor, row: int, n_rows: int, first_draw: int):
        """Fold draws first_draw .. first_draw + n_rows - 1, which sit in rows (row + r) mod ring_rows of `ring`
        (ring_rows, n, d), into the state, on the current stream."""
        args = hip.NfmcDiagStreamArgs(C.pointer(self.desc), hip.ptr(ring), int(ring.shape[0]), int(row), int(n_rows), 0,
                                      int(first_draw))
        with torch.cuda.device(self.device):
            hip.check(self.lib.nfmc_diag_stream_update_f32(C.byref(args), hip.stream()), 'nfmc_diag_stream_update_f32')

    def sums(self, group: int = 1) -> Dict[str, torch.Tensor]:
        """`chain_sums` of the draws seen so far; the half-chain rows are NaN unless all planned draws were seen."""
        _check_counts(self.n_seen, self.n, int(group))
        count = int(self.lib.nfmc_diag_sums_doubles(self.d, self.max_lag))
        nbytes = int(self.lib.nfmc_diag_stream_work_bytes(self.n, self.d, self.max_lag))
        sums = torch.empty(count, dtype=torch.float64, device=self.device)
        work = torch.empty(nbytes // 8, dtype=torch.float64, device=self.device)
        args = hip.NfmcDiagStreamSumsArgs(C.pointer(self.desc), int(group), 0, hip.ptr(sums, torch.float64),
                                          hip.ptr(work, torch.float64), nbytes)
        with torch.cuda.device(self.device):
            hip.check(self.lib.nfmc_diag_stream_sums_f32(C.byref(args), hip.stream()), 'nfmc_diag_stream_sums_f32')
        return unpack_sums(sums.cpu(), self.d)


def diagnose_running(acc, max_lag: Optional[int] = None, superchains: Optional[int] = None, shard=None,
                     rank_normalized: bool = False, event_shape=None) -> Diagnostics:
    """`diagnose` for a run that kept no states, from its accumulator (`RunningDiagnostics`): the same sums, the same
    all-reduce over a shard, the same `from_sums`.  `n_draws` is the number of draws the accumulator saw; when a time limit
    ended the run before the planned number, `rhat` is NaN (the half-chains were fixed before the run) and everything else
    describes the draws seen."""
    if rank_normalized:
        raise ValueError('rank_normalized diagnostics rank the kept states themselves: run with store_samples=True')
    L = int(acc.max_lag) if max_lag is None else int(max_lag)
    if L < 0:
        raise ValueError('max_lag must not be negative')
    if L > int(acc.max_lag):
        raise ValueError('max_lag %d exceeds the %d lags the run accumulated (running_diagnostics)' % (L, acc.max_lag))
    K, n = int(acc.n_seen), int(acc.n)
    M = 1 if superchains is None else int(superchains)
    _check_counts(K, n, M)
    sums = acc.sums(M)
    d = int(sums['sum_m'].numel())
    sums['acov'] = sums['acov'][:L + 1]
    if shard is not None and shard.world > 1:
        pack = torch.cat([pack_sums(sums), torch.tensor([float(n)], dtype=torch.float64)])
        pack = pack.to(acc.device)   # Shard moves it to the host itself under a gloo group
        shard.all_reduce_sum_(pack)
        pack = pack.cpu()
        n = int(round(float(pack[-1])))
        sums = unpack_sums(pack[:-1], d)
    return from_sums(sums, K, n, None if superchains is None else M, event_shape)
