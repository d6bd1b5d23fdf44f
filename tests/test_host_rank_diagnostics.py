"""CPU: the definitions of the rank-normalised diagnostics on the fp64 oracle (rank_fp64.py) -- the two tail thresholds
are the type-7 quantiles, a scale mixture that the plain split R-hat passes is flagged, heavy tails leave the bulk R-hat
alone -- and the declarations, argument rules and defaults of the new surface.  No GPU call."""
import os

import numpy as np
import pytest
import torch

import diagnostics_fp64 as plain
import rank_fp64 as ref
from nfmc_amd import diagnostics, hip
from nfmc_amd.containers import MCMCOutput

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RANK_FIELDS = ('rhat_bulk', 'rhat_tail', 'rhat_rank', 'ess_bulk', 'ess_tail', 'truncated_bulk', 'truncated_tail',
               'nested_rhat_bulk', 'n_nonfinite')


@pytest.mark.parametrize('S', [4, 5, 20, 21, 23, 100, 1601])
def test_the_thresholds_are_the_type_7_quantiles(S):
    """v <= x_(floor((S-1)/20)) is v <= quantile(v, 0.05) and v >= x_(ceil(19(S-1)/20)) is v >= quantile(v, 0.95) on fp32
    data, with ties and without."""
    rng = np.random.default_rng(S)
    for v in (rng.standard_normal(S).astype(np.float32), rng.integers(-3, 4, S).astype(np.float32),
              np.arange(S, dtype=np.float32)):
        lo, _, _, hi = ref.threshold_indices(S)
        s = np.sort(v)
        v64 = v.astype(np.float64)
        assert ((v64 <= s[lo]) == (v64 <= np.quantile(v64, 0.05))).all()
        assert ((v64 >= s[hi]) == (v64 >= np.quantile(v64, 0.95))).all()
        x = v.reshape(4, -1, 1) if S % 4 == 0 else v.reshape(S, 1, 1)   # the series themselves, through the same indices
        assert (ref.series(x, 'tail_low').reshape(-1) == (v64 <= np.quantile(v64, 0.05))).all()
        assert (ref.series(x, 'tail_high').reshape(-1) == (v64 >= np.quantile(v64, 0.95))).all()


def test_average_ranks_and_scores():
    v = np.array([2.0, -0.0, 0.0, 5.0, 2.0, 2.0], dtype=np.float32)
    assert ref.average_ranks(v).tolist() == [4.0, 1.5, 1.5, 6.0, 4.0, 4.0]
    z = ref.scores(np.array([3.5]), 6)                 # the middle rank of six: p = 1/2
    assert z[0] == 0.0
    const = np.full((4, 3, 1), 7.5, dtype=np.float32)
    assert (ref.series(const, 'bulk') == 0).all() and (ref.series(const, 'folded') == 0).all()
    assert (ref.series(const, 'tail_low') == 1).all() and (ref.series(const, 'tail_high') == 1).all()


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_a_scale_mixture_passes_the_plain_rhat_and_is_flagged(seed):
    """Four chains N(0, 1), four N(0, 3^2) in coordinate 0: same location, so the split R-hat of the values sees nothing."""
    x = np.random.default_rng(seed).standard_normal((200, 8, 2))
    x[:, 4:, 0] *= 3.0
    x = x.astype(np.float32)
    rhat = plain.direct(x, 127)['rhat']
    got = ref.direct(x, 127)
    print(seed, rhat, got['rhat_tail'], got['ess_bulk'], got['ess_tail'])
    assert rhat[0] < 1.01 and got['rhat_tail'][0] > 1.1 and got['ess_tail'][0] < got['ess_bulk'][0] / 3
    assert rhat[1] < 1.01 and got['rhat_tail'][1] < 1.01
    assert (got['rhat_rank'] == np.maximum(got['rhat_bulk'], got['rhat_tail'])).all()


def test_cauchy_draws_have_a_bulk_rhat_of_one():
    x = np.random.default_rng(5).standard_cauchy((200, 8, 2)).astype(np.float32)
    got = ref.direct(x, 127)
    print(got['rhat_bulk'])
    assert ((got['rhat_bulk'] > 0.99) & (got['rhat_bulk'] < 1.01)).all()


def test_a_nonfinite_coordinate_is_nan_and_the_rest_untouched():
    x = plain.ar1(np.random.default_rng(3), 10, 6, 3, 0.4)
    want = ref.direct(x[:, :, [0, 2]], 9, 3)
    x[4, 2, 1] = np.nan
    got = ref.direct(x, 9, 3)
    assert got['n_nonfinite'].tolist() == [0, 1, 0]
    for name in ('rhat_bulk', 'rhat_tail', 'rhat_rank', 'ess_bulk', 'ess_tail', 'nested_rhat_bulk'):
        assert np.isnan(got[name][1]) and (got[name][[0, 2]] == want[name]).all(), name


def test_the_abi_declares_the_rank_entry_points():
    names = {s[0] for s in hip.SYMBOLS}
    for fn in ('nfmc_rank_work_bytes', 'nfmc_rank_series_f32'):
        assert fn in names, fn
    assert os.path.exists(os.path.join(ROOT, 'nfmc_amd', 'csrc', 'rank_kernels.hpp'))


class TwoRanks:
    world = 2


def test_rank_normalized_refuses_a_shard_of_several_ranks():
    with pytest.raises(ValueError, match='shard'):
        diagnostics.diagnose(torch.zeros(8, 4, 2), shard=TwoRanks(), rank_normalized=True)
    with pytest.raises(ValueError, match='store_samples'):
        MCMCOutput((2,), store_samples=False).diagnostics(rank_normalized=True)
    with pytest.raises(ValueError):
        diagnostics.rank_series(torch.zeros(8), 'bulk')


def test_without_the_keyword_every_rank_field_is_none():
    x = plain.ar1(np.random.default_rng(1), 12, 4, 2, 0.3)
    s = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in plain.sums(x, 11, 2).items()}
    got = diagnostics.from_sums(s, 12, 4, 2)
    for name in RANK_FIELDS:
        assert getattr(got, name) is None, name
    assert not set(got.summary()) & {'max_rhat_rank', 'min_ess_bulk', 'min_ess_tail', 'n_nonfinite'}
    # positional construction is untouched: the new fields come last and default to None
    first = [getattr(got, f) for f in ('rhat', 'nested_rhat', 'ess', 'mcse_mean', 'mean', 'sd', 'truncated',
                                       'autocorrelation', 'n_draws', 'n_chains', 'max_lag')]
    again = diagnostics.Diagnostics(*first)
    assert again.rhat_rank is None and again.max_lag == got.max_lag
    got.rhat_rank, got.ess_bulk, got.ess_tail = got.rhat, got.ess, got.ess
    got.n_nonfinite = torch.tensor([0, 3])
    s = got.summary()
    assert s['max_rhat_rank'] == s['max_rhat'] and s['min_ess_bulk'] == s['min_ess_tail'] == s['min_ess']
    assert s['n_nonfinite'] == 1
