"""CPU: the host half of the convergence diagnostics (nfmc_amd/diagnostics.py: from_sums) against the fp64 restatement
of the definitions (diagnostics_fp64.py), the NaN / ValueError rules, and the behaviour of the definitions on
synthetic chains.  No GPU call."""
import math

import numpy as np
import pytest
import torch

import diagnostics_fp64 as ref
from nfmc_amd import diagnostics
from nfmc_amd.containers import MCMCOutput

FIELDS = ('rhat', 'ess', 'mcse_mean', 'mean', 'sd', 'autocorrelation')


def from_oracle_sums(x, max_lag, group):
    s = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in ref.sums(x, max_lag, 1 if group is None else group).items()}
    return diagnostics.from_sums(s, x.shape[0], x.shape[1], group)


def assert_matches(got, want, rel=1e-12):
    for name in FIELDS + (('nested_rhat',) if 'nested_rhat' in want else ()):
        g, w = getattr(got, name).numpy(), want[name]
        assert g.shape == w.shape, name
        assert (np.isnan(g) == np.isnan(w)).all(), name
        ok = ~np.isnan(w)
        # autocorrelations cross zero: their error is measured against rho_0 = 1
        scale = np.maximum(np.abs(w[ok]), 1.0) if name == 'autocorrelation' else np.abs(w[ok])
        assert (np.abs(g[ok] - w[ok]) <= rel * scale).all(), (name, np.abs(g[ok] - w[ok]).max())
    assert (got.truncated.numpy() == want['truncated']).all()
    assert got.max_lag == want['max_lag']


@pytest.mark.parametrize('K', [4, 5, 50])
@pytest.mark.parametrize('n', [1, 2, 64])
def test_from_sums_equals_the_definitions(K, n):
    rng = np.random.default_rng(100 * K + n)
    x = ref.ar1(rng, K, n, 3, 0.6)
    for M in sorted({1, 8, n}):
        if n % M:
            continue
        got = from_oracle_sums(x, 127, M)
        assert_matches(got, ref.direct(x, 127, M))
        assert (got.n_draws, got.n_chains) == (K, n)
    assert from_oracle_sums(x, 127, None).nested_rhat is None


def test_a_constant_coordinate_is_nan_and_the_rest_finite():
    x = ref.ar1(np.random.default_rng(1), 20, 8, 3, 0.3)
    x[:, :, 1] = 2.5
    got = from_oracle_sums(x, 19, 4)
    assert_matches(got, ref.direct(x, 19, 4))
    for name in ('rhat', 'nested_rhat', 'ess', 'mcse_mean'):
        t = getattr(got, name)
        assert torch.isnan(t[1]) and torch.isfinite(t[[0, 2]]).all(), name
    assert float(got.mean[1]) == 2.5 and not bool(got.truncated[1])
    s = got.summary()
    assert s['n_nan'] == 1 and math.isfinite(s['max_rhat']) and math.isfinite(s['min_ess'])
    assert set(s) >= {'max_rhat', 'min_ess', 'n_truncated', 'max_nested_rhat'}


def test_one_superchain_gives_nan():
    x = ref.ar1(np.random.default_rng(2), 10, 8, 2, 0.0)
    got = from_oracle_sums(x, 9, 8)
    assert torch.isnan(got.nested_rhat).all() and torch.isfinite(got.rhat).all()


def test_argument_errors():
    x = ref.ar1(np.random.default_rng(3), 3, 4, 2, 0.0)
    with pytest.raises(ValueError):
        ref.direct(x, 2)
    s = {k: torch.from_numpy(v) for k, v in ref.sums(ref.ar1(np.random.default_rng(3), 4, 4, 2, 0.0), 3).items()}
    with pytest.raises(ValueError):
        diagnostics.from_sums(s, 3, 4)
    with pytest.raises(ValueError):
        diagnostics.from_sums(s, 4, 4, 3)
    with pytest.raises(ValueError):
        diagnostics.diagnose(torch.zeros(3, 4, 2))
    with pytest.raises(ValueError):
        diagnostics.diagnose(torch.zeros(8, 4, 2), superchains=3)
    with pytest.raises(ValueError, match='store_samples'):
        MCMCOutput((2,), store_samples=False).diagnostics()


@pytest.mark.parametrize('phi', [0.0, 0.5, 0.9])
def test_ar1_chains_have_the_textbook_ess_and_agree(phi):
    K, n = 1000, 64
    x = ref.ar1(np.random.default_rng(int(10 * phi) + 7), K, n, 2, phi)
    got = from_oracle_sums(x, 127, None)
    ratio = got.ess.numpy() / (n * K) * (1 + phi) / (1 - phi)
    assert ((ratio >= 0.75) & (ratio <= 1.25)).all(), ratio
    assert (got.rhat.numpy() < 1.05).all(), got.rhat


def two_mode_chains(assign):
    """K = 50 draws of 64 chains; chain j sits at N(assign[j], 1)."""
    rng = np.random.default_rng(11)
    return (rng.standard_normal((50, 64, 2)) + np.asarray(assign, dtype=np.float64)[None, :, None]).astype(np.float32)


def test_chains_locked_in_two_modes_are_flagged():
    x = two_mode_chains([5.0 if j % 2 else -5.0 for j in range(64)])
    got = from_oracle_sums(x, 49, 8)
    assert (got.rhat.numpy() > 4).all(), got.rhat
    # every superchain of 8 holds both modes: the superchains agree although the chains do not
    assert (got.nested_rhat.numpy() < 1.01).all(), got.nested_rhat


def test_superchains_locked_in_two_modes_are_flagged():
    x = two_mode_chains([5.0] * 32 + [-5.0] * 32)
    got = from_oracle_sums(x, 49, 8)
    assert (got.nested_rhat.numpy() > 4).all(), got.nested_rhat
