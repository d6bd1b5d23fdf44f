"""CPU: tests/target_harness.py's own comparisons.  Ten GPU test files trust compare_states, compare_decisions and Spy: a
bug there silences all of them, so each is shown here to pass on the oracle's own output and to fail on every kind of
error it exists to catch.  The trace is a real one: oracle.samplers.mcmc_sample, MALA on a standard normal (d = 4, 64
chains, 3 transitions) with PhiloxNoise."""
import copy
import functools

import pytest
import torch

import target_harness as H

D, N, T = 4, 64, 3
MARGIN, ATOL, RTOL = 2e-3, 1e-3, 1e-4


def _u(x):
    return 0.5 * (x ** 2).sum(-1)


@functools.lru_cache(maxsize=None)
def _case():
    """(x0 fp32, oracle Trace), computed once; the tests copy what they change"""
    from oracle import samplers as osamp
    x0 = torch.randn(N, D, generator=torch.Generator().manual_seed(1))
    tr = osamp.mcmc_sample(x0.double(), _u, 'langevin', T, 0.8, adjustment=True, noise=osamp.PhiloxNoise(7, dtype=torch.float64))
    assert 0 < tr.n_accepted < N * T                       # both decisions occur
    return x0, tr


class _Rec:
    """stands for the kernel's Record: the masks and log ratios given"""

    def __init__(self, masks, log_ratios):
        self.m, self.lr = masks, log_ratios

    def stacked(self):
        return self.m, self.lr


def _oracle_rec(tr):
    return _Rec(torch.stack([m.reshape(-1).bool() for m in tr.masks]),
                torch.stack([v.reshape(-1).float() for v in tr.log_ratios]))


def _states(got, tr, margin=MARGIN):
    return H.compare_states(got, tr, 'host', margin=margin, atol=ATOL, rtol=RTOL)


def _tol(d, want_lr, mag):
    return 2e-4 * max(1.0, d / 64) + 1e-4 * abs(want_lr) + 8 * 2.0 ** -24 * mag


# ------------------------------------------------------------------------------------------------ states
def test_states_pass_on_the_oracles_own():
    _x0, tr = _case()
    keep = _states(tr.stacked().float(), tr)
    assert keep.dtype == torch.bool and keep.shape == (N,) and bool(keep.any())


def test_states_fail_on_one_moved_coordinate_of_a_kept_chain():
    _x0, tr = _case()
    got = tr.stacked().float()
    chain = int(torch.nonzero(_states(got, tr))[0])
    got[1, chain, 2] += 2 * (ATOL + RTOL * float(got[1, chain, 2].abs()))
    with pytest.raises(AssertionError):
        _states(got, tr)


def test_states_fail_on_a_nan():
    _x0, tr = _case()
    got = tr.stacked().float()
    got[0, 0, 0] = float('nan')
    with pytest.raises(AssertionError):
        _states(got, tr)


def test_states_fail_when_the_excluded_share_reaches_the_cap():
    _x0, tr = _case()
    with pytest.raises(AssertionError):
        _states(tr.stacked().float(), tr, margin=1e3)          # every chain a near-tie


# --------------------------------------------------------------------------------------------- decisions
def test_decisions_pass_on_the_oracles_own():
    x0, tr = _case()
    H.compare_decisions(_oracle_rec(tr), tr, 'mala', x0, _u, 'host')
    H.compare_decisions(_oracle_rec(tr), tr, 'mala', x0, _u, 'host', skip_below_minus_50=True)


def test_decisions_fail_on_flipped_first_masks():
    x0, tr = _case()
    rec = _oracle_rec(tr)
    rec.m = rec.m.clone()
    rec.m[0, :N // 8] ^= True                                  # 12.5 % of the chains disagree from the first transition on
    with pytest.raises(AssertionError):
        H.compare_decisions(rec, tr, 'mala', x0, _u, 'host')


def test_decisions_fail_on_one_log_ratio_off_by_twice_its_tolerance():
    x0, tr = _case()
    rec = _oracle_rec(tr)
    want = float(tr.log_ratios[0].reshape(-1)[5])
    rec.lr = rec.lr.clone()
    rec.lr[0, 5] = want + 2 * _tol(D, want, float(_u(x0[5].double())))
    with pytest.raises(AssertionError):
        H.compare_decisions(rec, tr, 'mala', x0, _u, 'host')


def test_decisions_compare_rows_below_minus_50_unless_told_not_to():
    x0, tr = _case()
    tr = copy.deepcopy(tr)
    tr.log_ratios[0].reshape(-1)[5] = -60.0                    # fp64 says: rejected whatever the uniform
    tr.masks[0].reshape(-1)[5] = False
    rec = _oracle_rec(tr)
    rec.lr[0, 5] = -61.0                                       # the kernel's is off by far more than the tolerance
    with pytest.raises(AssertionError):
        H.compare_decisions(rec, tr, 'mala', x0, _u, 'host')
    H.compare_decisions(rec, tr, 'mala', x0, _u, 'host', skip_below_minus_50=True)


def test_decisions_use_the_magnitude_given():
    x0, tr = _case()
    rec = _oracle_rec(tr)
    want = float(tr.log_ratios[0].reshape(-1)[5])
    rec.lr = rec.lr.clone()
    rec.lr[0, 5] = want + 2 * _tol(D, want, float(_u(x0[5].double())))
    H.compare_decisions(rec, tr, 'mala', x0, _u, 'host', mag=lambda prev: _u(prev).abs() + 1e5)


def test_unadjusted_decisions_fail_on_a_rejection():
    x0, tr = _case()
    rec = _oracle_rec(tr)
    rec.m = torch.ones_like(rec.m)
    H.compare_decisions(rec, tr, 'ula', x0, _u, 'host')
    rec.m[1, 3] = False
    with pytest.raises(AssertionError):
        H.compare_decisions(rec, tr, 'ula', x0, _u, 'host')


# --------------------------------------------------------------------------------------------------- spy
def test_spy_counts_a_call_through_a_subclass_with_its_own_split_step(monkeypatch):
    from nfmc_amd.samplers import mcmc
    monkeypatch.setattr(mcmc.MALA, '_split_step', lambda self, *a, **k: 'ran', raising=False)   # as an earlier test may leave it
    spy = H.Spy(monkeypatch)
    assert mcmc.MALA._split_step(object()) == 'ran'
    assert spy.calls == [1]
