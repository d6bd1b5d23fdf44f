"""GPU: nfmc_rank_series_f32 and the rank-normalised diagnostics built on it against the oracle (rank_fp64.py) on the
same fp32 inputs.

Exactness.  The two tail indicators, the order statistics and the non-finite counts equal the oracle bit for bit.  The
scores are held to |z_dev - fl32(z_ref)| <= 2^-23 max(|z_ref|, 1): one fp32 ulp for the single rounding of an fp64 value
whose algorithmic error (AS 241 on both sides, fused or not) is far below half an ulp.  At the sizes of this file
(S <= 2^18) the scores of neighbouring half-ranks are at least 1e-5 apart, so the bound pins every rank, the half-ranks of
ties included -- and with them the folded values f, which are only seen through the scores of their ranks.

Composition.  diagnose(rank_normalized=True) is held to diagnostics_fp64.direct applied to the device's own four series
read back, within the tolerances of test_gpu_diagnostics.py: the inputs are identical, so no new tolerance is needed."""
import ctypes as C

import numpy as np
import pytest
import torch

import diagnostics_fp64 as plain
import rank_fp64 as ref
from nfmc_amd import diagnostics, hip

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
TOL_RHAT = 6.4e-7      # tests/test_gpu_diagnostics.py
TOL_ESS = 1.3e-6
CANARY_F = -1.2345e30
CANARY_D = -1.2345e300
CANARY_I = -123456789
PAD = 16


@pytest.fixture(scope='module')
def dev():
    return hip.require_gpu()


def raw_call(dev, x, K, n, d, series, out=True, stats=True, nonfinite=True, work=True, short=0, null_x=False, alias=False):
    """One call with canary words behind every buffer: (status, out, order_stats, nonfinite, work) on the host, canaries
    included, and the byte length of work."""
    lib = hip.lib()
    dd = min(max(d, 1), 1024)
    nbytes = int(lib.nfmc_rank_work_bytes(max(K, 4), max(n, 1), dd))
    ne = max(K, 4) * max(n, 1) * dd
    ob = torch.full((ne + PAD,), CANARY_F, dtype=torch.float32, device=dev)
    sb = torch.full((4 * dd + PAD,), CANARY_D, dtype=torch.float64, device=dev)
    nb = torch.full((dd + PAD,), CANARY_I, dtype=torch.int32, device=dev)
    wb = torch.full((nbytes // 8 + PAD,), CANARY_D, dtype=torch.float64, device=dev)
    xp = None if null_x else hip.ptr(x)
    args = hip.NfmcRankArgs(xp, K, n, d, series, xp if alias else (hip.ptr(ob) if out else None),
                            hip.ptr(sb, torch.float64) if stats else None, hip.ptr(nb, torch.int32) if nonfinite else None,
                            hip.ptr(wb, torch.float64) if work else None, nbytes - short)
    rc = lib.nfmc_rank_series_f32(C.byref(args), hip.stream())
    torch.cuda.synchronize()
    return rc, ob.cpu(), sb.cpu(), nb.cpu(), wb.cpu(), nbytes


def device_series(dev, x, kind):
    """(series (K, n, d) fp32, order_stats (d, 4), nonfinite (d,)) as numpy; the canaries behind the buffers are checked."""
    K, n, d = x.shape
    xd = torch.from_numpy(x).to(dev)
    rc, ob, sb, nb, wb, nbytes = raw_call(dev, xd, K, n, d, hip.RANK_SERIES[kind])
    assert rc == hip.OK
    assert nbytes % 8 == 0
    assert (ob[K * n * d:] == CANARY_F).all() and (sb[4 * d:] == CANARY_D).all()
    assert (nb[d:] == CANARY_I).all() and (wb[nbytes // 8:] == CANARY_D).all()
    assert (bits32(xd.cpu().numpy()) == bits32(x)).all()   # x is only read
    return ob[:K * n * d].numpy().reshape(K, n, d), sb[:4 * d].numpy().reshape(d, 4), nb[:d].numpy()


def bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_exact(dev, x, kinds=ref.KINDS):
    """Every series of x, the order statistics and the counts against the oracle."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    bad = ref.nonfinite(x) > 0
    want_os = ref.order_stats(x)
    worst = 0.0
    for kind in kinds:
        got, os_, nf = device_series(dev, x, kind)
        assert (nf == ref.nonfinite(x)).all(), kind
        assert np.isnan(got[:, :, bad]).all(), kind
        assert (os_[~bad].view(np.int64) == want_os[~bad].view(np.int64)).all(), kind
        z = ref.series64(x, kind)[:, :, ~bad]
        g = got[:, :, ~bad]
        if kind in ('tail_low', 'tail_high'):
            assert (bits32(g) == bits32(z)).all(), kind
        else:
            err = np.abs(g.astype(np.float64) - z.astype(np.float32).astype(np.float64)) / np.maximum(np.abs(z), 1.0)
            if err.size:
                worst = max(worst, float(err.max()))
            assert (err <= ULP).all(), (kind, err.max() / ULP)
    print('score error %.3g ulp' % (worst / ULP), end=' ')


def draws(seed, K, n, d, phi=0.5):
    return plain.ar1(np.random.default_rng(seed), K, n, d, phi, mean=0.3, sd=1.5)


# ------------------------------------------------------------------------------------------------ shapes
@pytest.mark.parametrize('d', [1, 3, 5, 64, 65, 257, 1024])
def test_layout_edges(dev, d):
    for n in (1, 7, 130):
        for K in (4, 5, 33):
            print('d=%d n=%d K=%d:' % (d, n, K), end=' ')
            check_exact(dev, draws(d + n + K, K, n, d))
            print()


@pytest.mark.parametrize('K,n,d', [(5, 39323, 2), (4, 16385, 64), (6, 520, 1024)])
def test_past_a_scatter_block_and_past_the_grid(dev, K, n, d):
    """S = 96 x 2048 + 7; 33 tiles x 64 coordinates = 2112 tiles on a grid of 2048; 2 x 1024 tiles, the second one part full."""
    check_exact(dev, draws(n, K, n, d))


# ------------------------------------------------------------------------------------------------ data
SHAPES = [(4, 50, 3), (8, 300, 3)]       # S = 200: one part-full tile; S = 2400: a full tile and a part-full one


def scattered(values, K, n, d, seed):
    """Every coordinate holds `values` (S of them), in an order of its own."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(values) for _ in range(d)], axis=1).reshape(K, n, d).astype(np.float32)


@pytest.mark.parametrize('K,n,d', SHAPES)
def test_ar1_draws_and_repeated_states(dev, K, n, d):
    x = draws(1, K, n, d, phi=0.9)
    check_exact(dev, x)
    rng = np.random.default_rng(2)
    long = draws(3, 5 * K, n, d, phi=0.9)
    rep = np.empty_like(x)
    for j in range(n):                       # every state held for 1 to 5 draws: a chain that rejects
        idx = np.repeat(np.arange(5 * K), rng.integers(1, 6, 5 * K))[:K]
        rep[:, j] = long[idx, j]
    check_exact(dev, rep)


@pytest.mark.parametrize('K,n,d', SHAPES)
def test_seven_distinct_values_and_a_constant_coordinate(dev, K, n, d):
    x = np.random.default_rng(4).integers(-3, 4, (K, n, d)).astype(np.float32)
    check_exact(dev, x)
    x = draws(5, K, n, d)
    x[:, :, 1] = -7.25
    check_exact(dev, x)
    z, _, _ = device_series(dev, x, 'bulk')
    assert (z[:, :, 1] == 0).all()           # all ties: p = 1/2 exactly
    diag = diagnostics.diagnose(torch.from_numpy(x).to(dev), rank_normalized=True)
    for name in ('rhat_bulk', 'rhat_tail', 'rhat_rank', 'ess_bulk', 'ess_tail'):
        t = getattr(diag, name)
        assert torch.isnan(t[1]) and torch.isfinite(t[[0, 2]]).all(), name
    assert diag.summary()['n_nonfinite'] == 0


@pytest.mark.parametrize('K,n,d', SHAPES)
@pytest.mark.parametrize('sign', [1.0, -1.0])
def test_only_the_low_bits_vary(dev, K, n, d, sign):
    """1 + k 2^-23, k < S: at S = 200 every pass but the first sees one digit over the whole segment."""
    S = K * n
    values = sign * (1.0 + np.arange(S) * 2.0 ** -23)
    x = scattered(values, K, n, d, 6)
    assert len(np.unique(x[:, :, 0])) == S
    check_exact(dev, x)


@pytest.mark.parametrize('K,n,d', SHAPES)
def test_denormals_and_signed_zeros(dev, K, n, d):
    S = K * n
    k = np.arange(S) - S // 2
    values = (k * 2.0 ** -149).astype(np.float32)
    values[::7] = 0.0
    values[3::7] = -0.0
    x = scattered(values, K, n, d, 7)
    assert np.signbit(x[x == 0]).any() and not np.signbit(x[x == 0]).all()
    check_exact(dev, x)


@pytest.mark.parametrize('K,n,d', SHAPES)
def test_values_spanning_the_whole_range(dev, K, n, d):
    S = K * n
    rng = np.random.default_rng(8)
    values = (rng.choice([-1.0, 1.0], S) * 10.0 ** rng.uniform(-38, 38.47, S)).astype(np.float32)
    values[0], values[1] = 3e38, -3e38
    assert np.isfinite(values).all()
    check_exact(dev, scattered(values, K, n, d, 9))


@pytest.mark.parametrize('K,n,d', SHAPES)
@pytest.mark.parametrize('what', [np.nan, np.inf, -np.inf])
def test_a_nonfinite_value_flags_its_coordinate_only(dev, K, n, d, what):
    x = draws(10, K, n, d)
    x[K - 1, n // 2, 1] = what
    check_exact(dev, x)                      # the neighbours are exact, coordinate 1 is NaN and counted
    diag = diagnostics.diagnose(torch.from_numpy(x).to(dev), rank_normalized=True, superchains=2)
    assert diag.n_nonfinite.tolist() == [0, 1, 0] and diag.summary()['n_nonfinite'] == 1
    for name in ('rhat_bulk', 'rhat_tail', 'rhat_rank', 'ess_bulk', 'ess_tail', 'nested_rhat_bulk'):
        t = getattr(diag, name)
        assert torch.isnan(t[1]) and torch.isfinite(t[[0, 2]]).all(), name
    assert not bool(diag.truncated_bulk[1]) and not bool(diag.truncated_tail[1])


# ------------------------------------------------------------------------------------------------ composition
def check_fields(got, want, group):
    for name, tol in (('rhat_bulk', TOL_RHAT), ('rhat_tail', TOL_RHAT), ('rhat_rank', TOL_RHAT), ('ess_bulk', TOL_ESS),
                      ('ess_tail', TOL_ESS), ('nested_rhat_bulk', TOL_RHAT)):
        if name == 'nested_rhat_bulk' and group is None:
            assert got.nested_rhat_bulk is None
            continue
        g, w = getattr(got, name).numpy().reshape(-1), want[name]
        assert (np.isnan(g) == np.isnan(w)).all(), name
        ok = ~np.isnan(w)
        if ok.any():
            e = (np.abs(g[ok] - w[ok]) / np.abs(w[ok])).max()
            print('%s %.3g' % (name, e), end=' ')
            assert e <= tol, name
    assert (got.truncated_bulk.numpy().reshape(-1) == want['truncated_bulk']).all()
    assert (got.truncated_tail.numpy().reshape(-1) == want['truncated_tail']).all()
    print()


def composed(dev, x, max_lag, group, got=None):
    """diagnose(rank_normalized=True) -- or the result `got` of a caller's own path to it -- against the oracle's definitions
    applied to the device's own series."""
    xd = torch.from_numpy(x).to(dev)
    series = {k: diagnostics.rank_series(xd, k).cpu().numpy().astype(np.float64) for k in ref.KINDS}
    if got is None:
        got = diagnostics.diagnose(xd, max_lag=max_lag, superchains=group, rank_normalized=True)
    want = ref.from_series(series, max_lag, group)
    check_fields(got, want, group)
    tail = np.minimum(want['ess_tail_low'], want['ess_tail_high'])   # NaN where either indicator never changes within a chain
    g = got.ess_tail.numpy().reshape(-1)
    assert (np.isnan(g) == np.isnan(tail)).all()
    assert (np.abs(g - tail)[~np.isnan(tail)] <= TOL_ESS * tail[~np.isnan(tail)]).all()
    assert torch.equal(got.rhat_rank, torch.maximum(got.rhat_bulk, got.rhat_tail))
    return got, series


@pytest.mark.parametrize('M', [None, 1, 65])
def test_diagnose_composes_the_series(dev, M):
    x = draws(11, 33, 130, 5, phi=0.7)
    x[:, 65:, 0] *= 3.0                      # a scale mixture in coordinate 0: the folded R-hat and the tail ESS see it
    x[:, 65:, 1] += 2.0                      # the two halves disagree in location: the nested R-hat sees it at M = 65
    got, series = composed(dev, x, 32, M)
    for k in ref.KINDS:                      # rank_series is the entry point's output
        assert (bits32(series[k]) == bits32(device_series(dev, x, k)[0])).all()
    # oracle alone on these draws: rhat_tail 1.189 in coordinate 0, at most 1.072 elsewhere; nested_rhat_bulk at M = 65
    # 1.339 in coordinate 1, at most 1.008 elsewhere
    assert float(got.rhat_tail[0]) > 1.15 > float(got.rhat_tail[1:].max())
    if M == 65:
        assert float(got.nested_rhat_bulk[1]) > 1.3 > 1.02 > float(got.nested_rhat_bulk[[0, 2, 3, 4]].max())
    s = got.summary()
    assert s['max_rhat_rank'] == float(got.rhat_rank.max()) and s['min_ess_tail'] == float(got.ess_tail.min())
    assert s['min_ess_bulk'] == float(got.ess_bulk.min()) and s['n_nonfinite'] == 0


def test_the_plain_fields_do_not_change_with_the_keyword(dev):
    x = torch.from_numpy(draws(12, 20, 16, 6)).to(dev).reshape(20, 16, 2, 3)
    a = diagnostics.diagnose(x, superchains=4)
    b = diagnostics.diagnose(x, superchains=4, rank_normalized=True)
    for name in ('rhat', 'nested_rhat', 'ess', 'mcse_mean', 'mean', 'sd', 'truncated', 'autocorrelation'):
        assert torch.equal(getattr(a, name), getattr(b, name), ), name
    for name in ('rhat_bulk', 'rhat_tail', 'rhat_rank', 'ess_bulk', 'ess_tail', 'truncated_bulk', 'truncated_tail',
                 'nested_rhat_bulk', 'n_nonfinite'):
        assert getattr(a, name) is None and getattr(b, name).shape == (2, 3), name
    assert diagnostics.rank_series(x, 'folded').shape == x.shape
    assert diagnostics.rank_series(x.cpu(), 'tail_low').is_cuda      # host-resident states are moved to the device


# ------------------------------------------------------------------------------------------------ the C entry itself
@pytest.mark.parametrize('K,n,d', [(9, 11, 3), (40, 5, 257), (5, 300, 64)])
def test_canaries_stay_and_every_word_is_written(dev, K, n, d):
    x = draws(13, K, n, d)
    xd = torch.from_numpy(x).to(dev)
    keep = xd.clone()
    for kind, code in hip.RANK_SERIES.items():
        rc, ob, sb, nb, wb, nbytes = raw_call(dev, xd, K, n, d, code)
        assert rc == hip.OK
        ne = K * n * d
        assert (ob[ne:] == CANARY_F).all() and (sb[4 * d:] == CANARY_D).all()
        assert (nb[d:] == CANARY_I).all() and (wb[nbytes // 8:] == CANARY_D).all()
        assert (ob[:ne] != CANARY_F).all() and (sb[:4 * d] != CANARY_D).all() and (nb[:d] == 0).all()
        assert torch.equal(xd, keep), kind   # x is unchanged
        rc, ob2, _, _, _, _ = raw_call(dev, xd, K, n, d, code, stats=False)   # order_stats may be NULL
        assert rc == hip.OK and torch.equal(ob, ob2)
    S = K * n
    assert nbytes == 32 * d + 8 * S * d + 1024 * d * ((S + 2047) // 2048)     # the bound the header states


def test_status_codes_without_a_launch(dev):
    x = torch.from_numpy(draws(14, 8, 6, 3)).to(dev)
    ok = dict(K=8, n=6, d=3, series=hip.RANK_FOLDED)
    cases = [(dict(null_x=True), hip.EINVAL), (dict(out=False), hip.EINVAL), (dict(nonfinite=False), hip.EINVAL),
             (dict(work=False), hip.EINVAL), (dict(alias=True), hip.EINVAL), (dict(K=3), hip.EINVAL), (dict(n=0), hip.EINVAL),
             (dict(d=0), hip.EINVAL), (dict(series=4), hip.EINVAL), (dict(series=-1), hip.EINVAL),
             (dict(d=1025), hip.ESHAPE), (dict(K=1 << 20, n=1 << 11), hip.ESHAPE), (dict(short=1), hip.ESCRATCH)]
    keep = x.clone()
    for change, code in cases:
        if change.get('K', 0) > 8:           # S = 2^31: no buffers of that size, the shape is refused before they matter
            lib = hip.lib()
            one, count = torch.zeros(8, device=dev), torch.zeros(8, dtype=torch.int32, device=dev)
            args = hip.NfmcRankArgs(hip.ptr(x), change['K'], change['n'], 1, 0, hip.ptr(one), None,
                                    hip.ptr(count, torch.int32), hip.ptr(one), 1 << 40)
            assert lib.nfmc_rank_series_f32(C.byref(args), hip.stream()) == code
            continue
        rc, ob, sb, nb, wb, _ = raw_call(dev, x, **{**ok, **change})
        assert rc == code, (change, rc)
        assert (ob == CANARY_F).all() and (sb == CANARY_D).all() and (nb == CANARY_I).all() and (wb == CANARY_D).all(), change
        assert torch.equal(x, keep), change
    lib = hip.lib()
    assert lib.nfmc_rank_work_bytes(8, 6, 1025) == 0 and lib.nfmc_rank_work_bytes(3, 6, 3) == 0
    assert lib.nfmc_rank_work_bytes(8, 0, 3) == 0 and lib.nfmc_rank_work_bytes(1 << 20, 1 << 11, 1) == 0
    assert lib.nfmc_rank_work_bytes(8, 6, 3) > 0
    with pytest.raises(ValueError):
        diagnostics.rank_series(torch.zeros(8, 6, 1025, device=dev), 'bulk')
    with pytest.raises(ValueError):
        diagnostics.rank_series(x, 'middle')


def test_two_calls_give_the_same_bits(dev):
    x = draws(15, 40, 700, 70)
    x[1::2] = x[0::2]                        # ties
    xd = torch.from_numpy(x).to(dev)
    for kind in ref.KINDS:
        a = diagnostics.rank_series(xd, kind).clone()
        b = diagnostics.rank_series(xd, kind)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), kind


# ------------------------------------------------------------------------------------------------ end to end
def test_output_diagnostics_rank_normalized_on_the_funnel(dev):
    from nfmc_amd import sample
    from nfmc_amd.potentials import Funnel
    out = sample(Funnel((8,)), strategy='mala', n_chains=64, n_iterations=40, seed=23, show_progress=False,
                 param_kwargs=dict(store_samples=True))
    x = out.samples.numpy()
    assert x.shape == (40, 64, 8)
    before = out.diagnostics(superchains=8)
    for name in ('rhat_bulk', 'rhat_tail', 'rhat_rank', 'ess_bulk', 'ess_tail', 'truncated_bulk', 'truncated_tail',
                 'nested_rhat_bulk', 'n_nonfinite'):
        assert getattr(before, name) is None, name
    got = out.diagnostics(superchains=8, rank_normalized=True)
    for name in ('rhat', 'nested_rhat', 'ess', 'mcse_mean', 'mean', 'sd', 'truncated', 'autocorrelation'):
        assert torch.equal(getattr(before, name), getattr(got, name)), name
    want = plain.direct(x, 39, 8)            # the plain fields are what they were: the oracle of test_gpu_diagnostics.py
    assert (np.abs(before.rhat.numpy() - want['rhat']) <= TOL_RHAT * want['rhat']).all()
    assert (np.abs(before.ess.numpy() - want['ess']) <= TOL_ESS * want['ess']).all()
    # the rank fields of the output's own call: the oracle's series from the kept states are the device's (check_exact),
    # and `got` holds the definitions applied to them, every field with its NaN pattern (composed)
    check_exact(dev, x)
    composed(dev, x, 39, 8, got=got)
    assert got.n_nonfinite.tolist() == [0] * 8 and got.rhat_rank.shape == (8,) and got.nested_rhat_bulk.shape == (8,)
    # max_lag and superchains reach the rank fields as they reach the plain ones
    short = out.diagnostics(max_lag=10, rank_normalized=True)
    assert short.max_lag == 10 and short.nested_rhat_bulk is None and short.nested_rhat is None
    composed(dev, x, 10, None, got=short)
    # and it is the device-resident store that is diagnosed: the same bits as a call on the states themselves
    again = diagnostics.diagnose(torch.from_numpy(x).to(dev), superchains=8, rank_normalized=True)
    for name in ('rhat_bulk', 'rhat_tail', 'rhat_rank', 'ess_bulk', 'ess_tail', 'nested_rhat_bulk', 'truncated_bulk',
                 'truncated_tail', 'n_nonfinite'):
        a, b = getattr(got, name), getattr(again, name)
        assert torch.equal(torch.nan_to_num(a.double(), nan=-1.0), torch.nan_to_num(b.double(), nan=-1.0)), name
