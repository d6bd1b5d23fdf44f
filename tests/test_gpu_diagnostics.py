"""GPU: nfmc_chain_diagnostics_f32 and the diagnostics built from its sums against the fp64 oracle
(diagnostics_fp64.py) on the same fp32 inputs: layout edges, the sliding window, grid stride, superchains, offset and
constant data, buffer bounds, status codes, repeatability, additivity over chains, and MCMCOutput.diagnostics end to end.

Tolerances.  The kernel takes the means, the half-chain sums and every cross-chain total in fp64 and
centres each draw in fp64 before rounding it to fp32, so what is left in the autocovariances is the fp32 rounding of the
centred draws and of their products summed over at most 300 draws per lag.  Worst figures over every case of this file,
one run on the MI355X:
    autocovariance sums   3.4e-7    (|error| of sum_j a_{j,l} over the lag-0 sum of the coordinate; lags cross zero)
    half-chain sums       3.4e-13   (sum_s2h relative; sum_mh, sum_mh2 against n x sd and its square)
    rhat, nested rhat, sd 1.6e-7    (relative; rhat itself rests on the fp64 half-chain sums alone: 4e-16)
    ess, mcse_mean        3.2e-7    (relative)
Each bound below is 4 x its figure.  The other fp64-only sums (chain means, superchains) are held to 1e-12 of their
scale: fp64 rounding, 1.1e-16 x sqrt(n), is 4e-14 for the 1.3e5 chains of the largest case (observed 3.2e-15)."""
import ctypes as C

import numpy as np
import pytest
import torch

import diagnostics_fp64 as ref
from nfmc_amd import diagnostics, hip

pytestmark = pytest.mark.gpu

TOL_ACOV = 1.4e-6
TOL_HALF = 1.4e-12
TOL_RHAT = 6.4e-7
TOL_ESS = 1.3e-6
TOL_FP64 = 1e-12
WORST = {'acov': 0.0, 'half': 0.0, 'rhat': 0.0, 'ess': 0.0, 'fp64': 0.0}


@pytest.fixture(scope='module')
def dev():
    return hip.require_gpu()


def _worst(key, value):
    WORST[key] = max(WORST[key], float(value))
    return float(value)


def check_sums(got, x, max_lag, group):
    """The kernel's sums against the oracle's, each on its natural scale."""
    want = ref.sums(x, max_lag, group)
    n = x.shape[1]
    g = {k: v.numpy() for k, v in got.items()}
    a0 = want['acov'][0]
    assert g['acov'].shape == want['acov'].shape
    live = a0 > 0
    assert (g['acov'][:, ~live] == 0).all()          # a constant coordinate has exact zeros
    sd = np.sqrt(a0 / n)                              # per-coordinate within-chain scale
    scale1 = np.abs(want['sum_m']) + n * sd + 1e-300  # sums of n means
    scale2 = want['sum_m2'] + n * sd * sd + 1e-300    # sums of n squared means
    if live.any():
        e = _worst('acov', (np.abs(g['acov'] - want['acov'])[:, live] / a0[live]).max())
        print('acov %.3g' % e, end=' ')
        assert e <= TOL_ACOV
        e = max((np.abs(g['sum_s2h'] - want['sum_s2h'])[live] / want['sum_s2h'][live]).max(),
                (np.abs(g['sum_mh'] - want['sum_mh']) / (2 * n * sd + 1e-300))[live].max(),
                (np.abs(g['sum_mh2'] - want['sum_mh2']) / (2 * scale2))[live].max())
        print('half %.3g' % _worst('half', e), end=' ')
        assert e <= TOL_HALF
    e = max((np.abs(g['sum_m'] - want['sum_m']) / scale1).max(), (np.abs(g['sum_m2'] - want['sum_m2']) / scale2).max(),
            (np.abs(g['sum_mu'] - want['sum_mu']) / scale1).max(), (np.abs(g['sum_mu2'] - want['sum_mu2']) / scale2).max(),
            (np.abs(g['sum_bt'] - want['sum_bt']) / scale2).max())
    print('fp64 %.3g' % _worst('fp64', e), end=' ')
    assert e <= TOL_FP64
    assert (g['sum_mh'][~live] == want['sum_mh'][~live]).all() and (g['sum_s2h'][~live] == 0).all()


def check_diag(got, x, max_lag, group):
    want = ref.direct(x, max_lag, group)
    for name, key, tol in (('rhat', 'rhat', TOL_RHAT), ('nested_rhat', 'rhat', TOL_RHAT), ('ess', 'ess', TOL_ESS),
                           ('mcse_mean', 'ess', TOL_ESS), ('sd', 'rhat', TOL_RHAT)):
        if name not in want:
            assert getattr(got, name) is None
            continue
        g, w = getattr(got, name).numpy().reshape(-1), want[name]
        assert (np.isnan(g) == np.isnan(w)).all(), name
        ok = ~np.isnan(w)
        assert (g[ok][w[ok] == 0] == 0).all(), name          # sd of a constant coordinate
        ok &= w != 0
        if ok.any():
            e = _worst(key, (np.abs(g[ok] - w[ok]) / np.abs(w[ok])).max())
            print('%s %.3g' % (name, e), end=' ')
            assert e <= tol, name
    assert (got.truncated.numpy().reshape(-1) == want['truncated']).all()
    rho_g, rho_w = got.autocorrelation.numpy().reshape(want['autocorrelation'].shape), want['autocorrelation']
    assert (np.isnan(rho_g) == np.isnan(rho_w)).all()
    assert np.nanmax(np.abs(rho_g - rho_w), initial=0.0) <= TOL_ACOV * 4   # rho_l = 1 - (W - A_l) / varp, against rho_0 = 1
    print()


def run_case(dev, x, max_lag, group=1):
    xd = torch.from_numpy(x).to(dev)
    got = diagnostics.chain_sums(xd, max_lag, group)
    check_sums(got, x, max_lag, group)
    check_diag(diagnostics.from_sums(got, x.shape[0], x.shape[1], group), x, max_lag, group)
    return got


def draws(seed, K, n, d, phi=0.5):
    return ref.ar1(np.random.default_rng(seed), K, n, d, phi, mean=0.3, sd=1.5)


@pytest.mark.parametrize('d', [1, 3, 5, 64, 257, 1024])
def test_layout_edges(dev, d):
    for n in (1, 7, 130):
        for K in (4, 5, 33):
            print('d=%d n=%d K=%d:' % (d, n, K), end=' ')
            run_case(dev, draws(d + n + K, K, n, d), K - 1, 1 if n != 7 else 7)


@pytest.mark.parametrize('K,n,d', [(300, 7, 5), (289, 3, 64), (65, 2, 70)])
def test_window_slides_over_time_tiles(dev, K, n, d):
    run_case(dev, draws(K, K, n, d, phi=0.9), 127)


@pytest.mark.parametrize('max_lag', [0, 1, 31, 32, 126, 127, hip.DIAG_MAX_LAG])
def test_max_lag_edges(dev, max_lag):
    run_case(dev, draws(max_lag, 140, 5, 3, phi=0.8), max_lag)


def test_max_lag_above_the_draws_is_clipped(dev):
    x = draws(9, 33, 6, 3)
    got = run_case(dev, x, 100)                        # the kernel itself: lags >= K are empty sums
    assert (got['acov'][33:] == 0).all() and (got['acov'][:33, :].abs() > 0).all()
    diag = diagnostics.diagnose(torch.from_numpy(x).to(dev), max_lag=100)
    assert diag.max_lag == 32 and diag.autocorrelation.shape == (33, 3)
    check_diag(diag, x, 100, None)


@pytest.mark.parametrize('K,n,d', [(8, 8200, 64), (6, 520, 1024), (4, 131072 + 70, 1), (4, 21 * 2048 + 5, 3)])
def test_grid_stride(dev, K, n, d):
    run_case(dev, draws(n, K, n, d), K - 1)


@pytest.mark.parametrize('M', [1, 2, 65, 130])
def test_superchains(dev, M):
    x = draws(M, 6, 130, 3)
    x[:, 65:] += 2.0                                   # the two halves disagree: the nested R-hat sees it at M = 65 only
    run_case(dev, x, 5, M)


def test_offset_data_keeps_its_precision(dev):
    """Mean 1e3, sd 1, AR(1) phi = 0.9: an uncentred fp32 sum of x_t x_{t+l} has lost the covariance altogether."""
    x = ref.ar1(np.random.default_rng(5), 300, 16, 4, 0.9, mean=1e3, sd=1.0)
    run_case(dev, x, 127, 4)


def test_constant_coordinate_and_constant_chain(dev):
    x = draws(21, 12, 8, 4)
    x[:, 3, :] = 1.5                                   # a chain that never moved
    x[:, :, 2] = -7.25                                 # a coordinate without any variance, in any chain
    got = run_case(dev, x, 11, 4)
    diag = diagnostics.from_sums(got, 12, 8, 4)
    for t in (diag.rhat, diag.nested_rhat, diag.ess, diag.mcse_mean):
        assert torch.isnan(t[2]) and torch.isfinite(t[[0, 1, 3]]).all()
    assert float(diag.mean[2]) == -7.25 and float(diag.sd[2]) == 0.0


# ------------------------------------------------------------------------------------------------ the C entry itself
CANARY = -1.2345e300


def raw_call(dev, x, K, n, d, max_lag, group, sums=True, work=True, short=0, null_x=False):
    """One call with canary words behind `sums` and `work`; returns (status, sums buffer, work buffer, their lengths)."""
    lib = hip.lib()
    ns = max(int(lib.nfmc_diag_sums_doubles(min(d, 1024), min(max_lag, hip.DIAG_MAX_LAG))), 8)
    nbytes = int(lib.nfmc_diag_work_bytes(n, min(d, 1024), min(max(max_lag, 0), hip.DIAG_MAX_LAG)))
    nw = max(nbytes // 8, 8)
    sb = torch.full((ns + 16,), CANARY, dtype=torch.float64, device=dev)
    wb = torch.full((nw + 16,), CANARY, dtype=torch.float64, device=dev)
    args = hip.NfmcDiagArgs(None if null_x else hip.ptr(x), K, n, d, max_lag, group, 0,
                            hip.ptr(sb, torch.float64) if sums else None, hip.ptr(wb, torch.float64) if work else None,
                            nbytes - short)
    rc = lib.nfmc_chain_diagnostics_f32(C.byref(args), hip.stream())
    torch.cuda.synchronize()
    return rc, sb.cpu(), wb.cpu(), ns, nw


@pytest.mark.parametrize('K,n,d,max_lag,group', [(9, 11, 3, 8, 1), (40, 5, 257, 20, 5), (5, 300, 64, 4, 3)])
def test_canaries_behind_sums_and_work_stay(dev, K, n, d, max_lag, group):
    x = torch.from_numpy(draws(1, K, n, d)).to(dev)
    rc, sb, wb, ns, nw = raw_call(dev, x, K, n, d, max_lag, group)
    assert rc == hip.OK
    assert ns == (hip.DIAG_ACOV + max_lag + 1) * d
    assert (sb[ns:] == CANARY).all() and (wb[nw:] == CANARY).all()
    assert (sb[:ns] != CANARY).all()                   # every word of sums is written
    want = diagnostics.pack_sums(diagnostics.chain_sums(x, max_lag, group))
    assert torch.equal(sb[:ns], want)


def test_status_codes_without_a_launch(dev):
    x = torch.from_numpy(draws(2, 8, 6, 3)).to(dev)
    ok = dict(K=8, n=6, d=3, max_lag=7, group=2)
    cases = [(dict(null_x=True), hip.EINVAL), (dict(sums=False), hip.EINVAL), (dict(work=False), hip.EINVAL),
             (dict(K=3), hip.EINVAL), (dict(K=0), hip.EINVAL), (dict(n=0), hip.EINVAL), (dict(d=0), hip.EINVAL),
             (dict(max_lag=-1), hip.EINVAL), (dict(group=0), hip.EINVAL), (dict(group=4), hip.EINVAL),
             (dict(d=1025), hip.ESHAPE), (dict(max_lag=hip.DIAG_MAX_LAG + 1), hip.ESHAPE), (dict(short=1), hip.ESCRATCH)]
    for change, code in cases:
        rc, sb, wb, _, _ = raw_call(dev, x, **{**ok, **change})
        assert rc == code, (change, rc)
        assert (sb == CANARY).all() and (wb == CANARY).all(), change
    lib = hip.lib()
    assert lib.nfmc_diag_sums_doubles(1025, 5) == 0 and lib.nfmc_diag_sums_doubles(4, 128) == 0
    assert lib.nfmc_diag_work_bytes(0, 4, 5) == 0 and lib.nfmc_diag_work_bytes(10, 4, -1) == 0
    with pytest.raises(ValueError):
        diagnostics.chain_sums(x, 128)


def test_two_calls_give_the_same_bits(dev):
    x = torch.from_numpy(draws(3, 40, 700, 70)).to(dev)
    a = diagnostics.pack_sums(diagnostics.chain_sums(x, 39, 7))
    b = diagnostics.pack_sums(diagnostics.chain_sums(x, 39, 7))
    assert torch.equal(a, b)


def test_sums_are_additive_over_chains(dev):
    """The shard contract: the sums of chains [0, n/2) plus those of [n/2, n) are the sums of all of them."""
    x = draws(4, 20, 260, 5)
    xd = torch.from_numpy(x).to(dev)
    whole = diagnostics.pack_sums(diagnostics.chain_sums(xd, 19, 10))
    parts = sum(diagnostics.pack_sums(diagnostics.chain_sums(xd[:, lo:lo + 130].contiguous(), 19, 10)) for lo in (0, 130))
    scale = diagnostics.pack_sums({k: torch.from_numpy(np.abs(v) if k != 'acov' else np.broadcast_to(v[0], v.shape).copy())
                                   for k, v in ref.sums(x, 19, 10).items()})
    assert ((whole - parts).abs() <= 1e-12 * scale).all(), ((whole - parts).abs() / scale).max()


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize('store', [{}, {'thinning': 3, 'max_samples': 10}])
def test_output_diagnostics_match_the_oracle_on_the_kept_states(dev, store):
    from nfmc_amd import sample
    from nfmc_amd.potentials import SumOfSquares
    out = sample(SumOfSquares((8,)), strategy='mala', n_chains=256, n_iterations=64, seed=17, show_progress=False,
                 param_kwargs=dict(store))
    diag = out.diagnostics(superchains=16)
    x = out.samples.numpy()
    K = 10 if store else 64
    assert x.shape == (K, 256, 8) and (diag.n_draws, diag.n_chains, diag.max_lag) == (K, 256, K - 1)
    assert diag.rhat.shape == (8,) and diag.autocorrelation.shape == (K, 8)
    check_diag(diag, x, K - 1, 16)
    assert np.isfinite(diag.summary()['max_nested_rhat'])


def test_host_resident_states_are_moved_to_the_device(dev):
    x = draws(6, 16, 12, 6).reshape(16, 12, 2, 3)
    diag = diagnostics.diagnose(torch.from_numpy(x), superchains=3)
    assert diag.rhat.shape == (2, 3) and diag.autocorrelation.shape == (16, 2, 3)
    check_diag(diag, x.reshape(16, 12, 6), 15, 3)


def test_report_worst_figures():
    """Last in the file: the worst figure of every kind over the cases above (the header's numbers)."""
    print('worst figures:', {k: '%.3g' % v for k, v in WORST.items()})
