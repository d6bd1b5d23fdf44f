"""GPU: the running diagnostics (nfmc_diag_stream_*_f32) against the fp64 oracle (diagnostics_fp64.py)
applied to the concatenation of all draws fed.  Every entry-point case feeds an AR(1) slab to the update in blocks,
through a staging ring that is smaller than the slab and wraps, with guard words behind the state, the ring, `sums` and
`work` that are compared after every call.  Through `sample()` the ring has min(128, kept draws) rows: the 70-transition
cases fill it without wrapping, test_cutting_the_launches_leaves_the_chain_alone (300 transitions) wraps it.

Tolerances: those the diagnostics of the kept states hold (test_gpu_diagnostics.py), against the same oracle, but for
the ESS.  The accumulator takes the shifted sums, the half-chain sums and every cross-chain total in fp64; what is left in
the autocovariances is the fp32 rounding of the shifted draws and of their products, summed in fp32 over one block of
draws per chain (at most 32 in the entry-point cases, up to 128 through `sample()`) and in fp64 from there on.  The
draws are shifted by the chain's first draw, not centred on its mean, so a chain whose first draw lies 2 to 3 sd out carries products several times larger than the centred ones, and
with a single chain nothing averages that out.  Worst figures over every case of this file (the
end-to-end cases on the 128-row default ring), one run on the MI355X:
    autocovariance sums   8.7e-7    (n = 1, d = 1024; bound 1.4e-6 as for the kept states)
    half-chain sums       1.5e-13   (bound 1.4e-12)
    rhat, nested rhat, sd 3.2e-7    (bound 6.4e-7)
    ess, mcse_mean        1.31e-6   (n = 1, d = 257: over the kept states' 1.3e-6, so this bound is 4 x the figure, 5.3e-6)
    fp64-only sums        4.2e-16   (bound 1e-12)"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import diagnostics_fp64 as ref
from nfmc_amd import diagnostics, hip

pytestmark = pytest.mark.gpu

TOL_ACOV = 1.4e-6
TOL_HALF = 1.4e-12
TOL_RHAT = 6.4e-7
TOL_ESS = 5.3e-6
TOL_FP64 = 1e-12
WORST = {'acov': 0.0, 'half': 0.0, 'rhat': 0.0, 'ess': 0.0, 'fp64': 0.0}
GUARD = -1.2345e300
NGUARD = 16
PATTERN = [1, 5, 13, 2, 16]     # K = 37: a block of one draw, blocks shorter and longer than L = 12, one across h = 18


@pytest.fixture(scope='module')
def dev():
    return hip.require_gpu()


def _worst(key, value):
    WORST[key] = max(WORST[key], float(value))
    return float(value)


def check_sums(got, x, max_lag, group, halves=True):
    """The accumulator's sums against the oracle's on the draws fed, each on its natural scale."""
    want = ref.sums(x, max_lag, group)
    n = x.shape[1]
    g = {k: v.numpy() for k, v in got.items()}
    a0 = want['acov'][0]
    assert g['acov'].shape == want['acov'].shape
    live = a0 > 0
    assert (g['acov'][:, ~live] == 0).all()          # a constant coordinate has exact zeros
    assert (g['acov'][x.shape[0]:] == 0).all()       # lags at or beyond K are exact zeros
    sd = np.sqrt(a0 / n)
    scale1 = np.abs(want['sum_m']) + n * sd + 1e-300
    scale2 = want['sum_m2'] + n * sd * sd + 1e-300
    if live.any():
        e = _worst('acov', (np.abs(g['acov'] - want['acov'])[:, live] / a0[live]).max())
        print('acov %.3g' % e, end=' ')
        assert e <= TOL_ACOV
        if halves:
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
    if halves:
        assert (g['sum_mh'][~live] == want['sum_mh'][~live]).all() and (g['sum_s2h'][~live] == 0).all()
    else:
        assert all(np.isnan(g[k]).all() for k in ('sum_mh', 'sum_mh2', 'sum_s2h'))


def check_fields(got, want, nan_rhat=False):
    """`got` (a Diagnostics) against `want` (the oracle's dict, or another Diagnostics of the same draws)."""
    def field(src, name):
        v = src[name] if isinstance(src, dict) else getattr(src, name)
        return None if v is None else np.asarray(v.numpy() if torch.is_tensor(v) else v).reshape(-1)
    for name, key, tol in (('rhat', 'rhat', TOL_RHAT), ('nested_rhat', 'rhat', TOL_RHAT), ('ess', 'ess', TOL_ESS),
                           ('mcse_mean', 'ess', TOL_ESS), ('sd', 'rhat', TOL_RHAT), ('mean', 'rhat', TOL_RHAT)):
        if isinstance(want, dict) and name not in want:
            assert getattr(got, name) is None
            continue
        g, w = field(got, name), field(want, name)
        if name == 'rhat' and nan_rhat:
            assert np.isnan(g).all()
            continue
        assert (np.isnan(g) == np.isnan(w)).all(), name
        ok = ~np.isnan(w)
        assert (g[ok][w[ok] == 0] == 0).all(), name
        ok &= w != 0
        if ok.any():
            e = _worst(key, (np.abs(g[ok] - w[ok]) / np.abs(w[ok])).max())
            print('%s %.3g' % (name, e), end=' ')
            assert e <= tol, name
    assert (field(got, 'truncated') == field(want, 'truncated')).all()
    rho_g, rho_w = field(got, 'autocorrelation'), field(want, 'autocorrelation')
    assert rho_g.shape == rho_w.shape and (np.isnan(rho_g) == np.isnan(rho_w)).all()
    assert np.nanmax(np.abs(rho_g - rho_w), initial=0.0) <= TOL_ACOV * 4
    print()


class Guarded:
    """A device buffer of `count` elements with NGUARD guard words behind it."""

    def __init__(self, count, dtype, dev):
        self.count = int(count)
        self.full = torch.full((self.count + NGUARD,), GUARD if dtype == torch.float64 else -7.5e37, dtype=dtype, device=dev)
        self.guard = self.full[self.count:].clone()
        self.t = self.full[:self.count]

    def intact(self):
        return torch.equal(self.full[self.count:], self.guard)


class Acc:
    """The entry points on guarded buffers.  The ring has `ring_rows` rows and the first block starts at row `row`."""

    def __init__(self, dev, n, d, L, planned, ring_rows, row=0):
        self.lib = hip.lib()
        self.dev, self.n, self.d, self.L = dev, n, d, L
        nbytes = int(self.lib.nfmc_diag_stream_state_bytes(n, d, L))
        assert nbytes > 0 and nbytes % 8 == 0
        self.state = Guarded(nbytes // 8, torch.float64, dev)
        self.ring = Guarded(ring_rows * n * d, torch.float32, dev)
        self.ring_rows, self.row = ring_rows, row
        self.desc = hip.NfmcDiagStream(hip.ptr(self.state.t, torch.float64), nbytes, n, d, L, planned, -1)
        assert self.lib.nfmc_diag_stream_reset_f32(C.byref(self.desc), hip.stream()) == hip.OK
        assert self.desc.n_seen == 0 and self.intact()

    def intact(self):
        torch.cuda.synchronize()
        return self.state.intact() and self.ring.intact()

    def feed(self, block):
        """One block (b, n, d) through the ring: rows row .. row + b - 1 mod ring_rows."""
        b = block.shape[0]
        ring = self.ring.t.view(self.ring_rows, self.n, self.d)
        rows = torch.arange(self.row, self.row + b, device=self.dev) % self.ring_rows
        ring.index_copy_(0, rows, torch.from_numpy(np.ascontiguousarray(block)).to(self.dev))
        seen = int(self.desc.n_seen)
        args = hip.NfmcDiagStreamArgs(C.pointer(self.desc), hip.ptr(self.ring.t), self.ring_rows, self.row, b, 0, seen)
        rc = self.lib.nfmc_diag_stream_update_f32(C.byref(args), hip.stream())
        assert rc == hip.OK, rc
        assert self.desc.n_seen == seen + b and self.intact()
        self.row = (self.row + b) % self.ring_rows

    def sums(self, group=1):
        ns = int(self.lib.nfmc_diag_sums_doubles(self.d, self.L))
        nw = int(self.lib.nfmc_diag_stream_work_bytes(self.n, self.d, self.L))
        assert ns == (hip.DIAG_ACOV + self.L + 1) * self.d and nw > 0
        sb, wb = Guarded(ns, torch.float64, self.dev), Guarded(nw // 8, torch.float64, self.dev)
        before = self.state.t.clone()
        args = hip.NfmcDiagStreamSumsArgs(C.pointer(self.desc), group, 0, hip.ptr(sb.t, torch.float64),
                                          hip.ptr(wb.t, torch.float64), nw)
        assert self.lib.nfmc_diag_stream_sums_f32(C.byref(args), hip.stream()) == hip.OK
        assert self.intact() and sb.intact() and wb.intact()
        assert (sb.t != GUARD).all()                                  # every word of sums is written
        assert torch.equal(self.state.t.view(torch.int64), before.view(torch.int64))   # the state is only read
        return sb.t.cpu()


def feed_all(dev, x, blocks, L, planned=None, ring_rows=None, row=None, peek=None):
    """Feeds the leading sum(blocks) draws of x in `blocks`; `peek`: block indices after which the sums are also taken."""
    K, n, d = x.shape
    ring_rows = ring_rows or max(blocks) + 1
    acc = Acc(dev, n, d, L, K if planned is None else planned, ring_rows, ring_rows - 1 if row is None else row)
    t = 0
    for i, b in enumerate(blocks):
        acc.feed(x[t:t + b])
        t += b
        if peek and i in peek:
            acc.sums()
    return acc


def run_case(dev, x, blocks, L, group=1, **kw):
    acc = feed_all(dev, x, blocks, L, **kw)
    K = sum(blocks)
    flat = acc.sums(group)
    got = diagnostics.unpack_sums(flat, x.shape[2])
    whole = K == (kw.get('planned') or x.shape[0])
    check_sums(got, x[:K], L, group, halves=whole)
    check_fields(diagnostics.from_sums(got, K, x.shape[1], group), ref.direct(x[:K], L, group), nan_rhat=not whole)
    return flat


def draws(seed, K, n, d, phi=0.5, mean=0.3, sd=1.5):
    return ref.ar1(np.random.default_rng(seed), K, n, d, phi, mean=mean, sd=sd)


# ------------------------------------------------------------------------------------------------ the accumulator
@pytest.mark.parametrize('d', [1, 3, 64, 257, 1024])
def test_layout_edges(dev, d):
    for n in (1, 7, 130):
        print('d=%d n=%d:' % (d, n), end=' ')
        run_case(dev, draws(d + n, 37, n, d), PATTERN, 12, 1 if n != 7 else 7)


def test_grid_stride(dev):
    run_case(dev, draws(1, 8, 70000, 1), [3, 5], 4)


@pytest.mark.parametrize('K,L,blocks', [(37, 0, PATTERN), (300, 127, [32] * 9 + [12]), (5, 8, [1] * 5)])
def test_lags(dev, K, L, blocks):
    run_case(dev, draws(K, K, 5, 3, phi=0.9), blocks, L)


def test_a_small_ring_wraps(dev):
    """4 rows, the first block of 3 rows at row 3; later a block of exactly ring_rows."""
    run_case(dev, draws(4, 21, 9, 5), [3, 4, 1, 4, 2, 3, 4], 6, 3, ring_rows=4, row=3)


def test_offset_data_keeps_its_precision(dev):
    run_case(dev, ref.ar1(np.random.default_rng(5), 300, 16, 4, 0.9, mean=1000.0, sd=1.5), [32] * 9 + [12], 127, 4)


def test_constant_coordinate_and_constant_chain(dev):
    x = draws(21, 37, 8, 4)
    x[:, 3, :] = 1.5
    x[:, :, 2] = -7.25
    got = diagnostics.unpack_sums(run_case(dev, x, PATTERN, 12, 4), 4)
    diag = diagnostics.from_sums(got, 37, 8, 4)
    assert (got['acov'][:, 2] == 0).all()
    for t in (diag.rhat, diag.nested_rhat, diag.ess, diag.mcse_mean):
        assert torch.isnan(t[2]) and torch.isfinite(t[[0, 1, 3]]).all()
    assert float(diag.mean[2]) == -7.25 and float(diag.sd[2]) == 0.0


@pytest.mark.parametrize('n', [10, 130])
def test_superchains(dev, n):
    x = draws(n, 37, n, 3)
    x[:, n // 2:] += 2.0
    acc = feed_all(dev, x, PATTERN, 12)
    for M in (1, 2, 5, n):          # n: a single superchain, NaN
        got = diagnostics.unpack_sums(acc.sums(M), 3)
        check_sums(got, x, 12, M)
        diag = diagnostics.from_sums(got, 37, n, M)
        check_fields(diag, ref.direct(x, 12, M))
        assert torch.isnan(diag.nested_rhat).all() == (M == n)


def test_invariants(dev):
    x = draws(3, 37, 130, 70)
    a = run_case(dev, x, PATTERN, 12, 5)
    b = feed_all(dev, x, PATTERN, 12).sums(5)
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))                 # the same blocks: the same bits
    c = feed_all(dev, x, PATTERN, 12, peek={2, 3}).sums(5)
    assert torch.equal(a.view(torch.int64), c.view(torch.int64))                 # reading the sums in mid-run changes nothing
    other = run_case(dev, x, [7, 30], 12, 5)                                     # other blocks: within the tolerances
    a0 = diagnostics.unpack_sums(a, 70)['acov'][0]
    ga, go = diagnostics.unpack_sums(a, 70), diagnostics.unpack_sums(other, 70)
    assert ((ga['acov'] - go['acov']).abs() / a0).max() <= 2 * TOL_ACOV
    for name in hip.DIAG_ROWS:
        assert ((ga[name] - go[name]).abs() <= 2 * TOL_FP64 * (ga[name].abs() + 130 * a0.sqrt())).all(), name


def test_sums_are_additive_over_chains(dev):
    x = draws(4, 37, 130, 5)
    whole = feed_all(dev, x, PATTERN, 12).sums(10)
    parts = sum(feed_all(dev, np.ascontiguousarray(x[:, lo:hi]), PATTERN, 12).sums(10) for lo, hi in ((0, 60), (60, 130)))
    scale = diagnostics.pack_sums({k: torch.from_numpy(np.abs(v) if k != 'acov' else np.broadcast_to(v[0], v.shape).copy())
                                   for k, v in ref.sums(x, 12, 10).items()})
    assert ((whole - parts).abs() <= TOL_FP64 * scale).all(), ((whole - parts).abs() / scale).max()


def test_an_early_end(dev):
    """40 draws planned, 25 fed: everything but the half-chain rows is that of x[:25]; from_sums gives a NaN rhat."""
    x = draws(8, 40, 9, 5)
    run_case(dev, x, [7, 2, 16], 12, 3, planned=40)


# ------------------------------------------------------------------------------------------------ the C entries
def test_size_functions_refuse_what_is_out_of_range(dev):
    lib = hip.lib()
    for fn in (lib.nfmc_diag_stream_state_bytes, lib.nfmc_diag_stream_work_bytes):
        assert fn(10, 4, 5) > 0 and fn(1, 1024, 127) > 0 and fn(3, 1, 0) > 0
        assert fn(0, 4, 5) == 0 and fn(10, 0, 5) == 0 and fn(10, 1025, 5) == 0 and fn(10, 4, -1) == 0 and fn(10, 4, 128) == 0
    n, d, L = 65536, 64, 127
    S, nb = n * d, 1024
    assert lib.nfmc_diag_stream_state_bytes(n, d, L) == 8 * (5 * S + nb * (L + 1) * d) + 4 * (1 + 2 * L) * S
    assert lib.nfmc_diag_stream_state_bytes(7, 3, 2) == (8 * (5 * 21 + 1 * 3 * 3) + 4 * 5 * 21 + 7) // 8 * 8


def test_status_codes_without_a_launch(dev):
    lib = hip.lib()
    x = draws(2, 8, 6, 3)
    acc = feed_all(dev, x, [3], 7, ring_rows=4, row=0)
    state0, ring0 = acc.state.full.clone(), acc.ring.full.clone()
    EINVAL, ESHAPE, ESCRATCH = hip.EINVAL, hip.ESHAPE, hip.ESCRATCH

    def desc(**change):
        dsc = hip.NfmcDiagStream(acc.desc.state, acc.desc.state_bytes, 6, 3, 7, 8, acc.desc.n_seen)
        for k, v in change.items():
            setattr(dsc, k, v)
        return dsc

    bad_desc = [(dict(state=None), EINVAL), (dict(n=0), EINVAL), (dict(d=0), EINVAL), (dict(max_lag=-1), EINVAL),
                (dict(n_draws_planned=0), EINVAL), (dict(d=1025), ESHAPE), (dict(max_lag=128), ESHAPE),
                (dict(state_bytes=acc.desc.state_bytes - 1), ESCRATCH)]

    def update(dsc, **change):
        kw = dict(acc=C.pointer(dsc), ring=hip.ptr(acc.ring.t), ring_rows=4, row=3, n_rows=2, reserved=0, first_draw=3)
        kw.update(change)
        return lib.nfmc_diag_stream_update_f32(C.byref(hip.NfmcDiagStreamArgs(**kw)), hip.stream())

    def sums(dsc, short=0, **change):
        ns, nw = int(lib.nfmc_diag_sums_doubles(3, 7)), int(lib.nfmc_diag_stream_work_bytes(6, 3, 7))
        sb, wb = Guarded(ns, torch.float64, dev), Guarded(nw // 8, torch.float64, dev)
        kw = dict(acc=C.pointer(dsc), group=2, reserved=0, sums=hip.ptr(sb.full, torch.float64),
                  work=hip.ptr(wb.full, torch.float64), work_bytes=nw - short)
        kw.update(change)
        rc = lib.nfmc_diag_stream_sums_f32(C.byref(hip.NfmcDiagStreamSumsArgs(**kw)), hip.stream())
        torch.cuda.synchronize()
        assert (sb.full == GUARD).all() and (wb.full == GUARD).all()
        return rc

    for change, code in bad_desc:
        assert lib.nfmc_diag_stream_reset_f32(C.byref(desc(**change)), hip.stream()) == code, change
        assert update(desc(**change)) == code, change
        assert sums(desc(n_seen=8, **change)) == code, change
    assert lib.nfmc_diag_stream_reset_f32(None, hip.stream()) == EINVAL
    assert lib.nfmc_diag_stream_update_f32(None, hip.stream()) == EINVAL
    assert lib.nfmc_diag_stream_sums_f32(None, hip.stream()) == EINVAL
    for change in (dict(ring=None), dict(acc=None), dict(ring_rows=0), dict(n_rows=0), dict(n_rows=5), dict(row=4), dict(row=-1),
                   dict(first_draw=2), dict(first_draw=4),        # a repeated and a dropped draw
                   dict(n_rows=4, ring_rows=8, row=0, first_draw=3, acc=C.pointer(desc(n_draws_planned=6)))):   # past the plan
        dsc = desc()
        assert update(dsc, **change) == EINVAL, change
        assert dsc.n_seen == 3
    for change in (dict(sums=None), dict(work=None), dict(acc=None), dict(group=0), dict(group=4)):
        assert sums(desc(n_seen=8), **change) == EINVAL, change
    assert sums(desc(n_seen=3)) == EINVAL                         # fewer than 4 draws
    assert sums(desc(n_seen=8), short=1) == ESCRATCH
    torch.cuda.synchronize()
    assert torch.equal(acc.state.full.view(torch.int64), state0.view(torch.int64)) and torch.equal(acc.ring.full, ring0)
    with pytest.raises(ValueError):
        diagnostics.RunningDiagnostics(6, 3, dev, 128, 10)


# ------------------------------------------------------------------------------------------------ end to end
def _sumsq(x):
    return 0.5 * (x * x).flatten(1).sum(dim=1)


E2E = [
    # id, strategy, target, d, n_iterations, extra keywords of sample(), extra param_kwargs
    ('mala', 'mala', 'sumsq', 5, 70, {}, {}),
    ('mala-d64', 'mala', 'sumsq', 64, 70, {}, {}),
    ('mala-thinned', 'mala', 'funnel', 5, 70, {}, {'thinning': 3}),
    ('mala-split', 'mala', 'callable', 5, 70, {'fuse': 'never'}, {}),
    ('hmc', 'hmc', 'funnel', 5, 70, {}, {}),
    ('jump_mala', 'jump_mala', 'sumsq', 5, 3, {'inner_param_kwargs': {'n_iterations': 20}}, {}),
    ('imh', 'imh', 'sumsq', 5, 70, {}, {}),
    ('neutra_hmc', 'neutra_hmc', 'funnel', 5, 70, {}, {}),
    ('neutra_mh', 'neutra_mh', 'sumsq', 5, 70, {}, {}),
    ('dlmc', 'dlmc', 'sumsq', 5, 40, {'negative_log_likelihood': _sumsq}, {}),
]


@pytest.fixture
def launches(monkeypatch):
    """Records the (first transition, transitions) of every launch that `Run.launches` hands out, per sample() call."""
    from nfmc_amd.samplers import common
    calls = []
    plain = common.Run.launches

    def recording(self, *args, **kw):
        calls.append([])
        for item in plain(self, *args, **kw):
            calls[-1].append(item)
            yield item
    monkeypatch.setattr(common.Run, 'launches', recording)
    return calls


@pytest.mark.parametrize('case', E2E, ids=[c[0] for c in E2E])
def test_a_run_with_the_option_on_matches_the_kept_states(dev, case, launches):
    from nfmc_amd import sample
    from nfmc_amd.potentials import Funnel, SumOfSquares
    _, strategy, kind, d, T, kw, pk = case
    target = {'sumsq': lambda: SumOfSquares((d,)), 'funnel': lambda: Funnel((d,), 3.0), 'callable': lambda: _sumsq}[kind]
    x0 = torch.randn(64, d, generator=torch.Generator().manual_seed(3))

    def run(**params):
        torch.manual_seed(11)   # the flow's initial weights and the refits' batches
        # a far-away time limit: a watched run's launches (32 transitions at most) are shorter than what the staging ring
        # allows, so the three runs are cut alike (asserted below) and their pooled moments are summed in the same order
        return sample(target(), event_shape=(d,), strategy=strategy, x0=x0.clone(), n_iterations=T, seed=17,
                      show_progress=False, sampling_time_limit_seconds=1e9, param_kwargs={**pk, **params}, **kw)

    a = run(store_samples=False, running_diagnostics=12)
    b = run(store_samples=True)
    c = run(store_samples=False)
    assert a.samples is None and a.running is not None and c.running is None
    # the premise of the bitwise moments below: a watched run's launches are no longer than what the ring allows, so the
    # three runs were cut alike (the samplers that do not go through Run.launches record nothing)
    assert len(launches) in (0, 3) and all(seq == launches[0] for seq in launches), launches
    assert torch.equal(a.running_samples.last_sample, c.running_samples.last_sample)
    assert torch.equal(a.mean, c.mean) and torch.equal(a.variance, c.variance)
    sa, sc = a.statistics.as_dict(), c.statistics.as_dict()
    for name in a.statistics.COUNTERS + ('n_nonfinite_log_ratios',):
        assert getattr(a.statistics, name) == getattr(c.statistics, name), name
    assert sa.keys() == sc.keys()
    assert torch.equal(a.running_samples.last_sample, b.running_samples.last_sample)
    want = b.diagnostics(max_lag=12, superchains=4)
    got = a.diagnostics(superchains=4)
    K = b.samples_device.shape[0]
    assert K >= 13 and (got.n_draws, got.n_chains, got.max_lag) == (K, 64, 12) == (want.n_draws, want.n_chains, want.max_lag)
    assert got.rhat.shape == (d,)
    check_fields(got, want)
    check_fields(got, ref.direct(b.samples.numpy().reshape(K, 64, d), 12, 4))
    with pytest.raises(ValueError, match='store_samples'):
        a.diagnostics(rank_normalized=True)
    with pytest.raises(ValueError, match='max_lag'):
        a.diagnostics(max_lag=13)


@pytest.mark.parametrize('strategy', ['mala', 'hmc'])
def test_cutting_the_launches_leaves_the_chain_alone(dev, strategy):
    """Nobody watches these runs, so without the option all 300 transitions are one launch and with it three (the ring has
    128 rows and wraps).  The chains and the counters are the same to the bit.  The pooled moments are summed per launch (fp32 over
    the transitions of a launch, fp64 from there on), so they agree to the rounding of a sum of 300 fp32 terms only:
    |difference of sum x| <= 300 x 2^-24 x sum |x|, i.e. 300 x 2^-24 x sqrt(E x^2) for the mean, and the same with x^2 for
    the second moment."""
    from nfmc_amd import sample
    from nfmc_amd.potentials import SumOfSquares
    from nfmc_amd.containers import RUNNING_STAGE_ROWS
    assert 2 * RUNNING_STAGE_ROWS < 300 <= hip.MAX_STEPS_PER_CALL      # three launches against one
    x0 = torch.randn(64, 5, generator=torch.Generator().manual_seed(3))

    def run(**params):
        return sample(SumOfSquares((5,)), strategy=strategy, x0=x0.clone(), n_iterations=300, seed=17, show_progress=False,
                      param_kwargs=params)

    a = run(store_samples=False, running_diagnostics=12)
    b = run(store_samples=True)
    c = run(store_samples=False)
    for other in (b, c):
        assert torch.equal(a.running_samples.last_sample, other.running_samples.last_sample)
        for name in a.statistics.COUNTERS + ('n_nonfinite_log_ratios',):
            assert getattr(a.statistics, name) == getattr(other.statistics, name), name
        bound = 300 * 2.0 ** -24
        m2 = other.second_moment.double()
        assert ((a.mean.double() - other.mean.double()).abs() <= bound * m2.sqrt() + 2.0 ** -24 * other.mean.abs()).all()
        assert ((a.second_moment.double() - m2).abs() <= (bound + 2.0 ** -24) * m2).all()
    assert a.running.n_seen == 300
    check_fields(a.diagnostics(superchains=4), b.diagnostics(max_lag=12, superchains=4))


def test_a_run_the_clock_ends_part_way_has_no_rhat(dev, monkeypatch):
    """The clock (patched: up at its third reading) ends a run of 200 planned transitions after two launches of 32.
    n_draws is 64, rhat is NaN, and every other field is the oracle's on the 64 states that the same run keeps."""
    from nfmc_amd import sample
    from nfmc_amd.potentials import Funnel
    from nfmc_amd.samplers import common
    x0 = torch.randn(64, 5, generator=torch.Generator().manual_seed(3))

    def run(**params):
        readings = []
        monkeypatch.setattr(common.Run, 'time_is_up', lambda self, t0, limit: readings.append(1) or len(readings) >= 3)
        return sample(Funnel((5,), 3.0), strategy='mala', x0=x0.clone(), n_iterations=200, seed=17, show_progress=False,
                      sampling_time_limit_seconds=1e9, param_kwargs=params)

    a = run(store_samples=False, running_diagnostics=12)
    b = run(store_samples=True)
    x = b.samples.numpy()
    assert x.shape == (64, 64, 5) and a.running.n_seen == 64 and a.running.planned == 200
    assert torch.equal(a.running_samples.last_sample, b.running_samples.last_sample)
    got = a.diagnostics(superchains=4)
    assert got.n_draws == 64 and torch.isnan(got.rhat).all() and not torch.isnan(got.ess).any()
    check_fields(got, ref.direct(x, 12, 4), nan_rhat=True)


def test_a_run_the_clock_ends_at_once_has_nothing_to_diagnose(dev):
    """n_draws is what the accumulator saw, not what was planned: fewer than 4 draws is the usual ValueError."""
    from nfmc_amd import sample
    from nfmc_amd.potentials import SumOfSquares
    out = sample(SumOfSquares((5,)), strategy='mala', n_chains=64, n_iterations=200, seed=17, show_progress=False,
                 sampling_time_limit_seconds=0.0, param_kwargs=dict(store_samples=False, running_diagnostics=4))
    assert out.running.n_seen == 0
    with pytest.raises(ValueError, match='at least 4'):
        out.diagnostics()


def test_report_worst_figures():
    """Last in the file: the worst figure of every kind over the cases above."""
    print('worst figures:', {k: '%.3g' % v for k, v in WORST.items()})
