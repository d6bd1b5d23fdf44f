"""GPU: the mclmc sampler (nfmc_mclmc_steps_f32, samplers.mcmc.MCLMC) against the fp64 reference of tests/mclmc_fp64.py.

Tolerances.  There is no accept decision, so every chain is compared.  A case's tolerance is 4 x the largest difference
between the reference run in torch fp32 and in fp64 on the CPU for the case's own inputs (`_figures`): the margin covers
the kernels' butterfly association and fused multiply-adds, which torch does not share.  Every case prints what it
measured (pytest -s); DESIGN.md 3.7 records the figures.
"""
import functools
import math

import pytest
import torch

import mclmc_fp64 as M
from mclmc_cases import MARGIN, N, SEED, T, _figures, compare, launch, starts, velocity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from nfmc_amd import hip
    return hip.require_gpu()


# ------------------------------------------------------------------------------------------------ 1. step by step
def _quadratic_case(d):
    from nfmc_amd.potentials import QuadraticPotential
    a = torch.linspace(0.3, 2.0, d, dtype=torch.float64)
    b = torch.linspace(-0.5, 0.5, d, dtype=torch.float64)
    imd = torch.linspace(0.5, 2.0, d, dtype=torch.float64).float()
    return QuadraticPotential((d,), a.float(), b.float()), M.quadratic(a.float().double(), b.float().double()), imd


TEST_1_DS = [2, 3, 5, 13, 24, 33, 100, 200, 300, 1000]


def test_1_the_dimensions_reach_all_nine_default_layouts():
    import ctypes as C
    from nfmc_amd import hip
    got = set()
    for d in TEST_1_DS:
        cpl, lpc = C.c_int32(0), C.c_int32(0)
        assert hip.lib().nfmc_sampler_layout(d, hip.POT_QUADRATIC, C.byref(cpl), C.byref(lpc)) == hip.OK
        got.add((cpl.value, lpc.value))
    assert got == {(4, 1), (4, 2), (4, 4), (4, 8), (8, 8), (8, 16), (8, 32), (8, 64), (16, 64)}


@pytest.mark.parametrize('d', TEST_1_DS)
def test_1_every_step_follows_the_fp64_reference_at_every_layout(dev, d):
    pot, target, imd = _quadratic_case(d)
    x0, u0 = starts(N, d, 100 + d), velocity(N, d)
    eps, L = 0.25 * math.sqrt(d) * 0.5, math.sqrt(d)
    r64, tol = _figures(target, x0, u0, eps, L, imd, T)
    compare(launch(dev, pot, x0, u0, T, eps, L, imd), r64, tol, 'quadratic d=%d' % d)


def test_1_funnel(dev):
    from nfmc_amd.potentials import Funnel
    d = 10
    x0, u0 = starts(N, d, 7), velocity(N, d)
    r64, tol = _figures(M.funnel(3.0), x0, u0, 0.3, 3.0, None, T)
    compare(launch(dev, Funnel((d,), 3.0), x0, u0, T, 0.3, 3.0), r64, tol, 'funnel d=10')


# ------------------------------------------------------------------------------------------------ 2. every kind
def _kind_mixture():
    import neutra_mh_cases as cases
    pot, ref = cases.Route('mixture', 'mixture', 5, 8, 10, 'auto', False, False).problem()
    return pot, ref, starts(N, 5, 3)


def _kind_logreg():
    from logreg_fp64 import LogRegU64, synthetic
    from nfmc_amd.potentials import BayesianLogisticRegression
    n_obs, d = 65, 5
    X, y, _ = synthetic(n_obs, d, 11, scale=2.0 / math.sqrt(n_obs))
    return BayesianLogisticRegression(X, y, 1.5), LogRegU64(X, y, 1.5), starts(N, d, 4, 0.7)


def _kind_sv():
    from nfmc_amd.potentials import StochasticVolatility
    from sv_fp64 import SVU64, start_states
    d = 5
    y, x0, _ = start_states(d - 3, N, 21, -1.0, 0.25, 0.95, 0.05)
    return StochasticVolatility(y), SVU64(y), x0.float()


def _kind_irt():
    from irt_fp64 import IRTFast64, start_states
    from nfmc_amd.potentials import ItemResponseTheory
    S, Q = 3, 2
    pot, truth = ItemResponseTheory.synthetic(S, Q, S + Q + 1, missing=0.25)
    ref = IRTFast64(pot.responses, pot.observed)
    return pot, ref, start_states(ref, truth, N, S + Q + 2).float()


def _kind_vfx():
    from nfmc_amd.potentials import VaryingEffectsRegression
    from varying_effects_fp64 import VFX64, start_states
    Cn = 2
    pot, truth = VaryingEffectsRegression.synthetic(Cn, 2 * Cn + 7, 1000 + Cn, intercepts='varying', slopes='varying', centered=True)
    ref = VFX64(x=pot.x, y=pot.y, group=pot.group, intercepts='varying', slopes='varying', noise_scale=pot.noise_scale,
                centered=True, location_scale=pot.location_scale, scale_scale=pot.scale_scale)
    return pot, ref, start_states(ref, truth, N, pot.event_size + 1).float()


def _kind_particles():
    from nfmc_amd.potentials import ParticleSystem
    from particles_fp64 import Particles64
    P, D = 4, 2
    pot = ParticleSystem(P, D, 'lennard_jones')
    return pot, Particles64(P, D, 'lennard_jones'), pot.start_states(N, P * D + 1, 0.03).float()


def _kind_lgm():
    from latent_gaussian_fp64 import PAIRS, make_pair, problem_data, starts as lgm_starts
    lik, par = PAIRS[2]
    data = problem_data(8, lik, 13 * 8)
    pot, ref = make_pair(data, par, None)
    return pot, ref, lgm_starts(data, ref, N, 61).float()


def _kind_gmrf():
    from gmrf_fp64 import COMBOS, make_pair, n_of, problem_data, starts as gmrf_starts
    lik, mode = COMBOS[3]
    data = problem_data(n_of(8, mode), lik, 13 * 8, None)
    pot, ref = make_pair(data, mode, None, False)
    return pot, ref, gmrf_starts(data, ref, N, 61).float()


def _from_cases(name):
    import neutra_mh_cases as cases
    pot, ref, x0, _ = cases.OWN_KINDS[name]()
    return pot, ref, x0


KINDS = {'mixture': _kind_mixture, 'logreg': _kind_logreg, 'sv': _kind_sv, 'irt': _kind_irt, 'vfx': _kind_vfx,
         'particles': _kind_particles, 'lgm': _kind_lgm, 'gmrf': _kind_gmrf,
         'fullrank': functools.partial(_from_cases, 'fullrank'), 'rosenbrock': functools.partial(_from_cases, 'rosenbrock'),
         'sparse_logreg': functools.partial(_from_cases, 'sparse_logreg'), 'phi4': functools.partial(_from_cases, 'phi4'),
         'diffusion': functools.partial(_from_cases, 'diffusion')}


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_2_every_kind_follows_its_fp64_restatement(dev, kind):
    pot, ref, x0 = KINDS[kind]()
    n, d = x0.shape
    u0 = velocity(n, d)
    # a step a tenth of blackjax's default start, scaled by the gradient the starts see: every kind takes every step
    g = M.value_and_grad(ref, x0.double())[1]
    eps = float(0.1 * math.sqrt(d) / max(1.0, float(g.norm(dim=1).median()) / math.sqrt(d)))
    r64, tol = _figures(ref, x0, u0, eps, math.sqrt(d), None, T)
    compare(launch(dev, pot, x0, u0, T, eps, math.sqrt(d)), r64, tol, '%s d=%d eps=%.3g' % (kind, d, eps))


# ------------------------------------------------------------------------------------------------ 3. launch seams
def test_3_two_calls_of_four_steps_are_one_call_of_eight(dev):
    d = 13
    pot, _, imd = _quadratic_case(d)
    x0, u0 = starts(N, d, 5), velocity(N, d)
    one = launch(dev, pot, x0, u0, 8, 0.6, 3.0, imd)
    a = launch(dev, pot, x0, u0, 4, 0.6, 3.0, imd)
    b = launch(dev, pot, a['x'], a['u'], 4, 0.6, 3.0, imd, step0=4)
    assert torch.equal(b['x'], one['x']) and torch.equal(b['u'], one['u'])
    assert torch.equal(torch.cat([a['kept'], b['kept']]), one['kept'])
    assert torch.equal(torch.cat([a['de'], b['de']]), one['de'])
    again = launch(dev, pot, x0, u0, 8, 0.6, 3.0, imd)
    assert all(torch.equal(again[k], one[k]) for k in ('x', 'u', 'kept', 'de'))


def test_3_a_shard_of_the_chains_is_the_same_rows(dev):
    """chains are independent and Philox is keyed by the global chain id: rows 40 .. 95 alone, bitwise"""
    d = 13
    pot, _, imd = _quadratic_case(d)
    x0, u0 = starts(N, d, 5), velocity(N, d)
    one = launch(dev, pot, x0, u0, 8, 0.6, 3.0, imd)
    part = launch(dev, pot, x0[40:], u0[40:], 8, 0.6, 3.0, imd, chain_offset=40)
    assert torch.equal(part['x'], one['x'][40:]) and torch.equal(part['u'], one['u'][40:])
    assert torch.equal(part['de'], one['de'][:, 40:]) and torch.equal(part['kept'], one['kept'][:, 40:])


def test_3_one_chain_runs(dev):
    pot, target, imd = _quadratic_case(5)
    x0, u0 = starts(1, 5, 5), velocity(1, 5)
    r64, tol = _figures(target, x0, u0, 0.4, 2.0, imd, T)
    compare(launch(dev, pot, x0, u0, T, 0.4, 2.0, imd), r64, tol, 'one chain')


def test_3_a_zero_gradient_moves_along_the_velocity(dev):
    from nfmc_amd.potentials import SumOfSquares
    d, eps = 6, 0.25
    u0 = velocity(N, d)
    run = launch(dev, SumOfSquares((d,)), torch.zeros(N, d), u0, 1, eps, 1e6)
    assert torch.isfinite(run['x']).all() and torch.isfinite(run['u']).all() and torch.isfinite(run['de']).all()
    assert torch.allclose(run['x'].cpu(), eps * u0, rtol=0, atol=1e-7)
    # dK_1 = 0, so dE = U(x') + dK_2 with the second kick from the gradient at x' = eps u: the reference's figure
    r64, tol = _figures(M.quadratic(1.0, 0.0), torch.zeros(N, d), u0, eps, 1e6, None, 1)
    compare(run, r64, tol, 'zero gradient')
    u1, dk1 = M.kick(u0.double(), torch.zeros(N, d, dtype=torch.float64), torch.ones(1, d, dtype=torch.float64), eps / 2, d)
    assert torch.equal(dk1, torch.zeros(N, dtype=torch.float64)) and torch.equal(u1, u0.double())


# ------------------------------------------------------------------------------------------------ 4. store
def test_4_the_thinned_bounded_store_holds_rows_of_the_dense_run(dev):
    from nfmc_amd.containers import DeviceSampleStore
    d, steps = 13, 11
    pot, _, imd = _quadratic_case(d)
    x0, u0 = starts(N, d, 5), velocity(N, d)
    dense = launch(dev, pot, x0, u0, steps, 0.6, 3.0, imd)
    store = DeviceSampleStore(N, d, dev, steps, 3, 2)
    a = launch(dev, pot, x0, u0, 5, 0.6, 3.0, imd, store=store)
    launch(dev, pot, a['x'], a['u'], steps - 5, 0.6, 3.0, imd, store=store, step0=5)
    kept_steps = [s for s in range(steps) if s % 3 == 0][-2:]          # thinning 3, the newest two
    got = store.ordered()
    assert tuple(got.shape) == (2, N, d) and kept_steps == [6, 9]
    assert torch.equal(got, dense['kept'][kept_steps])


# ------------------------------------------------------------------------------------------------ 5. non-finite steps
def test_5_a_step_that_overflows_is_not_taken(dev):
    from nfmc_amd import hip
    from nfmc_amd.potentials import Funnel
    d, eps, L = 10, 2.0, 3.0
    x0, u0 = starts(N, d, 7), velocity(N, d)
    bad = [3, 40, 95]
    x0[bad, 0] = -60.0
    r32 = M.steps(M.funnel(3.0), x0, u0, eps, L, None, SEED, 0, 1, torch.float32)
    r64 = M.steps(M.funnel(3.0), x0.double(), u0.double(), eps, L, None, SEED, 0, 1, torch.float64)
    assert (~r32[3][0]).nonzero().flatten().tolist() == bad, 'the inputs overflow fp32 there and only there'
    stats = hip.DeviceStats(d, dev)
    run = launch(dev, Funnel((d,), 3.0), x0, u0, 1, eps, L, stats=stats)
    x1, u1 = run['x'].cpu(), run['u'].cpu()
    assert torch.equal(x1[bad], x0[bad])
    assert int(stats.counters[hip.CNT_NONFINITE]) == len(bad) and int(stats.counters[hip.CNT_ATTEMPTED]) == N
    assert int(stats.counters[hip.CNT_ACCEPTED]) == N
    assert float((u1[bad] - u0[bad]).abs().max()) > 1e-3 and torch.allclose(u1.norm(dim=1), torch.ones(N), atol=1e-5)
    assert not torch.isfinite(run['de'].cpu()[0, bad]).any()
    # the velocity of a chain that stayed: O from the old velocity
    nu = math.sqrt(math.expm1(2.0 * eps / L) / d)
    from oracle import samplers as osamp
    z = osamp.PhiloxNoise(SEED, dtype=torch.float64).normal(N, (d,), 0, 0)
    w = u0.double() + nu * z
    assert torch.allclose(u1[bad].double(), (w / w.norm(dim=1, keepdim=True))[bad], atol=1e-5)
    good = [i for i in range(N) if i not in bad]
    fig = MARGIN * float((r32[0][0][good].double() - r64[0][0][good]).abs().max())
    got = float((x1[good].double() - r64[0][0][good]).abs().max())
    print('non-finite case: the other chains differ by %.3g (tol %.3g)' % (got, fig))
    assert got <= fig


# ------------------------------------------------------------------------------------------------ 6. statistics
def test_6_the_moments_and_the_energy_sums_are_those_of_the_run(dev):
    from nfmc_amd import hip
    d, steps = 13, 16
    pot, _, imd = _quadratic_case(d)
    x0, u0 = starts(N, d, 5), velocity(N, d)
    stats = hip.DeviceStats(d, dev)
    esums = torch.zeros(3, dtype=torch.float64, device=dev)
    run = launch(dev, pot, x0, u0, steps, 0.6, 3.0, imd, stats=stats, esums=esums)
    kept, de = run['kept'].cpu().double(), run['de'].cpu().double()
    sx, sx2, cnt, _ = stats.host_totals()
    m = N * steps
    # the tolerance tests/test_gpu_parity.py holds uhmc's moments to
    assert torch.allclose(sx / m, kept.mean((0, 1)), rtol=1e-5, atol=1e-6)
    assert torch.allclose(sx2 / m, (kept ** 2).mean((0, 1)), rtol=1e-5, atol=1e-6)
    assert int(cnt[hip.CNT_ATTEMPTED]) == m == int(cnt[hip.CNT_ACCEPTED]) and int(cnt[hip.CNT_NONFINITE]) == 0
    want = torch.stack([(de ** 2).sum(), de.sum(), torch.tensor(float(m), dtype=torch.float64)])
    # fp64 sums of fp32 values in another order
    assert torch.allclose(esums.cpu(), want, rtol=1e-12, atol=1e-12 * float(de.abs().sum())), (esums.cpu(), want)


def test_6_sample_reports_the_moments_of_its_kept_states(dev):
    from nfmc_amd import sample
    d = 13
    pot, _, imd = _quadratic_case(d)
    out = sample(pot, strategy='mclmc', flow=None, n_iterations=16, x0=starts(N, d, 5), seed=SEED, show_progress=False,
                 kernel_kwargs={'inv_mass_diag': imd, 'step_size': 0.6, 'decoherence_length': 3.0})
    kept = out.samples.double()
    assert kept.shape == (16, N, d)
    assert torch.allclose(out.mean.double().cpu(), kept.mean((0, 1)), rtol=1e-5, atol=1e-6)
    assert torch.allclose(out.variance.double().cpu(), (kept ** 2).mean((0, 1)) - kept.mean((0, 1)) ** 2, rtol=1e-4, atol=1e-5)
    assert out.statistics.n_target_calls == 16 * N == out.statistics.n_target_gradient_calls
    assert out.kernel.energy_variance > 0


# ------------------------------------------------------------------------------------------------ 7. controller
def test_7_every_device_update_is_the_replay_of_its_own_records(dev):
    from nfmc_amd import hip
    from nfmc_amd.samplers import mcmc
    d, every, updates = 13, 8, 3
    pot, _, imd0 = _quadratic_case(d)
    x0 = starts(N, d, 5)
    s = mcmc.MCLMC((d,), pot, mcmc.MCLMCKernel(d, step_size=0.6, decoherence_length=2.0, inv_mass_diag=imd0),
                   mcmc.MCLMCParameters(n_iterations=every * updates, tune_every=every, tune_inv_mass_diag=True, tuning=True))
    s.seed, s.shard, s.fuse, s.replay = SEED, None, 'auto', None
    from nfmc_amd.samplers.common import Run
    run = Run(s, x0)
    tune = mcmc.MclmcTuning(s, run, updates)
    stats = hip.DeviceStats(d, dev)
    x, u = x0, velocity(N, d, SEED, hip.WARMUP_STEP0)
    eps, L, imd = 0.6, 2.0, imd0.clone()
    kw = dict(target=5e-4, imd_adjustment=0.25, decoherence_factor=1.0, tune_inv_mass_diag=True)
    for j in range(updates):
        r = launch(dev, pot, x, u, every, eps, L, tune=tune, stats=stats, step0=hip.WARMUP_STEP0 + j * every)
        c64 = M.replay_update(r['de'].cpu(), r['kept'].cpu(), eps, L, imd, torch.float64, **kw)
        c32 = M.replay_update(r['de'].cpu(), r['kept'].cpu(), eps, L, imd, torch.float32, **kw)
        st = tune.state.cpu()
        got = (float(st[hip.MCLMC_STEP_SIZE]), float(st[hip.MCLMC_DECOHERENCE_LENGTH]), tune.imd.cpu().double())
        want = (c64.step_size, c64.decoherence_length, c64.inv_mass_diag.double())
        spread = (abs(c32.step_size - c64.step_size), abs(c32.decoherence_length - c64.decoherence_length),
                  float((c32.inv_mass_diag.double() - want[2]).abs().max()))
        # 4 x the replay's own fp32-against-fp64 difference, and never under an fp32 ulp of the value (the scales are fp32 words)
        tol = [MARGIN * sp + 2.0 ** -23 * abs(w) for sp, w in zip(spread, (want[0], want[1], float(want[2].abs().max())))]
        diff = (abs(got[0] - want[0]), abs(got[1] - want[1]), float((got[2] - want[2]).abs().max()))
        print('update %d: eps %.6g (diff %.3g tol %.3g)  L %.6g (diff %.3g tol %.3g)  scales diff %.3g tol %.3g  V %.3g'
              % (j, got[0], diff[0], tol[0], got[1], diff[1], tol[1], diff[2], tol[2], float(st[hip.MCLMC_ENERGY_VARIANCE])))
        assert all(dd <= tt for dd, tt in zip(diff, tol)), (j, diff, tol)
        assert float(st[hip.MCLMC_COUNT]) == N * every
        x, u, eps, L, imd = r['x'], r['u'], got[0], got[1], tune.imd.cpu().clone()
    tune.download(s.kernel)
    st = tune.state.cpu()
    assert s.kernel.step_size == float(st[hip.MCLMC_STEP_SIZE]) and s.kernel.decoherence_length == float(st[hip.MCLMC_DECOHERENCE_LENGTH])
    h = s.kernel.adaptation_history
    assert h.shape == (updates, hip.MCLMC_ROW_WORDS)
    assert float(h[0, hip.MCLMC_ROW_STEP_SIZE]) == 0.6 and float(h[-1, hip.MCLMC_ROW_NEXT_STEP_SIZE]) == s.kernel.step_size
    assert torch.equal(h[1:, hip.MCLMC_ROW_STEP_SIZE], h[:-1, hip.MCLMC_ROW_NEXT_STEP_SIZE])
    assert s.kernel.energy_variance == float(h[-1, hip.MCLMC_ROW_ENERGY_VARIANCE])


def test_7_one_call_enqueues_every_update(dev):
    """a whole warmup in one call (NfmcMclmcTune.every) leaves the words of one call per update"""
    from nfmc_amd import hip
    from nfmc_amd.samplers import mcmc
    from nfmc_amd.samplers.common import Run
    d, every, updates = 13, 8, 3
    pot, _, imd0 = _quadratic_case(d)
    x0 = starts(N, d, 5)
    words = []
    for whole in (True, False):
        s = mcmc.MCLMC((d,), pot, mcmc.MCLMCKernel(d, step_size=0.05, decoherence_length=2.0, inv_mass_diag=imd0),
                       mcmc.MCLMCParameters(n_iterations=every * updates, tune_every=every, tune_inv_mass_diag=True, tuning=True))
        s.seed, s.shard, s.fuse, s.replay = SEED, None, 'auto', None
        tune = mcmc.MclmcTuning(s, Run(s, x0), updates)
        stats = hip.DeviceStats(d, dev)
        x, u = x0, velocity(N, d)
        for j in range(1 if whole else updates):
            k = every * updates if whole else every
            r = launch(dev, pot, x, u, k, 0.05, 2.0, tune=tune, stats=stats, step0=j * every)
            x, u = r['x'], r['u']
        words.append((tune.state.cpu()[:hip.MCLMC_WORDS].clone(), tune.imd.cpu().clone(), x.cpu().clone()))
    assert all(torch.equal(a, b) for a, b in zip(*words))


def test_7_the_two_level_fold_leaves_what_the_one_level_fold_leaves(dev, monkeypatch):
    """Above 256 workgroup tiles a tuning launch runs on the full grid and its slabs are folded in two levels: 20000
    chains at d = 13 (layout (4, 4), 64 chains per workgroup) are 313 tiles.  NFMC_TUNE_ONE_LEVEL=1, read per call, holds
    the same call to 256 workgroups and one fold.  A chain's arithmetic does not depend on the grid, so its outputs are the
    same bits; the two folds add the same 160 000 fp64 addends per column in another order, at most 160 000 x 2^-53 ~ 2e-11
    relative apart, held to 1e-9; the scales are those fp64 values rounded to fp32: one ulp."""
    from nfmc_amd import hip
    from nfmc_amd.samplers import mcmc
    from nfmc_amd.samplers.common import Run
    d, n, every = 13, 20000, 8
    pot, _, imd0 = _quadratic_case(d)
    x0, u0 = starts(n, d, 5), velocity(n, d)
    monkeypatch.delenv('NFMC_TUNE_ONE_LEVEL', raising=False)
    runs = []
    for one_level in (False, True):
        if one_level:
            monkeypatch.setenv('NFMC_TUNE_ONE_LEVEL', '1')
        s = mcmc.MCLMC((d,), pot, mcmc.MCLMCKernel(d, step_size=0.6, decoherence_length=2.0, inv_mass_diag=imd0),
                       mcmc.MCLMCParameters(n_iterations=every, tune_every=every, tune_inv_mass_diag=True, tuning=True))
        s.seed, s.shard, s.fuse, s.replay = SEED, None, 'auto', None
        tune = mcmc.MclmcTuning(s, Run(s, x0), 1)
        stats = hip.DeviceStats(d, dev)
        esums = torch.zeros(3, dtype=torch.float64, device=dev)
        r = launch(dev, pot, x0, u0, every, 0.6, 2.0, tune=tune, stats=stats, esums=esums, dense=False)
        runs.append((r, tune.state.cpu()[:hip.MCLMC_WORDS].clone(), tune.imd.cpu().clone(), stats.host_totals()[2].clone(),
                     esums.cpu().clone()))
    (ra, sa, ia, ca, ea), (rb, sb, ib, cb, eb) = runs
    assert all(torch.equal(ra[k], rb[k]) for k in ('x', 'u', 'de'))
    assert torch.equal(ca, cb) and int(ca[hip.CNT_ATTEMPTED]) == n * every
    assert float(sa[hip.MCLMC_COUNT]) == float(sb[hip.MCLMC_COUNT]) == n * every
    assert float(sa[hip.MCLMC_HISTORY_USED]) == 1 == float(sb[hip.MCLMC_HISTORY_USED])
    words = [hip.MCLMC_STEP_SIZE, hip.MCLMC_DECOHERENCE_LENGTH, hip.MCLMC_ENERGY_VARIANCE]
    rel = float(((sa[words] - sb[words]).abs() / sb[words].abs()).max())
    rel_e = float(((ea - eb).abs() / eb.abs()).max())
    ulp = 2.0 ** (torch.floor(torch.log2(torch.minimum(ia, ib).abs().double())) - 23)   # of the smaller: the finer spacing
    ulps = float(((ia.double() - ib.double()).abs() / ulp).max())
    print('two-level against one-level fold: eps, L, V differ by %.3g relative, the energy sums by %.3g, the scales by %.3g ulp'
          % (rel, rel_e, ulps))
    assert rel <= 1e-9 and rel_e <= 1e-9
    assert ulps <= 1.0

def test_8_the_warmup_finds_the_step_size_of_the_reference_on_a_standard_gaussian(dev):
    from nfmc_amd import hip, sample
    from nfmc_amd.potentials import DiagonalGaussian
    d, n, W, every = 16, 1024, 80, 8
    x0 = starts(n, d, 8)
    pot = DiagonalGaussian((d,), 0.0, 1.0)
    out = sample(pot, strategy='mclmc', flow=None, n_iterations=8, n_warmup_iterations=W, x0=x0, seed=SEED, warmup=True,
                 show_progress=False, kernel_kwargs={'step_size': 0.01}, param_kwargs={'tune_every': every})
    k = out.kernel
    target = M.quadratic(0.5, 0.0)
    c64 = M.free_run(target, x0.double(), 0.01, math.sqrt(d), None, SEED, hip.WARMUP_STEP0, W, every, torch.float64)[0]
    c32 = M.free_run(target, x0, 0.01, math.sqrt(d), None, SEED, hip.WARMUP_STEP0, W, every, torch.float32)[0]
    hist = k.adaptation_history
    spread = abs(c32.step_size - c64.step_size)
    print('standard Gaussian d=16: eps %.6g, reference %.6g (fp32 %.6g, spread %.3g); eps / sqrt(d) = %.3f; last V %.3g; L %.4g'
          % (k.step_size, c64.step_size, c32.step_size, spread, k.step_size / math.sqrt(d),
             float(hist[-1, hip.MCLMC_ROW_ENERGY_VARIANCE]), k.decoherence_length))
    assert hist.shape[0] == W // every
    assert abs(k.step_size - c64.step_size) <= MARGIN * spread
    assert 5e-4 / 2 <= float(hist[-1, hip.MCLMC_ROW_ENERGY_VARIANCE]) <= 2 * 5e-4
    assert torch.isfinite(out.mean).all()


def test_9_the_tuned_sampler_recovers_the_variances_of_a_badly_scaled_gaussian(dev):
    from nfmc_amd import sample
    from nfmc_amd.potentials import DiagonalGaussian
    d, n = 64, 1024
    sig = torch.logspace(-1, 1, d, dtype=torch.float64)
    x0 = (torch.randn(n, d, generator=torch.Generator().manual_seed(9), dtype=torch.float64) * sig).float()
    out = sample(DiagonalGaussian((d,), 0.0, sig.float()), strategy='mclmc', flow=None, n_iterations=400, n_warmup_iterations=640,
                 x0=x0, seed=SEED, warmup=True, show_progress=False, kernel_kwargs={'step_size': 0.1},
                 param_kwargs={'tune_inv_mass_diag': True, 'store_samples': False})
    ratio = out.variance.double().cpu() / sig ** 2
    k = out.kernel
    print('diagonal Gaussian d=64: eps %.4g  L %.4g  s/sigma^2 in [%.3f, %.3f]  variance ratio in [%.3f, %.3f]  V %.3g'
          % (k.step_size, k.decoherence_length, float((k.inv_mass_diag.double() / sig ** 2).min()),
             float((k.inv_mass_diag.double() / sig ** 2).max()), float(ratio.min()), float(ratio.max()), k.energy_variance))
    assert 0.95 <= float(ratio.min()) and float(ratio.max()) <= 1.12


# ------------------------------------------------------------------------------------------------ 10. torch path
def test_10_a_callable_with_no_closed_form_runs_the_same_step(dev):
    from nfmc_amd import sample
    d, steps = 5, 4
    pot, target, imd = _quadratic_case(d)
    x0 = starts(N, d, 5)
    kw = dict(strategy='mclmc', flow=None, n_iterations=steps, x0=x0, seed=SEED, show_progress=False,
              kernel_kwargs={'inv_mass_diag': imd, 'step_size': 0.4, 'decoherence_length': 2.0})
    fused = sample(pot, **kw)
    a, b = pot.a.to(dev), pot.b.to(dev)
    split = sample(lambda x: (a * (x - b) ** 2).sum(-1), event_shape=(d,), fuse='never', **kw)
    u0 = velocity(N, d)
    _, tol = _figures(target, x0, u0, 0.4, 2.0, imd, steps)
    diff = float((fused.samples.double() - split.samples.double()).abs().max())
    print('torch path against the fused run: %.3g (tol %.3g)' % (diff, tol['x']))
    assert diff <= tol['x']
    assert split.statistics.n_target_calls == steps * N


def test_10_the_host_controller_of_the_torch_path_tunes_like_the_device(dev):
    """A warmup of two updates on either path.  Both run the same recurrence on steps that differ by fp32 rounding (test
    10: states to 3e-7, dE to ~1e-5 on |dE| ~ 1e-2, so V to under 1e-3 relative before averaging over 768 steps): log eps
    moves by a sixth of log V and L by half the relative change of the variances, hence 1e-3 relative on both."""
    from nfmc_amd import create_sampler
    d = 5
    pot, _, imd = _quadratic_case(d)
    x0 = starts(N, d, 5)
    a, b = pot.a.to(dev), pot.b.to(dev)
    got = []
    for target, fuse in ((pot, 'auto'), (lambda x: (a * (x - b) ** 2).sum(-1), 'never')):
        s = create_sampler(target, event_shape=(d,), strategy='mclmc', flow=None,
                           kernel_kwargs={'inv_mass_diag': imd, 'step_size': 0.5, 'decoherence_length': 2.0},
                           param_kwargs={'n_iterations': 4, 'n_warmup_iterations': 16, 'tune_inv_mass_diag': True})
        s.seed, s.fuse = SEED, fuse
        s.warmup(x0, show_progress=False)
        k = s.kernel
        assert k.adaptation_history.shape == (2, 6) and s._next_velocity is not None
        got.append((k.step_size, k.decoherence_length, k.inv_mass_diag.double().cpu(), k.energy_variance))
    print('warmup, fused / torch path: eps %.6g / %.6g  L %.6g / %.6g  V %.4g / %.4g'
          % (got[0][0], got[1][0], got[0][1], got[1][1], got[0][3], got[1][3]))
    assert got[0][0] == pytest.approx(got[1][0], rel=1e-3) and got[0][1] == pytest.approx(got[1][1], rel=1e-3)
    assert torch.allclose(got[0][2], got[1][2], rtol=1e-3, atol=0)


def test_10_what_the_sampler_refuses(dev):
    from nfmc_amd import create_sampler
    from nfmc_amd.potentials import SumOfSquares

    class TwoRanks:
        world, rank = 2, 0

        def bounds(self, n):
            return 0, n // 2

        def broadcast_int(self, v):
            return v

    def sampler(**params):
        s = create_sampler(SumOfSquares((6,)), strategy='mclmc', flow=None, param_kwargs={'n_iterations': 8, **params})
        s.seed = SEED
        return s

    s = sampler()
    s.shard = TwoRanks()
    with pytest.raises(ValueError, match='sharded warmup'):
        s.warmup(starts(N, 6, 5), show_progress=False)
    s = sampler()
    s.rng_rounds = 7
    with pytest.raises(ValueError, match='rng_rounds=7'):
        s.sample(starts(N, 6, 5), show_progress=False)
    with pytest.raises(ValueError, match='tune_every'):
        sampler(tune_every=513).warmup(starts(N, 6, 5), show_progress=False)


# ------------------------------------------------------------------------------------------------ 11. diagnostics
def test_11_the_diagnostics_read_an_mclmc_run(dev):
    from nfmc_amd import sample
    d = 6
    pot, _, imd = _quadratic_case(d)
    kw = dict(strategy='mclmc', flow=None, n_iterations=32, x0=starts(64, d, 5), seed=SEED, show_progress=False)
    diag = sample(pot, **kw).diagnostics()
    running = sample(pot, param_kwargs={'store_samples': False, 'running_diagnostics': True}, **kw).diagnostics()
    for dg in (diag, running):
        for name in ('rhat', 'ess'):
            v = getattr(dg, name)
            assert tuple(v.shape) == (d,) and torch.isfinite(v).all(), name
