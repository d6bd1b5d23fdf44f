"""The trajectory-length adaptation of the device warmup (NfmcTune.trajectory: ChEES-HMC about the lagged centre) against
tests/chees_fp64.py.

  every update     from the kernel's own previous state (tuning state and mass diagonal copied before each launch, kept
                   states): leapfrog totals as integers; g-hat and sum(alpha) within
                       8 * max(|fp32 restatement - fp64|, 2^-22 * magnitude of the terms)
                   (8: the harness's KAPPA; 2^-22: four fp32 ulps of the terms); log T, v and log T-bar within what that
                   tolerance of g-hat moves the replayed controller, plus 1e-12; and to 1e-12 when the replayed controller is
                   fed the kernel's own g-hat
  transitions      each shadowed in fp64 (oracle/shadow.py) with its own leapfrog count: one shadow call per transition,
                   every check of the report per call, and the near-tie share -- the part of the chains the oracle cannot
                   decide -- over the transitions of the run, as the warmup tests take it (one transition of 150 chains
                   passes 1 % with one near tie and misses it with two)
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import chees_fp64 as CH
import target_harness as H
from test_gpu_warmup import _target

pytestmark = pytest.mark.gpu

ULP4 = 2.0 ** -22


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


class Shadows:
    """One oracle.shadow call per transition, each with its own leapfrog count; the near ties are counted over the run."""

    def __init__(self, target, seed, max_tie_share):
        self.target, self.seed, self.max_tie_share = target, seed, max_tie_share
        self.ties = self.decisions = 0

    def transition(self, pre, post, h, imd, step, L, what):
        from oracle import shadow as oshadow
        wl = oshadow.Workload('hmc', self.target, step_size=h, n_leapfrog=L, inv_mass_diag=imd, step0=step)
        rep = oshadow.shadow(torch.stack([pre, post]), wl, self.seed)
        fails = rep.failures(H.KAPPA, max_tie_share=1.0)
        assert not fails, (what, fails, rep.summary())
        self.ties += rep.n_ties
        self.decisions += rep.n_chains * rep.n_transitions

    def check(self, what):
        assert self.decisions > 0 and self.ties <= self.max_tie_share * self.decisions, (what, self.ties, self.decisions)


def _sampler(d, pot, W, T, h, every=1, L=4, **params):
    s = H.warmup_sampler('hmc', d, pot, W, T, h, L=L, every=every)
    s.params.tune_trajectory_length = True
    for k, v in params.items():
        setattr(s.params, k, v)
    return s


def _words(state, d):
    """(step size, centre, trajectory block, controller row) of a tuning state on the host."""
    from nfmc_amd import hip
    off = int(hip.lib().nfmc_tune_state_doubles(d))
    c0 = hip.tune_shift_offset(d)
    tr = state[off:]
    row = dict(log_length=float(tr[hip.TRAJ_LOG_LENGTH]), log_averaged=float(tr[hip.TRAJ_LOG_AVERAGED]),
               v=float(tr[hip.TRAJ_V]), count=int(round(float(tr[hip.TRAJ_COUNT]))))
    return float(state[hip.TUNE_STEP_SIZE]), state[c0:c0 + d].clone(), tr, row


def _check_updates(s, snaps, x0, states, target, d, seed, every, what, ties, shadow=True):
    """Every controller update of the warmup from the state the kernel started it from.  Returns the worst ratios of
    the g-hat and sum(alpha) errors to their tolerances."""
    from nfmc_amd import hip
    launches, final = snaps.rows()
    n = x0.shape[0]
    worst_g = worst_a = 0.0
    shadows = Shadows(target, seed, ties)
    hist = s.kernel.trajectory_history
    assert hist.shape == (len(launches), hip.TRAJ_ROW_WORDS), (what, hist.shape)
    done = 0
    for u, (st, imd, k0, k) in enumerate(launches):
        after = launches[u + 1][0] if u + 1 < len(launches) else final[0]
        h, c, tr, row = _words(st, d)
        h_next, _c, tr_after, row_after = _words(after, d)
        T = float(tr[hip.TRAJ_LENGTH])
        lmax = int(tr[hip.TRAJ_MAX_LEAPFROG])
        assert k0 == hip.WARMUP_STEP0 + done and k == min(every, states.shape[0] - done), (what, u, k0, k)
        pre = x0 if done == 0 else states[done - 1]
        kw = dict(h_next=h_next, max_leapfrog_steps=lmax)
        rep = CH.replay_update(row, states[done:done + k], pre, c, h, T, k0, k, target, imd, seed, **kw)
        tag = '%s update %d' % (what, u)
        # leapfrog totals, as integers
        total = int(round(float(tr_after[hip.TRAJ_LEAPFROG_TOTAL] - tr[hip.TRAJ_LEAPFROG_TOTAL])))
        assert total == sum(rep.leapfrogs) == int(round(float(hist[u, hip.TRAJ_ROW_LEAPFROGS]))), (tag, total, rep.leapfrogs)
        # the pooled sums
        g_k, a_k = float(tr_after[hip.TRAJ_G_HAT]), float(tr_after[hip.TRAJ_ALPHA_SUM])
        tol_g = H.KAPPA * max(abs(rep.g_hat32 - rep.g_hat), ULP4 * rep.magnitude)
        tol_a = H.KAPPA * max(abs(rep.alpha_sum32 - rep.alpha_sum), ULP4 * rep.alpha_sum)
        assert math.isfinite(g_k) and rep.alpha_sum > 0, tag
        worst_g = max(worst_g, abs(g_k - rep.g_hat) / tol_g)
        worst_a = max(worst_a, abs(a_k - rep.alpha_sum) / tol_a)
        assert abs(g_k - rep.g_hat) <= tol_g, (tag, g_k, rep.g_hat, rep.g_hat32, rep.magnitude)
        assert abs(a_k - rep.alpha_sum) <= tol_a, (tag, a_k, rep.alpha_sum, rep.alpha_sum32)
        # the controller: within what g-hat's tolerance moves the replay ...
        lo = CH.replay_update(row, states[done:done + k], pre, c, h, T, k0, k, target, imd, seed, g_shift=-tol_g, **kw)
        hi = CH.replay_update(row, states[done:done + k], pre, c, h, T, k0, k, target, imd, seed, g_shift=tol_g, **kw)
        for name in ('log_length', 'v', 'log_averaged'):
            want = getattr(rep.controller, name)
            slack = max(abs(getattr(lo.controller, name) - want), abs(getattr(hi.controller, name) - want)) + 1e-12
            assert abs(row_after[name] - want) <= slack, (tag, name, row_after[name], want, slack)
        # ... and exactly the recurrence, fed the kernel's own sums
        own = CH.controller_from(row, s.params.trajectory_adaptation, lmax)
        own.step(g_k, a_k, h_next)
        assert row_after['count'] == own.count == row['count'] + 1, tag
        for name in ('log_length', 'v', 'log_averaged'):
            np.testing.assert_allclose(row_after[name], getattr(own, name), rtol=1e-12, atol=1e-12, err_msg=tag + ' ' + name)
        np.testing.assert_allclose(float(tr_after[hip.TRAJ_LENGTH]), math.exp(row_after['log_length']), rtol=1e-14)
        # the history row is what the block held
        want_row = [T, h, g_k, a_k, total, row_after['log_length'], row_after['v'], row_after['log_averaged'], h_next]
        assert hist[u].tolist() == want_row, (tag, hist[u].tolist(), want_row)
        if shadow:
            for j, L in enumerate(rep.leapfrogs):
                t = done + j
                shadows.transition(x0 if t == 0 else states[t - 1], states[t], h, imd.clone(), k0 + j, L,
                                   '%s transition %d (L = %d)' % (tag, t, L))
        done += k
    assert done == states.shape[0]
    if shadow:
        shadows.check(what)
    return worst_g, worst_a


# (target, d, n, every): one lane per chain; padded coordinates and chains far from the origin; pooled updates with a short
# last pool; funnel; staged-LDS target; neighbour exchange; the (8, 8) layout; d = 130; more than 256 chain tiles
CASES = [
    ('sumsq', 1, 300, 1),
    ('offset', 3, 257, 1),
    ('offset', 8, 129, 3),
    ('funnel', 25, 200, 1),
    ('logreg', 8, 150, 2),
    ('rosenbrock', 8, 140, 1),
    ('offset', 64, 96, 1),
    ('offset', 130, 70, 1),
    ('sumsq', 8, 128 * 257, 1),
]
UPDATES = 12


@pytest.mark.parametrize('tname,d,n,every', CASES)
def test_every_update_one_step_ahead(dev, monkeypatch, tname, d, n, every):
    pot, target, draw = _target(tname, d, seed=d)
    x0 = draw(n).float()
    h0 = 0.1 * d ** (-1 / 3) * (0.3 if tname in ('funnel', 'rosenbrock', 'logreg') else 1.0)
    W = UPDATES * every - (1 if every > 1 else 0)           # every > 1: the last pool is one transition short
    s = _sampler(d, pot, W, 6, h0, every=every)
    s.seed = 4242 + d
    snaps = CH.Snapshots(monkeypatch, s, every)
    wout = s.warmup(x0, show_progress=False)
    states = wout.samples.reshape(W, n, d)
    assert torch.isfinite(states).all()
    what = 'hmc %s d=%d n=%d every=%d' % (tname, d, n, every)
    ties = 0.05 if tname == 'rosenbrock' else 0.01
    worst_g, worst_a = _check_updates(s, snaps, x0, states, target, d, s.seed, every, what, ties)
    print('%s: worst |g-hat error| / tolerance %.3f, worst |sum(alpha) error| / tolerance %.3f' % (what, worst_g, worst_a))
    assert s.kernel.trajectory_length == math.exp(float(s.kernel.trajectory_history[-1, 7]))


def test_non_finite_chains_drop_out(dev, monkeypatch):
    from nfmc_amd import hip
    tname, d, n = 'funnel', 8, 130
    pot, target, draw = _target(tname, d, seed=d)
    x0 = draw(n).float()
    x0[[3, 64, 129], 0] = -800.0                            # exp(-x_0) overflows: U, the gradient and the log ratio
    s = _sampler(d, pot, UPDATES, 6, 0.03 * d ** (-1 / 3))
    s.seed = 77
    snaps = CH.Snapshots(monkeypatch, s, 1)
    wout = s.warmup(x0, show_progress=False)
    states = wout.samples.reshape(UPDATES, n, d)
    assert (states[:, [3, 64, 129], 0] == -800.0).all()     # never accepted
    hist = s.kernel.trajectory_history
    assert torch.isfinite(hist).all() and math.isfinite(s.kernel.trajectory_length), hist
    assert (hist[:, hip.TRAJ_ROW_ALPHA_SUM] <= n - 3).all() and (hist[:, hip.TRAJ_ROW_ALPHA_SUM] > 0).all()
    worst_g, worst_a = _check_updates(s, snaps, x0, states, target, d, s.seed, 1, 'non-finite chains', 0.01, shadow=False)
    print('non-finite chains: worst ratios %.3f (g-hat) %.3f (sum alpha)' % (worst_g, worst_a))


def test_hand_off_to_sampling(dev):
    from nfmc_amd import hip
    from nfmc_amd.tuning import leapfrog_count
    tname, d, n, T = 'offset', 8, 140, 6
    pot, target, draw = _target(tname, d, seed=d)
    x0 = draw(n).float()
    s = _sampler(d, pot, UPDATES, T, 0.1 * d ** (-1 / 3))
    s.seed = 99
    wout = s.warmup(x0, show_progress=False)
    hist = s.kernel.trajectory_history
    assert hist.shape[0] == UPDATES
    Tbar = s.kernel.trajectory_length
    assert Tbar == math.exp(float(hist[-1, hip.TRAJ_ROW_LOG_AVERAGED]))
    assert s.kernel.step_size == float(hist[-1, hip.TRAJ_ROW_NEXT_STEP_SIZE])
    assert 'ignored' in repr(s.kernel)
    x1 = wout.running_samples.last_sample.cpu()
    h, imd = s.kernel.step_size, s.kernel.inv_mass_diag.clone()
    Ls = [leapfrog_count(k, Tbar, h, s.params.max_leapfrog_steps) for k in range(T)]
    outs = [s.sample(x1, show_progress=False) for _ in range(2)]
    got = outs[0].samples.reshape(T, n, d)
    assert torch.isfinite(got).all()
    assert torch.equal(got, outs[1].samples.reshape(T, n, d))                       # bitwise, run to run
    for out in outs:
        st = out.statistics
        assert st.n_target_gradient_calls == 2 * n * sum(Ls), (st.n_target_gradient_calls, Ls)
        assert st.n_target_calls == 2 * n * sum(Ls) + 2 * n * T
        assert st.n_attempted_trajectories == n * T
    shadows = Shadows(target, s.seed, 0.01)
    for k, L in enumerate(Ls):
        shadows.transition(x1 if k == 0 else got[k - 1], got[k], h, imd, k, L, 'hand-off transition %d (L = %d)' % (k, L))
    shadows.check('hand-off')
    assert s.kernel.trajectory_length == Tbar and s.kernel.trajectory_history is hist   # sampling tunes nothing
    # max_leapfrog_steps pins L
    s.params.max_leapfrog_steps = 1
    out = s.sample(x1, show_progress=False)
    assert out.statistics.n_target_gradient_calls == 2 * n * T


def test_off_is_off(dev, monkeypatch):
    from nfmc_amd import hip
    from nfmc_amd.samplers import mcmc
    d, n = 8, 140
    pot, _t, draw = _target('offset', d, seed=d)
    x0 = draw(n).float()
    s = H.warmup_sampler('hmc', d, pot, 5, 4, 0.05)
    seen = []
    orig = mcmc.MetropolisSampler._args

    def args(self, run, pot, k, step0, samples, **kw):
        a = orig(self, run, pot, k, step0, samples, **kw)
        tune = kw.get('tune')
        seen.append((a.tune.trajectory, bool(a.tune.state), None if tune is None else tune.state.numel()))
        return a
    monkeypatch.setattr(mcmc.MetropolisSampler, '_args', args)
    wout = s.warmup(x0, show_progress=False)
    s.sample(wout.running_samples.last_sample, show_progress=False)
    base = int(hip.lib().nfmc_tune_state_doubles(d))
    assert seen[0] == (0, True, base) and seen[-1] == (0, False, None), seen           # no trailer, mode 0, no tuning state
    assert all(m == 0 for m, _s, _n in seen)
    assert s.kernel.trajectory_length is None and s.kernel.trajectory_history is None
    monkeypatch.undo()
    # the ABI refuses a mode without the Metropolis test, without a state, outside 1 .. 2, and on the Langevin entry point
    run = mcmc.Run(s, x0)
    for kind, mode, adjust, null_state, want in [('hmc', 1, 0, False, hip.EINVAL), ('hmc', 2, 0, False, hip.EINVAL),
                                                 ('hmc', 1, 1, True, hip.EINVAL), ('hmc', 2, 1, True, hip.EINVAL),
                                                 ('hmc', 3, 1, False, hip.EINVAL), ('hmc', -1, 1, False, hip.EINVAL),
                                                 ('mala', 1, 1, False, hip.EINVAL), ('mala', 2, 1, False, hip.EINVAL)]:
        smp = s if kind == 'hmc' else H.warmup_sampler('mala', d, pot, 5, 4, 0.05)
        tune = mcmc.DeviceTuning(s, run, hip.TRAJECTORY_ADAPT)                          # a state with a valid block behind it
        a = smp._args(run, pot, 1, 0, None, tune=tune)
        a.tune.trajectory = mode
        a.adjust = adjust
        if null_state:
            a.tune.state = None
        rc = getattr(hip.lib(), smp._entry)(C.byref(a), hip.stream())
        assert rc == want, (kind, mode, adjust, null_state, rc)
    torch.cuda.synchronize()
    assert torch.equal(run.x.cpu(), x0)                                                # nothing was launched


@pytest.mark.parametrize('name', ['unit8', 'lin16'])
def test_behaviour_matches_the_fp64_reference(dev, name):
    """The device's T-bar after 300 warmup transitions lies in the range of the fp64 free run over 8 seeds, widened on each
    side by that range."""
    from nfmc_amd.potentials import DiagonalGaussian
    from nfmc_amd.samplers import mcmc
    scales = CH.BEHAVIOUR[name]
    d = scales.numel()
    ref = np.array([CH.behaviour_reference(name, seed) for seed in range(8)])
    lo, hi = ref.min(), ref.max()
    pot = DiagonalGaussian((d,), 0.0, scales)
    s = mcmc.HMC((d,), pot, mcmc.HMCKernel(event_size=d, n_leapfrog_steps=CH.BEHAVIOUR_L0, step_size=CH.BEHAVIOUR_H0),
                 mcmc.HMCParameters(n_iterations=10, n_warmup_iterations=CH.BEHAVIOUR_W, tune_trajectory_length=True,
                                    tune_inv_mass_diag=False, store_samples=False))
    s.seed = 5
    s.warmup(CH.behaviour_x0(name, 0), show_progress=False)
    got = s.kernel.trajectory_length
    print('%s: device T-bar %.4f, fp64 free runs %s' % (name, got, np.round(ref, 4)))
    assert lo - (hi - lo) <= got <= hi + (hi - lo), (got, ref)
    assert s.kernel.trajectory_history.shape[0] == CH.BEHAVIOUR_W
