"""The device warmup (NfmcTune: the controller inside the statistics fold of the tuning launches) against an fp64 replay
of the controller (oracle/samplers.py: replay_controller) over the kernel's own kept states and accept counts, every
warmup transition shadowed in fp64 with the step size and mass diagonal the replay says it ran with, and the sampling
run that follows shadowed with the tuned kernel.  Also: both fold levels, the tune_every schedule against how the warmup
is cut into calls, targets far from the origin relative to their spread, and the Philox stream of a warmup against the
sampling run's.

  controller       step size and dual-averaging state to 1e-10 relative (integer accept counts: only fp64 reassociation
                   separates them), inv_mass_diag to a few fp32 ulps (fp32 partial sums of the shifted states), iteration exact
  transitions      oracle/shadow.py at kappa 8 (tests/test_gpu_benchmarked_workloads.py)
"""
import functools
import math

import numpy as np
import pytest
import torch

import target_harness as H
from target_harness import (check_controller as _check_controller, controller_params as _controller_params,
                            warmup_sampler as _sampler)

pytestmark = pytest.mark.gpu

_Record = functools.partial(H.Record, log_ratios=False)     # accept counts alone: the launches get no log-ratio buffer


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


def _tile(d):
    """Chains per tile of the mcmc kernels' default layout (4 waves x 64 / LPC chains, choose_cfg)."""
    for cpl, lpc in [(4, 1), (4, 2), (4, 4), (4, 8), (8, 8), (8, 16), (8, 32), (8, 64), (16, 64)]:
        if cpl * lpc >= d:
            return 4 * 64 // lpc
    raise ValueError(d)


# ------------------------------------------------------------------------------------------------ targets
def _target(name, d, seed=0):
    """(package potential, fp64-capable oracle callable, x0 generator)."""
    from nfmc_amd import potentials as P
    g = torch.Generator().manual_seed(seed)
    if name == 'sumsq':
        pot = P.SumOfSquares((d,))
        return pot, pot, lambda n: 0.7 * torch.randn(n, d, generator=g)
    if name == 'offset':
        mu, sig = torch.linspace(-3.0, 5.0, d), torch.linspace(0.5, 1.5, d)
        pot = P.DiagonalGaussian((d,), mu, sig)
        return pot, pot, lambda n: mu + sig * torch.randn(n, d, generator=g)
    if name == 'funnel':
        pot = P.Funnel((d,), 3.0)
        return pot, pot, lambda n: 0.5 * torch.randn(n, d, generator=g)
    if name.startswith('mixture'):
        K = int(name[len('mixture'):])
        means = 2.0 * torch.randn(K, d, generator=g)
        pot = P.GaussianMixture((d,), means, 0.8)
        return pot, pot, lambda n: means[torch.randint(0, K, (n,), generator=g)] + 0.8 * torch.randn(n, d, generator=g)
    if name == 'logreg':
        N = 96
        X = torch.randn(N, d, generator=g) / math.sqrt(d)
        y = (torch.rand(N, generator=g) < 0.5).double()
        pot = P.BayesianLogisticRegression(X, y)
        return pot, pot, lambda n: 0.3 * torch.randn(n, d, generator=g)
    if name == 'fullrank':
        A = torch.randn(d, d, generator=g, dtype=torch.float64) / math.sqrt(d)
        cov = A @ A.T + 0.5 * torch.eye(d, dtype=torch.float64)
        mu = torch.linspace(-1.0, 2.0, d, dtype=torch.float64)
        pot = P.FullRankGaussian(mu, covariance=cov)
        Lc = torch.linalg.cholesky(cov).float()
        return pot, pot, lambda n: mu.float() + torch.randn(n, d, generator=g) @ Lc.T
    if name == 'rosenbrock':
        pot = P.Rosenbrock((d,), mu=1.0, a=0.05, b=5.0, block=2)
        return pot, pot, lambda n: 1.0 + 0.2 * torch.randn(n, d, generator=g)
    raise ValueError(name)


# ------------------------------------------------------------------- 1-3. controller, transitions, handoff
# (kind, target, d, n, W, every): every closed-form target, every kind, every default lane layout, chain counts off the
# tile sizes, tune_every > 1 on the staged-LDS targets
CASES = [
    ('mala', 'sumsq', 1, 300, 12, 1),
    ('mala', 'offset', 3, 257, 12, 1),
    ('hmc', 'offset', 8, 129, 10, 3),
    ('ula', 'funnel', 25, 200, 10, 1),
    ('uhmc', 'mixture2', 8, 130, 8, 1),
    ('mala', 'mixture8', 3, 333, 12, 4),
    ('mh', 'offset', 64, 96, 10, 1),
    ('hmc', 'logreg', 8, 150, 10, 3),
    ('mala', 'fullrank', 25, 140, 12, 5),
    ('hmc', 'rosenbrock', 8, 140, 10, 2),
    ('mala', 'rosenbrock', 130, 70, 8, 1),
    ('mala', 'offset', 512, 40, 6, 1),
]


@pytest.mark.parametrize('kind,tname,d,n,W,every', CASES)
def test_warmup_controller_transitions_and_handoff(dev, monkeypatch, kind, tname, d, n, W, every):
    pot, target, draw = _target(tname, d, seed=d)
    x0 = draw(n).float()
    h0 = {'mala': 0.3, 'ula': 0.05, 'hmc': 0.1, 'uhmc': 0.05, 'mh': 0.3}[kind] * d ** (-1 / 3)
    if tname in ('funnel', 'rosenbrock', 'logreg'):
        h0 *= 0.3
    imd0 = torch.full((d,), 0.3 * d ** -0.5) if kind == 'mh' else torch.ones(d)
    # Rosenbrock's Hamiltonians are large next to their differences: fp32 rounding of the margin widens more tie windows
    ties = 0.05 if tname == 'rosenbrock' else 0.01
    H.warmup_matches_controller(monkeypatch, H.Problem(pot, target, target, x0, d, tname), kind, W=W, T=6, L=4, every=every,
                                h0=h0, imd0=imd0, seed=4242 + d, what='%s %s d=%d n=%d every=%d' % (kind, tname, d, n, every),
                                ties=ties)


# ------------------------------------------------------------------------------------------- 4. fold levels
@pytest.mark.parametrize('tname,d,extra_tiles', [('sumsq', 8, 1), ('mixture2', 3, 3), ('logreg', 8, 1)])
def test_fold_levels_agree(dev, monkeypatch, tname, d, extra_tiles):
    """More than 256 chain tiles: the default launch folds its slabs in two levels (tune_fold_kernel), NFMC_TUNE_ONE_LEVEL
    caps the grid at 256 workgroups that walk several tiles each.  Both against the replay and against each other."""
    from oracle import samplers as osamp
    pot, _t, draw = _target(tname, d, seed=3)
    n = (256 + extra_tiles) * _tile(d) + 37
    x0 = draw(n).float()
    W, h0 = 4, 0.2 * d ** (-1 / 3)
    got = {}
    for one in (False, True):
        if one:
            monkeypatch.setenv('NFMC_TUNE_ONE_LEVEL', '1')
        else:
            monkeypatch.delenv('NFMC_TUNE_ONE_LEVEL', raising=False)
        s = _sampler('mala', d, pot, W, 1, h0, beta=0.5)
        s.seed = 99
        rec = _Record(monkeypatch, s)
        wout = s.warmup(x0, show_progress=False)
        ups, _h, _m = osamp.replay_controller(wout.samples.reshape(W, n, d), rec.accepted(), 1,
                                              _controller_params(s, h0, torch.ones(d)))
        _check_controller(s, ups, '%s one_level=%s' % (tname, one))
        got[one] = (s.kernel.step_size, s.kernel.inv_mass_diag.clone())
        monkeypatch.undo()
    np.testing.assert_allclose(got[True][0], got[False][0], rtol=1e-6)
    np.testing.assert_allclose(got[True][1].numpy(), got[False][1].numpy(), rtol=1e-5)


# ------------------------------------------------------------------------------------------ 5. chunking
@pytest.mark.parametrize('W', [100, 1030])
@pytest.mark.parametrize('every', [1, 3, 7, 10])
def test_tune_every_schedule_does_not_depend_on_the_call_size(dev, every, W):
    """A progress bar or a time limit cuts the warmup into calls of max(32, every) transitions instead of 512: the
    controller must still update once per `every` transitions, ceil(W / every) times in all."""
    from nfmc_amd.potentials import DiagonalGaussian
    d, n = 6, 200
    pot = DiagonalGaussian((d,), torch.linspace(-1.0, 1.0, d), torch.linspace(0.5, 1.0, d))
    x0 = torch.randn(n, d, generator=torch.Generator().manual_seed(every))
    res = []
    for show, limit in ((False, None), (True, None), (False, 1e6)):
        s = _sampler('mala', d, pot, W, 1, 0.3, every=every)
        s.params.store_samples = False
        s.seed = 7
        out = s.warmup(x0, show_progress=show, time_limit_seconds=limit)
        res.append((s.kernel.step_size, s.kernel.inv_mass_diag.clone(), out.running_samples.last_sample.cpu(),
                    s.kernel.da.iteration))
    for r in res:
        assert r[3] == 10 + math.ceil(W / every), (every, W, [q[3] for q in res])
    for r in res[1:]:
        assert r[0] == res[0][0]
        assert torch.equal(r[1], res[0][1])
        assert torch.equal(r[2], res[0][2])


# ---------------------------------------------------------------------------------------- 6. offset targets
def _offset_problem(tname, d, ratio, seed=1):
    """A target whose chains sit at |mean| / spread ~ ratio: (potential, x0 draw, spread)."""
    from nfmc_amd import potentials as P
    g = torch.Generator().manual_seed(seed)
    if tname == 'diag':
        sig = torch.linspace(0.01, 0.02, d, dtype=torch.float64)
        mu = ratio * sig * torch.linspace(0.5, 1.0, d, dtype=torch.float64)
        return P.DiagonalGaussian((d,), mu, sig), lambda n: (mu + sig * torch.randn(n, d, generator=g, dtype=torch.float64)).float()
    if tname == 'fullrank':
        A = torch.randn(d, d, generator=g, dtype=torch.float64) / math.sqrt(d)
        cov = 1e-4 * (A @ A.T + 0.5 * torch.eye(d, dtype=torch.float64))
        sd = cov.diagonal().sqrt()
        mu = ratio * sd * torch.linspace(0.5, 1.0, d, dtype=torch.float64)
        Lc = torch.linalg.cholesky(cov)
        return (P.FullRankGaussian(mu, covariance=cov),
                lambda n: (mu + torch.randn(n, d, generator=g, dtype=torch.float64) @ Lc.T).float())
    # logistic regression with many rows: a narrow posterior about a large coefficient vector
    N = 4096
    theta = torch.full((d,), 3.0, dtype=torch.float64)
    X = torch.randn(N, d, generator=g, dtype=torch.float64)
    y = (torch.rand(N, generator=g, dtype=torch.float64) < torch.sigmoid(X @ theta)).double()
    pot = P.BayesianLogisticRegression(X.float(), y, prior_scale=100.0)
    return pot, lambda n: (theta + 0.05 * torch.randn(n, d, generator=g, dtype=torch.float64)).float()


@pytest.mark.parametrize('beta', [1e-3, 0.5, 1.0])
@pytest.mark.parametrize('tname,d,ratio', [('diag', 4, 1e3), ('diag', 8, 1e4), ('fullrank', 6, 3e3), ('logreg', 4, 0)])
def test_offset_target_mass_diagonal(dev, monkeypatch, tname, d, ratio, beta):
    """Chains far from the origin relative to their spread: one-pass fp32 sums of x and x^2 cancel.  The tuned
    inv_mass_diag matches the fp64 two-pass replay to 1e-4 relative, is finite and positive, and the sampling run
    that follows stays finite."""
    from oracle import samplers as osamp
    pot, draw = _offset_problem(tname, d, ratio)
    n, W = 300, 12
    x0 = draw(n)
    h0 = 1e-6 if tname != 'logreg' else 1e-5
    s = _sampler('mala', d, pot, W, 4, h0, beta=beta)
    s.seed = 11
    rec = _Record(monkeypatch, s)
    wout = s.warmup(x0, show_progress=False)
    ups, _h, _m = osamp.replay_controller(wout.samples.reshape(W, n, d), rec.accepted(), 1,
                                          _controller_params(s, h0, torch.ones(d)))
    got, want = s.kernel.inv_mass_diag.double(), ups[-1].inv_mass_diag.double()
    what = '%s d=%d m/s=%g beta=%g' % (tname, d, ratio, beta)
    assert torch.isfinite(got).all() and (got > 0).all(), (what, got)
    np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-4, err_msg=what)
    out = s.sample(wout.running_samples.last_sample, show_progress=False)
    assert torch.isfinite(out.samples).all(), what


# --------------------------------------------------------------------------------------------- 7. streams
class _Draws:
    """Every Philox draw range of the runs: (seed, first step, steps, warmup?) from Run.rng and hip.make_rng."""

    def __init__(self, monkeypatch):
        from nfmc_amd import hip
        from nfmc_amd.samplers import common
        self.ranges = []
        self.phase = [False]
        rng0, make0, init0 = common.Run.rng, hip.make_rng, common.Run.__init__

        def init(run, sampler, x0):
            init0(run, sampler, x0)
            self.phase[0] = bool(getattr(sampler.params, 'tuning', False))

        def rng(run, step0, k=0, adjusted=True):
            self.ranges.append((run.seed, int(step0), max(1, int(k)), self.phase[0]))
            self.inside = True
            try:
                return rng0(run, step0, k, adjusted)
            finally:
                self.inside = False

        def make(seed, chain_offset, step0, *a, **kw):
            if not getattr(self, 'inside', False):
                self.ranges.append((int(seed), int(step0), 1, self.phase[0]))
            return make0(seed, chain_offset, step0, *a, **kw)
        monkeypatch.setattr(common.Run, '__init__', init)
        monkeypatch.setattr(common.Run, 'rng', rng)
        monkeypatch.setattr(hip, 'make_rng', make)

    def shared(self):
        warm = [r for r in self.ranges if r[3]]
        samp = [r for r in self.ranges if not r[3]]
        assert warm and samp
        out = []
        for ws, w0, wk, _ in warm:
            for ss, s0, sk, _ in samp:
                if ws == ss and w0 < s0 + sk and s0 < w0 + wk:
                    out.append(((ws, w0, wk), (ss, s0, sk)))
        return out


@pytest.mark.parametrize('strategy', ['mala', 'hmc'])
def test_warmup_and_sampling_draw_disjoint_streams(dev, monkeypatch, strategy):
    """sample(seed=..., warmup=True): no (seed, chain, step, tag) draw of the warmup is drawn again by the sampling run
    (the state the warmup hands over was produced by those innovations)."""
    from nfmc_amd.potentials import SumOfSquares
    from nfmc_amd.sample import sample
    rec = _Draws(monkeypatch)
    out = sample(SumOfSquares((8,)), strategy=strategy, n_iterations=20, n_warmup_iterations=30, n_chains=64,
                 warmup=True, show_progress=False, seed=1234)
    assert torch.isfinite(out.samples).all()
    shared = rec.shared()
    assert not shared, shared[:3]


def test_jump_warmup_and_run_draw_disjoint_streams(dev, monkeypatch):
    """jump_mala: the inner sampler's warmup does not inherit the run's seed -- it draws a fresh one, so its stream is
    apart from the run's by seed (the warmup step offset is not what separates them here) -- and no draw of the warmup
    is drawn again by the run."""
    from nfmc_amd.potentials import SumOfSquares
    from nfmc_amd.sample import create_sampler
    rec = _Draws(monkeypatch)
    d = 6
    s = create_sampler(target=SumOfSquares((d,)), event_shape=(d,), strategy='jump_mala',
                       param_kwargs={'n_iterations': 3, 'n_warmup_iterations': 20})
    s.params.warmup_fit_kwargs.update(n_epochs=5, n_samples=64)
    s.seed = 4321
    x0 = torch.randn(64, d)
    w = s.warmup(x0, show_progress=False)
    out = s.sample(w.running_samples.last_sample, show_progress=False)
    assert torch.isfinite(out.samples).all()
    warm_seeds = {r[0] for r in rec.ranges if r[3]}
    run_seeds = {r[0] for r in rec.ranges if not r[3]}
    assert 4321 in run_seeds, run_seeds
    assert warm_seeds and 4321 not in warm_seeds, warm_seeds
    assert not rec.shared(), rec.shared()[:3]
