"""GPU: LatentGaussianModel (NFMC_POT_LATENT_GAUSSIAN) on the fused HIP kernels against the fp64 CPU oracle, with the
target restated in fp64 (tests/latent_gaussian_fp64.py).  Section by section the full-rank Gaussian's file
(tests/test_gpu_fullrank.py), plus the overflow and the two-parameterisation checks this kind needs.

Problem (latent_gaussian_fp64.problem_data): d seeded uniform points in the unit square, K = SE(variance 1, lengthscale
0.25) + 0.05 I, m = 1 for Poisson and 0 otherwise, a generating state z* ~ N(0, I); weights U(0.5, 1.5) (Poisson), trials
1 .. 5 (binomial), 1 (Student-t, nu = 4, s = 0.5, 10 % outliers of 5 s); a seeded 20 % of the coordinates unobserved.
Starts are z* + 0.3 eps mapped to the object's parameterisation and rounded to fp32.

Step sizes, lambda = hessian_bound at the generating state: mala 1.5 d^(-1/3) / lambda, ula 0.1 d^(-1/3) / lambda,
hmc 1.0 d^(-1/4) / sqrt(lambda) with L = 5, uhmc 0.3 d^(-1/4) / sqrt(lambda), mh proposal scale 0.5 / sqrt(d lambda).

Tolerances are the full-rank file's: MARGIN 2e-3, ATOL 1e-3 + RTOL 1e-4, and the harness's 10 % cap on near-ties.  With
these inputs the fp64 oracle alone (96 chains, 4 transitions, d in DIMS, all six (likelihood, parameterisation) pairs)
puts at most 2.1 % of the chains of a mala, hmc or mh run within 2e-3 of a tie, accepts 0.64 to 1.0 of the proposals
(both branches of the accept step are taken), and keeps max |f| <= 4.2: no overflow at the test inputs.

DIMS covers every default (CPL, LPC) layout below (16, 64) and tiles of 1024 rows (d <= 4) down to 8 rows (d = 512), so
each matrix streams through up to 64 tiles per pass, and the whitened form makes two passes.

Flow-proposal cases (section 2 and 2b): from d = 25 on a flow centred by a Laplace fit (H.flow_inputs).  The fp64 oracle
alone accepts 0.092 to 0.236 of the jumps and 0.176 to 0.495 of the IMH proposals of section 2, and in the matrix 0.161 to
0.826 up to capacity 128 and 0.042 to 0.411 above; at most 2.1 % of the chains of a case are within MARGIN of a tie.  At
capacities 128 and 256 some proposals are hopeless (fp64 log ratios down to -547): those cases set skip_below_minus_50;
the others keep every log ratio above -50.
"""
import functools
import math

import pytest
import torch

import target_harness as H
from latent_gaussian_fp64 import PAIRS, LatentGaussian64, make_pair, problem_data, starts, truth
from target_harness import Spy as _Spy, flow_pair as _flow_pair

pytestmark = pytest.mark.gpu

MARGIN = 2e-3
ATOL, RTOL = 1e-3, 1e-4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


class _Problem:
    """What the harness takes (pot, ref, target, x0, d, name) with the problem's data and lambda."""

    def __init__(self, d, lik, par, seed, n, x0_seed, event_shape=None):
        self.data = _data(d, lik, seed)
        self.pot, self.ref = make_pair(self.data, par, event_shape)
        self.target = self.ref
        self.x0 = starts(self.data, self.ref, n, x0_seed)
        self.d, self.name = d, '%s %s d=%d' % (lik, par, d)
        self.lam = self.pot.hessian_bound(truth(self.data, self.ref))


@functools.lru_cache(maxsize=None)
def _data(d, lik, seed):
    return problem_data(d, lik, seed)


_compare = functools.partial(H.compare_states, margin=MARGIN, atol=ATOL, rtol=RTOL)
_sampler = functools.partial(H.mcmc_sampler, imd_kinds=('mh',))      # Langevin and HMC keep the unit mass diagonal
_oracle = functools.partial(H.oracle_trace, imd_kinds=('mh',))


def _mh_scale(p):
    return torch.full((p.d,), 0.5 / math.sqrt(p.d * p.lam), dtype=torch.float64)


def _step(kind, p):
    if kind in ('hmc', 'uhmc'):
        return {'hmc': 1.0, 'uhmc': 0.3}[kind] * p.d ** (-1 / 4) / math.sqrt(p.lam)
    return {'mala': 1.5, 'ula': 0.1, 'mh': 0.0}[kind] * p.d ** (-1 / 3) / p.lam


KINDS = list(H.KINDS)
DIMS = [1, 3, 8, 25, 64, 130, 256, 512]


def _pair_of(d):
    """(likelihood, parameterisation) rotating with d over the six pairs"""
    return PAIRS[DIMS.index(d) % len(PAIRS)] if d in DIMS else PAIRS[d % len(PAIRS)]


def _against_oracle(check, monkeypatch, kind, p, T, event_shape=None, decisions=H.compare_decisions, **kw):
    h, imd = _step(kind, p), _mh_scale(p)
    shape = p.d if event_shape is None else event_shape
    check(monkeypatch, p, kind, T, _sampler(kind, shape, p.pot, T, h, imd=imd),
          lambda noise: _oracle(kind, p.x0, p.target, T, h, noise, imd=imd, label=p.name), compare=_compare,
          decisions=decisions, **({} if event_shape is None else {'event_shape': event_shape}), **kw)


# ------------------------------------------------------------------------- 1. fused kernels vs fp64 oracle, replayed noise
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d', DIMS)
def test_mcmc_replay_matches_oracle(dev, monkeypatch, kind, d):
    lik, par = _pair_of(d)
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, _Problem(d, lik, par, 10 * d + 1, 96, d + 2), 4, torch_seed=d,
                    what='%s %s %s d=%d' % (kind, lik, par, d))


@pytest.mark.parametrize('lik,par', PAIRS)
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
@pytest.mark.parametrize('d', [25, 130])
def test_every_likelihood_and_parameterisation(dev, monkeypatch, kind, d, lik, par):
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, _Problem(d, lik, par, 10 * d + 1, 96, d + 2), 4, torch_seed=d,
                    what='%s %s %s d=%d' % (kind, lik, par, d))


@pytest.mark.parametrize('kind,lik,par', [('mala', 'poisson', 'whitened'), ('hmc', 'student_t', 'centered')])
def test_two_dimensional_event_shape(dev, monkeypatch, kind, lik, par):
    """(H, W) = (5, 5) through event_shape=: the kernels see the flattened d = 25."""
    p = _Problem(25, lik, par, 77, 96, 5, event_shape=(5, 5))
    assert p.pot.event_shape == (5, 5)
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, p, 4, event_shape=(5, 5), torch_seed=25,
                    what='%s (5, 5) %s %s' % (kind, lik, par))


# ------------------------------------------------------------------------- 2. native Philox streams
# all on the whitened binomial problem, which is near N(0, I): the flow's jump proposals are accepted
@pytest.mark.parametrize('kind,d', [('mala', 25), ('ula', 8), ('mh', 130), ('hmc', 64), ('uhmc', 3), ('hmc', 512)])
def test_mcmc_native_stream_matches_oracle(dev, monkeypatch, kind, d):
    _against_oracle(H.native_matches_oracle, monkeypatch, kind, _Problem(d, 'binomial', 'whitened', 7 * d + 3, 160, d), 5,
                    seed=777 + d, what='native %s d=%d' % (kind, d))


@functools.lru_cache(maxsize=None)
def _flow_built(d, lik, par, seed, n, x0_seed):
    """one object per distinct problem of the flow tests: the Laplace fit (H.laplace_fit) is kept per object"""
    return _Problem(d, lik, par, seed, n, x0_seed)


@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('d', [5, 25, 64])
def test_jump_mala_native_stream_matches_oracle(dev, monkeypatch, fuse_tail, d):
    n, T = 192, 3
    p = _flow_built(d, 'binomial', 'whitened', 3 * d + 5, n, 3)
    q, flows = H.flow_inputs(p, d, n)
    H.jump_mala_matches_oracle(monkeypatch, q, T=T, Kin=4, seed=31337, h=0.3 * d ** (-1 / 3) / p.lam, imd=None,
                               fuse_tail=fuse_tail, spline=False, atol=ATOL, rtol=RTOL, share=0.95,
                               jump_slack=max(2, int(0.03 * n * T)), margin=MARGIN, skip_below_minus_50=False, flows=flows)


@pytest.mark.parametrize('d', [2, 25, 64, 256])
def test_imh_runs_on_the_sequential_flow_mh_kernel(dev, monkeypatch, d):
    p = _flow_built(d, 'binomial', 'whitened', 5 * d + 7, 256, 9)
    q, flows = H.flow_inputs(p, d, 256, 9)
    H.imh_matches_oracle(monkeypatch, q, T=6, seed=4711 + d, flow_seed=9, spline=False, compare=_compare, what='imh d=%d' % d,
                         margin=MARGIN, skip_below_minus_50=False, flows=flows)


# ------------------------------------------------------------------------- 2b. the flow-MH matrix
FLOW_CASES = H.flow_cases()
FLOW_TESTS = ('test_jump_mala_native_stream_matches_oracle', 'test_imh_runs_on_the_sequential_flow_mh_kernel',
              'test_flow_mh_matrix')
# the 120 KB LDS bound with this kind's 16 KB tile of the matrix behind the image: two affine coupling layers of width 8
# at the ragged capacity 512 are 132 KB by themselves, two spline layers of width 8 at capacity 64 are 111 KB
FLOW_REFUSED = {'mh-cap512-d300-h8', 'jump_mala-cap512-d300-h8', 'mh-cap64-d50-h8-spline', 'mh-cap64-d50-h8-cpl8-spline'}
# a diagonal proposal against the prior's correlations: Poisson / whitened at d = 100 and binomial / centred at d = 200
# have fp64 log ratios down to -547 and -158
FLOW_SKIP_CAPS = (128, 256)


@pytest.mark.parametrize('case', FLOW_CASES, ids=H.flow_case_id)
def test_flow_mh_matrix(dev, monkeypatch, case):
    """H.flow_cases: every flow-MH layout, sibling, width and coupling, the unadjusted carry path and the jump tails, with
    decisions and log ratios compared row by row (H.compare_flow_mh); the (likelihood, parameterisation) pair rotates
    with the capacity"""
    d = case.d
    lik, par = PAIRS[int(math.log2(case.cap)) % len(PAIRS)]
    p = _flow_built(d, lik, par, 5 * d + 7, 96, 9)
    H.run_flow_case(dev, monkeypatch, p, case, margin=MARGIN, compare=_compare, atol=ATOL, rtol=RTOL,
                    h_mala=0.3 * d ** (-1 / 3) / p.lam, h_hmc=0.5 * d ** (-1 / 4) / math.sqrt(p.lam),
                    refused=H.flow_case_id(case) in FLOW_REFUSED, skip_caps=FLOW_SKIP_CAPS)


# ------------------------------------------------------------------------- 3. fused equals split
@pytest.mark.parametrize('kind,d,lik,par', [('mala', 25, 'poisson', 'whitened'), ('hmc', 9, 'student_t', 'centered'),
                                            ('mh', 64, 'binomial', 'whitened')])
def test_fused_equals_split(dev, monkeypatch, kind, d, lik, par):
    T = 6
    p = _Problem(d, lik, par, 17 * d, 200, 17)
    H.fused_equals_split(monkeypatch, p, lambda target: _sampler(kind, d, target, T, _step(kind, p), imd=_mh_scale(p)), T,
                         seed=2024, atol=ATOL, rtol=RTOL, share=0.95)


# ------------------------------------------------------------------------- 4. NeuTra (VALU kernels)
@pytest.mark.parametrize('par', ['centered', 'whitened'])
@pytest.mark.parametrize('d,nh', [(2, 4), (3, 8), (8, 16), (25, 32), (64, 8), (64, 32), (128, 16), (130, 8), (256, 4)])
def test_neutra_gradient_matches_fp64_autograd(dev, d, nh, par):
    """On a perturbed RealNVP (couplings need d >= 2); the likelihood rotates with the shape.  d = 64 / 128 are the
    shapes the matrix-core kernels would take for the other kinds.  Tolerance: relative 2e-4 of (1 + max |.|) per row."""
    lik = ('poisson', 'binomial', 'student_t')[(d + nh) % 3]
    p = _Problem(d, lik, par, 11 * d + nh, 130, d)
    H.neutra_gradient_matches_autograd(dev, p.pot, p.ref, p.x0, nh, '%s %s d=%d H=%d' % (lik, par, d, nh), flow_seed=3,
                                       bound=2e-4)


@pytest.mark.parametrize('d,nh,lik,par', [(8, 8, 'poisson', 'whitened'), (64, 16, 'binomial', 'centered'),
                                          (128, 8, 'student_t', 'whitened')])
def test_neutra_hmc_fused_matches_oracle(dev, monkeypatch, d, nh, lik, par):
    p = _Problem(d, lik, par, 13 * d, 96, 61)
    H.neutra_hmc_fused_matches_oracle(monkeypatch, p, _flow_pair(d, 9, n_hidden=nh), T=3, L=4, h=0.2 / math.sqrt(p.lam),
                                      seed=12, atol=1e-3, share=0.93, accept_slack=6)


def test_neutra_wide_conditioner_takes_the_split_path_and_matches_the_oracle(dev):
    d = 64
    p = _Problem(d, 'binomial', 'whitened', 29, 96, 62)
    H.neutra_wide_takes_the_split_path(dev, p, _flow_pair(d, 9, n_hidden=64), T=3, L=4, h=0.2 / math.sqrt(p.lam), seed=12,
                                       atol=1e-3, share=0.93)


# ------------------------------------------------------------------------- 5. refused entry points, bad descriptors
@pytest.mark.parametrize('par', ['centered', 'whitened'])
def test_refusing_entry_points_answer_unsupported(dev, par):
    from nfmc_amd import hip
    d = 64
    p = _Problem(d, 'poisson', par, 4, 256, 4)
    pd = p.pot.descriptor(dev)
    assert pd.kind == hip.POT_LATENT_GAUSSIAN and pd.n_components == d and pd.a_scalar == (4.0 if par == 'whitened' else 0.0)
    H.refusing_entry_points(dev, p.pot, p.x0, functools.partial(_flow_pair, d))


def test_philox7_and_bad_descriptors_are_refused(dev):
    """A NULL matrix block or table, n_components != d and an invalid code are argument errors; a misaligned matrix block
    or table is an alignment error."""
    from nfmc_amd import hip
    d = 25
    p = _Problem(d, 'student_t', 'whitened', 8, 128, 8)
    b = p.pot.descriptor(dev).b
    bad = [('a', 0, hip.EINVAL), ('b', 0, hip.EINVAL), ('a', 'misaligned', hip.EALIGN), ('b', b + 4, hip.EALIGN),
           ('b', b + 8, hip.EALIGN), ('n_components', d - 1, hip.EINVAL), ('n_components', d + 1, hip.EINVAL),
           ('a_scalar', 3.0, hip.EINVAL), ('a_scalar', 7.0, hip.EINVAL), ('a_scalar', 8.0, hip.EINVAL),
           ('a_scalar', 4.5, hip.EINVAL), ('a_scalar', -1.0, hip.EINVAL)]
    ok = [('a_scalar', float(c)) for c in (0, 1, 2, 4, 5, 6)]
    H.bad_descriptors_are_refused(dev, p.pot, p.x0, _flow_pair(d)[0], bad, ok)


# ------------------------------------------------------------------------- 6. determinism and sharding
@pytest.mark.parametrize('kind,lik,par', [('mala', 'poisson', 'whitened'), ('hmc', 'binomial', 'centered')])
def test_determinism_and_sharding(dev, kind, lik, par):
    d, T = 20, 8
    p = _Problem(d, lik, par, 44, 300, 44)
    H.determinism_and_sharding(lambda: _sampler(kind, d, p.pot, T, _step(kind, p)), p.x0, T, d, seed=7, world=2)


# ------------------------------------------------------------------------- 7. overflow
def test_overflowing_poisson_rates_are_rejected_and_the_state_stays_finite(dev, monkeypatch):
    """d = 8, Poisson, centred, random-walk proposals of scale 40: many proposals have f > 89, where e^f overflows fp32
    and U = inf.  Every kept state is finite; every proposal whose fp64 log ratio is below -50 or non-finite is rejected
    by the kernel; the others are compared as everywhere (states, masks, log ratios of the finite ones).  In fp64 every
    proposal of these inputs is below -50 (a step of scale 40 in 8 coordinates), so the kernel must reject them all."""
    d, n, T = 8, 96, 4
    p = _Problem(d, 'poisson', 'centered', 81, n, 10)
    imd = torch.full((d,), 40.0, dtype=torch.float64)
    s = _sampler('mh', d, p.pot, T, 0.0, imd=imd)
    out, tr, rec, spy = H.replay_run(monkeypatch, s, lambda noise: _oracle('mh', p.x0, p.target, T, 0.0, noise, imd=imd,
                                                                            label='overflow'), p.x0, 8, True)
    assert not spy.calls
    got = out.samples.reshape(T, n, d)
    assert bool(torch.isfinite(got).all())
    _compare(got, tr, 'overflow')
    got_m, _got_lr = rec.stacked()
    want_lr = torch.stack([v.reshape(-1).double() for v in tr.log_ratios])
    hopeless = ~torch.isfinite(want_lr) | (want_lr < -50)
    # the states stay at x0 while everything is rejected, so the proposals are x0 + 40 eps: one of the 8 coordinates
    # passes 89 when its eps > 2.2, which is 8 x 1.4 % of the proposals
    prop = p.x0.double()[None] + 40.0 * torch.stack([v.reshape(n, d).double() for v in s.replay[0]])
    over = float((prop.amax(2) > 89).float().mean())
    print('overflow: %.0f %% of the proposals hopeless, %.0f %% with some f > 89' % (100 * float(hopeless.float().mean()), 100 * over))
    assert over > 0.05
    assert not bool(got_m[hopeless].any())
    if bool((~hopeless).any()):                              # at this scale usually none: nothing finite is left to compare
        H.compare_decisions(rec, tr, 'mh', p.x0, p.ref, 'overflow', skip_below_minus_50=True)
    else:
        assert not bool(got_m.any())


# ------------------------------------------------------------------------- 8. statistics of long fused runs
LGCP = dict(variance=1.0, lengthscale=0.25, jitter=0.05, mean=math.log(60.0))


def _lgcp(par, seed=5):
    """A 4 x 4 log-Gaussian Cox process (lengthscale of one cell and a nugget of 0.05, so that the centred form mixes
    within the run too) with counts drawn at a seeded generating state: (potential, f*)."""
    from nfmc_amd.potentials import LatentGaussianModel
    g = torch.Generator().manual_seed(seed)
    proto = LatentGaussianModel.log_gaussian_cox(torch.zeros(4, 4), parameterization=par, **LGCP)
    f = proto.mean + proto.cholesky @ torch.randn(16, generator=g, dtype=torch.float64)
    counts = torch.poisson(proto.weight * torch.exp(f), generator=g).reshape(4, 4)
    return LatentGaussianModel.log_gaussian_cox(counts, parameterization=par, **LGCP), f


def _long_run(monkeypatch, pot, f0, T, L, h, seed):
    """T fused HMC transitions from the f-space starts f0; (per-chain time averages of f over every 4th state of the
    last 4/5 (n, d), pooled sd of f (d,), acceptance)."""
    d, n = pot.dim, f0.shape[0]
    s = _sampler('hmc', pot.event_shape, pot, T, h, L=L)
    s.seed = seed
    spy = _Spy(monkeypatch)
    out = s.sample(pot.coordinates(f0).float().reshape((n,) + pot.event_shape), show_progress=False)
    assert not spy.calls
    acc = out.statistics.n_accepted_trajectories / (n * T)
    kept = pot.latent(out.samples.reshape(T, n, d)[T // 5::4].double())
    return kept.mean(0), kept.reshape(-1, d).std(0), acc


def test_both_parameterisations_sample_the_same_posterior(dev, monkeypatch):
    """d = 16 (a 4 x 4 LGCP), 4096 chains, 200 fused HMC transitions (L = 8), once per parameterisation from the same
    f-space starts.  The posterior means of f agree within 5 combined standard errors (from the per-chain time
    averages: the chains are independent) + 0.02 posterior sd, the full-rank file's allowance for the leapfrog's O(h^2)
    bias.  Acceptance in (0.5, 1); no split-path call.  Step 1.0 d^(-1/4) / sqrt(lambda) = 0.5 / sqrt(lambda), lambda the
    Hessian bound at the generating state."""
    n, T, L = 4096, 200, 8
    means, ses, sds = [], [], []
    for par in ('whitened', 'centered'):
        pot, fstar = _lgcp(par)
        g = torch.Generator().manual_seed(3)
        f0 = fstar[None] + 0.3 * torch.randn(n, 16, generator=g, dtype=torch.float64) @ pot.cholesky.t()
        h = 16 ** (-1 / 4) / math.sqrt(pot.hessian_bound(pot.coordinates(fstar)))
        per_chain, sd, acc = _long_run(monkeypatch, pot, f0, T, L, h, 2718)
        print('%s: acceptance %.3f' % (par, acc))
        assert 0.5 < acc < 1.0, (par, acc)
        means.append(per_chain.mean(0))
        ses.append(per_chain.std(0) / math.sqrt(n))
        sds.append(sd)
    diff = (means[0] - means[1]).abs()
    bound = 5 * torch.sqrt(ses[0] ** 2 + ses[1] ** 2) + 0.02 * torch.maximum(sds[0], sds[1])
    print('worst mean difference / bound %.3f' % float((diff / bound).max()))
    assert bool((diff < bound).all()), (diff.tolist(), bound.tolist())


@pytest.mark.parametrize('par', ['whitened', 'centered'])
def test_one_dimensional_posterior_mean_matches_quadrature(dev, monkeypatch, par):
    """d = 1, Poisson: the fused run's mean of f against fp64 quadrature of the posterior on a fine grid, within 5 SE."""
    from nfmc_amd.potentials import LatentGaussianModel
    k, m, y, w = 0.8, 0.5, 3.0, 1.5
    pot = LatentGaussianModel(torch.tensor([y]), torch.tensor([[k]]), 'poisson', mean=m, weight=w, parameterization=par)
    grid = torch.linspace(m - 12 * math.sqrt(k), m + 12 * math.sqrt(k), 200001, dtype=torch.float64)
    logp = -0.5 * (grid - m) ** 2 / k - (w * torch.exp(grid) - y * grid)
    wts = torch.exp(logp - logp.max())
    want = float((wts * grid).sum() / wts.sum())
    n, T, L = 4096, 200, 8
    f0 = want + 0.5 * torch.randn(n, 1, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    h = 1.0 / math.sqrt(pot.hessian_bound(pot.coordinates(torch.tensor([want], dtype=torch.float64))))
    per_chain, _sd, acc = _long_run(monkeypatch, pot, f0, T, L, h, 99)
    mean, se = float(per_chain.mean()), float(per_chain.std() / math.sqrt(n))
    print('%s: mean %.5f quadrature %.5f se %.5f acceptance %.3f' % (par, mean, want, se, acc))
    assert 0.5 < acc <= 1.0, acc
    assert abs(mean - want) < 5 * se, (mean, want, se)
