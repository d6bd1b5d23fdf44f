"""GPU: FullRankGaussian (NFMC_POT_GAUSSIAN_FULL) on the fused HIP kernels against the fp64 CPU oracle, with the target
restated in fp64 (tests/fullrank_fp64.py).

Targets: precision matrices of condition number up to 1e3 (eigenvalues log-spaced from 1 to cond in a seeded random
basis); starts are draws of the target itself, spread 1.2x, so U(x) ~ d / 2 and its fp32 rounding stays small.  Step
sizes scale with 1 / lambda_max (the stiffest direction), as any sampler of such a target must.

Tolerances are the logistic-regression tests' (tests/test_gpu_logreg.py):
  states        atol 1e-3 + rtol 1e-4.  The gradient is a sum of d terms Lambda_ij r_i in fp32; h Lambda r moves a
                transition by ~1e-6 relative, and the comparison runs a handful of transitions.
  decisions     tie-aware: a chain whose fp64 |log u - log ratio| falls under MARGIN at any of its transitions is
                excluded; the excluded share must stay under 10 %, all other chains must match.

d in {1, 3, 8, 25, 64, 130, 256, 512} covers every (CPL, LPC) layout choose_cfg picks (LPC 1 ... 64, CPL 4 / 8 / 16 at
d = 512 in the jump-tail-free kernels: (8, 64)) and tiles of 1024 rows (d <= 4) down to 8 rows (d = 512), so that
Lambda streams through up to 64 tiles per evaluation.

Flow-proposal cases (section 2 and 2b).  On a flow about the origin the fp64 oracle alone accepted 4 of 1536 IMH
proposals at d = 25 and none at d = 64 and 256, so from d = 25 they run on a flow centred by a Laplace fit
(H.flow_inputs).  With the present inputs the oracle alone accepts 865, 406, 285 and 436 of 1536 IMH proposals at d = 2,
25, 64 and 256 (0.186 to 0.563) and 0.064 to 0.361 of the jumps of section 2, and in the matrix 0.156 to 0.729 up to
capacity 128 and 0.229 to 0.401 above; at most 1.2 % of the chains of a case are within MARGIN of a tie, and every log
ratio is above -31.
"""
import functools
import math

import pytest
import torch

import target_harness as H
from fullrank_fp64 import FullRankU64, draw, spd
from target_harness import Spy as _Spy, flow_pair as _flow_pair

pytestmark = pytest.mark.gpu

MARGIN = 2e-3
ATOL, RTOL = 1e-3, 1e-4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


def _cond(d):
    return 1e3 if d >= 3 else 10.0


def _problem(d, seed, cond=None):
    """The class and its fp64 restatement: precision spd(d, cond), mean of O(1)."""
    from nfmc_amd.potentials import FullRankGaussian
    lam = spd(d, cond if cond is not None else _cond(d), seed)
    mu = 0.5 * torch.randn(d, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64)
    return FullRankGaussian(mu, precision=lam), FullRankU64(lam, mu)


def _x0(ref, n, seed):
    return draw(ref.lam, ref.mu, n, seed, spread=1.2).float()


def _lmax(ref):
    return float(torch.linalg.eigvalsh(ref.lam).max())


def _record(d, seed, n, x0_seed, cond=None):
    """the problem as the harness takes it: the restatement is the oracle's target"""
    pot, ref = _problem(d, seed, cond)
    return H.Problem(pot, ref, ref, _x0(ref, n, x0_seed), d, 'd=%d' % d)


_compare = functools.partial(H.compare_states, margin=MARGIN, atol=ATOL, rtol=RTOL)
_sampler = functools.partial(H.mcmc_sampler, imd_kinds=('mh',))      # Langevin and HMC keep the unit mass diagonal
_oracle = functools.partial(H.oracle_trace, imd_kinds=('mh',))


def _mh_scale(d, ref):
    return torch.full((d,), 0.5 / math.sqrt(d * _lmax(ref)), dtype=torch.float64)


def _step(kind, d, ref):
    """MALA h ~ d^(-1/3) / lambda_max; HMC h ~ d^(-1/4) / sqrt(lambda_max) (the leapfrog's stability limit is
    2 / sqrt(lambda_max))."""
    lm = _lmax(ref)
    if kind in ('hmc', 'uhmc'):
        return {'hmc': 0.5, 'uhmc': 0.3}[kind] * d ** (-1 / 4) / math.sqrt(lm)
    return {'mala': 0.5, 'ula': 0.1, 'mh': 0.0}[kind] * d ** (-1 / 3) / lm


KINDS = ['mala', 'ula', 'mh', 'hmc', 'uhmc']
DIMS = [1, 3, 8, 25, 64, 130, 256, 512]


def _against_oracle(check, monkeypatch, kind, p, T, **kw):
    """Log ratios: the kernel's U(x) and U(x') are fp32 sums of d^2 products, so their difference cannot be closer than a
    few of their ulps (H.compare_decisions)."""
    d = p.d
    h, imd = _step(kind, d, p.ref), _mh_scale(d, p.ref)
    check(monkeypatch, p, kind, T, _sampler(kind, d, p.pot, T, h, imd=imd),
          lambda noise: _oracle(kind, p.x0, p.target, T, h, noise, imd=imd), compare=_compare, decisions=H.compare_decisions, **kw)


# ------------------------------------------------------------------------- 1. fused kernels vs fp64 oracle, replayed noise
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d', DIMS)
def test_mcmc_replay_matches_oracle(dev, monkeypatch, kind, d):
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, _record(d, 10 * d + 1, 96, d + 2), 4, torch_seed=d,
                    what='%s d=%d' % (kind, d))


# ------------------------------------------------------------------------- 2. native Philox streams
@pytest.mark.parametrize('kind,d', [('mala', 25), ('ula', 8), ('mh', 130), ('hmc', 64), ('uhmc', 3), ('hmc', 512)])
def test_mcmc_native_stream_matches_oracle(dev, monkeypatch, kind, d):
    _against_oracle(H.native_matches_oracle, monkeypatch, kind, _record(d, 7 * d + 3, 160, d), 5, seed=777 + d,
                    what='native %s d=%d' % (kind, d))


@functools.lru_cache(maxsize=None)
def _mild(d, seed, n, x0_seed):
    """a mildly correlated target (cond 4), one object per distinct problem (the Laplace fit is kept per object)"""
    return _record(d, seed, n, x0_seed, cond=4.0)


@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('d', [5, 25, 64])
def test_jump_mala_native_stream_matches_oracle(dev, monkeypatch, fuse_tail, d):
    """A mildly correlated target (cond 4).  At d = 5 the jump proposals of a perturbed identity-like flow are accepted
    often enough (97 of 576 in the fp64 oracle alone); from d = 25 the flow is centred on the target (H.flow_inputs)."""
    n, T = 192, 3
    p = _mild(d, 3 * d + 5, n, 3)
    q, flows = H.flow_inputs(p, d, n)
    H.jump_mala_matches_oracle(monkeypatch, q, T=T, Kin=4, seed=31337, h=0.3 * d ** (-1 / 3) / _lmax(p.ref), imd=None,
                               fuse_tail=fuse_tail, spline=False, atol=ATOL, rtol=RTOL, share=0.95,
                               jump_slack=max(2, int(0.03 * n * T)), margin=MARGIN, skip_below_minus_50=False, flows=flows)


@pytest.mark.parametrize('d', [2, 25, 64, 256])
def test_imh_runs_on_the_sequential_flow_mh_kernel(dev, monkeypatch, d):
    p = _mild(d, 5 * d + 7, 256, 9)
    q, flows = H.flow_inputs(p, d, 256, 9)
    H.imh_matches_oracle(monkeypatch, q, T=6, seed=4711 + d, flow_seed=9, spline=False, compare=_compare, what='imh d=%d' % d,
                         margin=MARGIN, skip_below_minus_50=False, flows=flows)


# ------------------------------------------------------------------------- 2b. the flow-MH matrix
FLOW_CASES = H.flow_cases()
FLOW_TESTS = ('test_jump_mala_native_stream_matches_oracle', 'test_imh_runs_on_the_sequential_flow_mh_kernel',
              'test_flow_mh_matrix')
# the 120 KB LDS bound with this kind's 16 KB tile of Lambda behind the image: two affine coupling layers of width 8 at
# the ragged capacity 512 are 132 KB by themselves, two spline layers of width 8 at capacity 64 are 111 KB
FLOW_REFUSED = {'mh-cap512-d300-h8', 'jump_mala-cap512-d300-h8', 'mh-cap64-d50-h8-spline', 'mh-cap64-d50-h8-cpl8-spline'}


@pytest.mark.parametrize('case', FLOW_CASES, ids=H.flow_case_id)
def test_flow_mh_matrix(dev, monkeypatch, case):
    """H.flow_cases: every flow-MH layout, sibling, width and coupling, the unadjusted carry path and the jump tails, with
    decisions and log ratios compared row by row (H.compare_flow_mh); the mildly correlated target (cond 4)"""
    d = case.d
    p = _mild(d, 5 * d + 7, 96, 9)
    H.run_flow_case(dev, monkeypatch, p, case, margin=MARGIN, compare=_compare, atol=ATOL, rtol=RTOL,
                    h_mala=0.3 * d ** (-1 / 3) / _lmax(p.ref), h_hmc=0.5 * d ** (-1 / 4) / math.sqrt(_lmax(p.ref)),
                    refused=H.flow_case_id(case) in FLOW_REFUSED)


# ------------------------------------------------------------------------- 3. fused equals split
@pytest.mark.parametrize('kind,d', [('mala', 25), ('hmc', 9), ('mh', 64)])
def test_fused_equals_split(dev, monkeypatch, kind, d):
    T = 6
    p = _record(d, 17 * d, 200, 17)
    H.fused_equals_split(monkeypatch, p,
                         lambda target: _sampler(kind, d, target, T, _step(kind, d, p.ref), imd=_mh_scale(d, p.ref)), T, seed=2024, atol=ATOL, rtol=RTOL, share=0.95)


# ------------------------------------------------------------------------- 4. NeuTra (VALU kernels)
@pytest.mark.parametrize('d,nh', [(2, 4), (3, 8), (8, 16), (25, 32), (64, 8), (64, 32), (128, 16), (130, 8), (256, 4)])
def test_neutra_gradient_matches_fp64_autograd(dev, d, nh):
    """On a perturbed RealNVP (couplings need d >= 2).  d = 64 / 128 are the shapes the matrix-core kernels would take
    for the other kinds.  Tolerance: relative 2e-4 of (1 + max |.|) per row, fp32 arithmetic through the coupling stack
    and a d-term dot product per gradient coordinate."""
    pot, ref = _problem(d, 11 * d + nh, cond=100.0)
    H.neutra_gradient_matches_autograd(dev, pot, ref, draw(ref.lam, torch.zeros(d), 130, d), nh, 'd=%d H=%d' % (d, nh),
                                       flow_seed=3, bound=2e-4)


@pytest.mark.parametrize('d,nh', [(8, 8), (64, 16), (128, 8)])
def test_neutra_hmc_fused_matches_oracle(dev, monkeypatch, d, nh):
    p = _record(d, 13 * d, 96, 61, cond=10.0)
    H.neutra_hmc_fused_matches_oracle(monkeypatch, p, _flow_pair(d, 9, n_hidden=nh), T=3, L=4, h=0.2 / math.sqrt(_lmax(p.ref)),
                                      seed=12, atol=1e-3, share=0.93, accept_slack=6)


def test_neutra_wide_conditioner_takes_the_split_path_and_matches_the_oracle(dev):
    d = 64
    p = _record(d, 29, 96, 62, cond=10.0)
    H.neutra_wide_takes_the_split_path(dev, p, _flow_pair(d, 9, n_hidden=64), T=3, L=4, h=0.2 / math.sqrt(_lmax(p.ref)), seed=12,
                                       atol=1e-3, share=0.93)


# ------------------------------------------------------------------------- 5. refused entry points, bad descriptors
def test_refusing_entry_points_answer_unsupported(dev):
    from nfmc_amd import hip
    d = 64
    pot, ref = _problem(d, 4)
    pd = pot.descriptor(dev)
    assert pd.kind == hip.POT_GAUSSIAN_FULL and pd.n_components == d
    H.refusing_entry_points(dev, pot, _x0(ref, 256, 4), functools.partial(_flow_pair, d))


def test_philox7_and_bad_descriptors_are_refused(dev):
    """A NULL Lambda or mu, a misaligned Lambda and n_components != d are argument errors."""
    from nfmc_amd import hip
    d = 25
    pot, ref = _problem(d, 8)
    bad = [('a', 0), ('b', 0), ('a', 'misaligned'), ('n_components', d - 1), ('n_components', d + 1)]
    H.bad_descriptors_are_refused(dev, pot, _x0(ref, 128, 8), _flow_pair(d)[0], [(f, v, hip.EINVAL) for f, v in bad])


# ------------------------------------------------------------------------- 6. determinism and sharding
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
def test_determinism_and_sharding(dev, kind):
    d, T = 20, 8
    p = _record(d, 44, 300, 44)
    H.determinism_and_sharding(lambda: _sampler(kind, d, p.pot, T, _step(kind, d, p.ref)), p.x0, T, d, seed=7, world=2)


def test_sample_api_with_a_two_dimensional_event(dev):
    """nfmc_amd.sample() takes the object and its (2, 4) event shape; the kernels see the flattened d = 8."""
    from nfmc_amd import sample
    from nfmc_amd.potentials import FullRankGaussian
    lam = spd(8, 10.0, 3)
    pot = FullRankGaussian(torch.zeros(2, 4), precision=lam, event_shape=(2, 4))
    out = sample(pot, flow=None, strategy='hmc', n_iterations=5, n_chains=64, show_progress=False, seed=1,
                 x0=draw(lam, torch.zeros(8), 64, 1).float().reshape(64, 2, 4),
                 kernel_kwargs={'step_size': 0.2 / math.sqrt(float(torch.linalg.eigvalsh(lam).max())),
                                'n_leapfrog_steps': 3})
    assert out.samples.shape[-2:] == (2, 4)
    assert torch.isfinite(out.samples).all() and out.statistics.n_attempted_trajectories == 64 * 5


# ------------------------------------------------------------------------- 7. statistics of a long fused run
def test_long_hmc_run_recovers_mean_and_covariance(dev, monkeypatch):
    """d = 8, covariance with correlations up to |rho| ~ 0.9 (condition number 100), 4096 chains started from the
    target, 200 fused HMC transitions (L = 8), every 4th state of the last 160 kept: 40 x 4096 draws.  Consecutive kept
    states are nearly independent at this step (acceptance checked), but the bounds use the per-chain time averages
    anyway: the chains are independent, so the spread of those averages gives an honest standard error.
      mean       |E[x] - mu|_j < 5 SE_j
      covariance |S_jk - Sigma_jk| < 5 SE_jk + 0.02 sqrt(Sigma_jj Sigma_kk), SE_jk from the per-chain second-moment
                 averages; the 0.02 absorbs the leapfrog's O(h^2) bias of the stationary law"""
    from nfmc_amd.potentials import FullRankGaussian
    d, n, T, L = 8, 4096, 200, 8
    lam = spd(d, 100.0, 91)
    cov = torch.linalg.inv(lam)
    cov = 0.5 * (cov + cov.t())
    rho = cov / torch.sqrt(torch.diagonal(cov)[:, None] * torch.diagonal(cov)[None, :])
    assert float((rho - torch.eye(d, dtype=torch.float64)).abs().max()) > 0.5      # strongly correlated
    mu = torch.linspace(-2.0, 3.0, d, dtype=torch.float64)
    pot = FullRankGaussian(mu, covariance=cov)
    h = 0.25 / math.sqrt(float(torch.linalg.eigvalsh(lam).max()))
    s = _sampler('hmc', d, pot, T, h, L=L)
    s.seed = 2718
    spy = _Spy(monkeypatch)
    out = s.sample(draw(lam, mu, n, 5).float(), show_progress=False)
    assert not spy.calls
    acc = out.statistics.n_accepted_trajectories / (n * T)
    assert 0.5 < acc < 1.0, acc
    kept = out.samples.reshape(T, n, d)[T // 5::4].double()                   # (40, n, d)
    m = kept.shape[0]
    per_chain = kept.mean(0)                                                   # (n, d)
    mean = per_chain.mean(0)
    se = per_chain.std(0) / math.sqrt(n)
    print('mean', mean.tolist(), 'se', se.tolist())
    assert bool(((mean - mu).abs() < 5 * se).all()), ((mean - mu).tolist(), se.tolist())
    r = kept - mu
    second = torch.einsum('tni,tnj->nij', r, r) / m                           # (n, d, d) per-chain averages
    S = second.mean(0)
    se2 = second.std(0) / math.sqrt(n)
    scale = torch.sqrt(torch.diagonal(cov)[:, None] * torch.diagonal(cov)[None, :])
    err = (S - cov).abs()
    print('worst covariance error / scale', float((err / scale).max()))
    assert bool((err < 5 * se2 + 0.02 * scale).all()), float((err - 5 * se2).max())
    # the kernel's own running moments agree with the stored states
    assert torch.isfinite(out.mean).all()


@pytest.mark.parametrize('kind', KINDS)
def test_ill_conditioned_targets_stay_finite(dev, kind):
    """Condition number 1e6 at d = 64, step sizes set by the stiffest direction: every state finite, no divergence
    counted; the loose directions barely move, which is the sampler's problem, not the kernel's."""
    d, n, T = 64, 512, 20
    pot, ref = _problem(d, 3, cond=1e6)
    x0 = _x0(ref, n, 3)
    s = _sampler(kind, d, pot, T, _step(kind, d, ref), imd=_mh_scale(d, ref))
    s.seed = 5
    out = s.sample(x0, show_progress=False)
    assert torch.isfinite(out.samples).all()
    assert torch.isfinite(out.mean).all() and torch.isfinite(out.second_moment).all()
    st = out.statistics
    assert st.n_attempted_trajectories == n * T
    assert getattr(st, 'n_divergences', 0) == 0
