"""GPU: stochastic volatility (NFMC_POT_STOCHASTIC_VOLATILITY) on the fused HIP kernels against the fp64 CPU oracle, with
the target restated in fp64 (tests/sv_fp64.py).

Every problem is a series of T = d - 3 returns simulated from the model at mu = -1, sigma = 0.25, phi = 0.95; chains
start near those parameters with h near the simulated path (sv_fp64.start_states).  The oracle samplers evaluate the
model's log densities from torch.distributions in fp64 (sv_fp64.constrained_u64, U up to one constant: vectorised, and
independent of both the kernels and the class); values are checked against the loop of sv_fp64.SVU64.  Step sizes scale
with the largest diagonal Hessian entry at the start (90th percentile over the chains).

Tolerances are the Rosenbrock tests' (tests/test_gpu_rosenbrock.py):
  states        atol 1e-3 + rtol 1e-4
  decisions     tie-aware: a chain whose fp64 |log u - log ratio| falls under MARGIN at any of its transitions is
                excluded; the excluded share must stay under 10 %, all other chains must match.

d in {4, 5, 8, 25, 64, 130, 256, 512, 1024} covers every default (CPL, LPC) layout choose_cfg picks (LPC 1 ... 64, CPL
4 / 8 / 16) and the lane wrap of the neighbour exchange.

Flow-proposal cases (section 2 and 2b).  The posterior's mode in log sigma is degenerate (a Laplace fit leaves it with a
gradient of 1e8), so from d = 25 the proposals sit about the mean of the file's starts with 0.3 of the conditional
standard deviations there (_flow_centre), and the inner steps of the jumps shrink with them.  The fp64 oracle alone
accepts 0.036 to 0.155 of the jumps and up to 0.325 of the IMH proposals of section 2 (none at the spline d = 6, a flow
about the origin), and in the matrix 0.115 to 0.495 up to capacity 128 and 0.307 to 0.406 above; under 1 % of the chains
of a case are within MARGIN of a tie.  Some proposals are hopeless (fp64 log ratios down to -8602, in the matrix -234):
every case sets skip_below_minus_50.
"""
import functools
import math

import pytest
import torch

import target_harness as H
from sv_fp64 import SVU64, constrained_u64, start_states
from target_harness import Spy as _Spy

pytestmark = pytest.mark.gpu

MARGIN = 2e-3
ATOL, RTOL = 1e-3, 1e-4
SKIP = True     # skip_below_minus_50 of the flow-MH cases: a proposal's log sigma can be far off: see the docstring
MU, SIGMA, PHI = -1.0, 0.25, 0.95


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


def _problem(d, n, seed, spread=0.05):
    """(potential, fp64 loop, fp64 oracle target, x0 fp32 (n, d))"""
    from nfmc_amd.potentials import StochasticVolatility
    y, x0, _ = start_states(d - 3, n, seed, MU, SIGMA, PHI, spread)
    return StochasticVolatility(y), SVU64(y), functools.partial(constrained_u64, y=y), x0.float()


def _lmax(ref, x0):
    return float(torch.quantile(ref.hess_diag(x0.double()).abs().amax(dim=1), 0.9))


def _record(d, n, seed, spread=0.05):
    """the problem as the harness takes it, and the curvature its steps scale with"""
    pot, ref, target, x0 = _problem(d, n, seed, spread)
    return H.Problem(pot, ref, target, x0, d, 'd=%d' % d), _lmax(ref, x0)


_compare = functools.partial(H.compare_states, margin=MARGIN, atol=ATOL, rtol=RTOL)
_sampler = functools.partial(H.mcmc_sampler, imd_kinds=('mh',))      # Langevin and HMC keep the unit mass diagonal
_oracle = functools.partial(H.oracle_trace, imd_kinds=('mh',))


def _mh_scale(d, lm):
    return torch.full((d,), 0.5 / math.sqrt(d * lm), dtype=torch.float64)


def _step(kind, d, lm):
    """MALA h ~ d^(-1/3) / lambda_max; HMC h ~ d^(-1/4) / sqrt(lambda_max)"""
    if kind in ('hmc', 'uhmc'):
        return {'hmc': 0.5, 'uhmc': 0.3}[kind] * d ** (-1 / 4) / math.sqrt(lm)
    return {'mala': 0.5, 'ula': 0.1, 'mh': 0.0}[kind] * d ** (-1 / 3) / lm


def _compare_decisions(rec, tr, kind, x0, ref, what):
    """Log ratios to 2e-4 max(1, d / 64) + 1e-4 |log r| + 8 ulp(fp32) (|U(x)| + sum_t |h_t| / 2), the second term for the
    lane partial sums of a U whose data terms cancel.  Finite fp64 log ratios above -50 only: H.compare_decisions says why."""
    H.compare_decisions(rec, tr, kind, x0, ref, what, skip_below_minus_50=True,
                        mag=lambda prev: ref(prev).abs() + 0.5 * prev[:, 3:].abs().sum(1))


KINDS = ['mala', 'ula', 'mh', 'hmc', 'uhmc']
DIMS = [4, 5, 8, 25, 64, 130, 256, 512, 1024]


def _against_oracle(check, monkeypatch, kind, d, n, T, problem_seed, **kw):
    p, lm = _record(d, n, problem_seed)
    h, imd = _step(kind, d, lm), _mh_scale(d, lm)
    check(monkeypatch, p, kind, T, _sampler(kind, d, p.pot, T, h, imd=imd),
          lambda noise: _oracle(kind, p.x0, p.target, T, h, noise, imd=imd), compare=_compare, decisions=_compare_decisions, **kw)


# ------------------------------------------------------------------------- 1. fused kernels vs fp64 oracle, replayed noise
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d', DIMS)
def test_mcmc_replay_matches_oracle(dev, monkeypatch, kind, d):
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, d, 96, 4, d, torch_seed=d, what='%s d=%d' % (kind, d))


# ------------------------------------------------------------------------- 2. native Philox streams
@pytest.mark.parametrize('kind,d', [('mala', 25), ('ula', 8), ('mh', 130), ('hmc', 64), ('uhmc', 5), ('hmc', 1024),
                                    ('mala', 512), ('hmc', 4)])
def test_mcmc_native_stream_matches_oracle(dev, monkeypatch, kind, d):
    _against_oracle(H.native_matches_oracle, monkeypatch, kind, d, 160, 5, d + 1, seed=777 + d, what='native %s d=%d' % (kind, d))


@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('d', [5, 25, 64])
def test_jump_mala_native_stream_matches_oracle(dev, monkeypatch, fuse_tail, d):
    n, T = 192, 3
    p, lm = _record(d, n, 3 + d)
    q, flows = H.flow_inputs(p, d, n, centre=_flow_centre(p))
    shrink = FLOW_SHRINK ** 2 if d >= 25 else 1.0          # the inner steps shrink with the proposal: test_flow_mh_matrix
    H.jump_mala_matches_oracle(monkeypatch, q, T=T, Kin=4, seed=31337, h=shrink * 0.3 * d ** (-1 / 3) / lm, imd=None, fuse_tail=fuse_tail,
                               spline=False, atol=ATOL, rtol=RTOL, share=0.95, jump_slack=max(2, int(0.03 * n * T)), margin=MARGIN,
                               skip_below_minus_50=SKIP, flows=flows)


@pytest.mark.parametrize('d,spline', [(4, False), (25, False), (130, False), (256, False), (6, True), (33, True)])
def test_imh_runs_on_the_sequential_flow_mh_kernel(dev, monkeypatch, d, spline):
    """Affine and spline ('c-rqnsf') instantiations of the register flow-MH kernel for kind 6.  The flows are near the
    identity, so starts with a wide spread give a useful share of accepted proposals."""
    p, _lm = _record(d, 256, 9 + d, spread=0.3)
    q, flows = H.flow_inputs(p, d, 256, 3 if spline else 9, spline=spline, centre=_flow_centre(p))
    H.imh_matches_oracle(monkeypatch, q, T=6, seed=4711 + d, flow_seed=3 if spline else 9, spline=spline, compare=_compare,
                         what='%s imh d=%d' % ('c-rqnsf' if spline else 'realnvp', d), margin=MARGIN, skip_below_minus_50=SKIP,
                         flows=flows)

# ------------------------------------------------------------------------- 2b. the flow-MH matrix
FLOW_DIMS = dict(H.FLOW_DIMS)
FLOW_DIMS[4] = 4                       # d = T + 3 >= 4: capacity 4 is an exact fit
FLOW_SKIP_CAPS = (4, 8, 16, 32, 64, 128, 256, 512)    # some proposals are hopeless at every capacity: see the docstring
FLOW_CASES = H.flow_cases(FLOW_DIMS)
FLOW_TESTS = ('test_jump_mala_native_stream_matches_oracle', 'test_imh_runs_on_the_sequential_flow_mh_kernel',
              'test_flow_mh_matrix')
# the 120 KB LDS bound: two affine coupling layers of width 8 at the ragged capacity 512 are 132 KB by themselves
FLOW_REFUSED = {'mh-cap512-d300-h8', 'jump_mala-cap512-d300-h8'}
FLOW_SHRINK = 0.3


@functools.lru_cache(maxsize=None)
def _flow_problem(d):
    """one object per distinct problem of the flow tests: the fit of the proposal's centre is kept per object"""
    return _record(d, 96, 9 + d)


def _flow_centre(p):
    """The posterior's mode in log sigma is degenerate (a Laplace fit leaves with a gradient of 1e8): the proposals sit about the
    mean of the file's starts, FLOW_SHRINK of the conditional standard deviations there"""
    return H.local_fit(p, FLOW_SHRINK, at='starts')


@pytest.mark.parametrize('case', FLOW_CASES, ids=H.flow_case_id)
def test_flow_mh_matrix(dev, monkeypatch, case):
    """H.flow_cases: every flow-MH layout, sibling, width and coupling, the unadjusted carry path and the jump tails, with
    decisions and log ratios compared row by row (H.compare_flow_mh).  The inner steps of the jump cases shrink with the
    proposal (FLOW_SHRINK^2 for MALA, FLOW_SHRINK for HMC), so that a chain is still inside it when the jump comes."""
    d = case.d
    p, lm = _flow_problem(d)
    H.run_flow_case(dev, monkeypatch, p, case, margin=MARGIN, compare=_compare, atol=ATOL, rtol=RTOL,
                    h_mala=FLOW_SHRINK ** 2 * 0.3 * d ** (-1 / 3) / lm, h_hmc=FLOW_SHRINK * _step('hmc', d, lm),
                    refused=H.flow_case_id(case) in FLOW_REFUSED, centre=_flow_centre(p), skip_caps=FLOW_SKIP_CAPS)


# ------------------------------------------------------------------------- 3. fused equals split
@pytest.mark.parametrize('kind,d', [('mala', 25), ('hmc', 9), ('mh', 64), ('hmc', 130)])
def test_fused_equals_split(dev, monkeypatch, kind, d):
    T = 6
    p, lm = _record(d, 200, 17 + d)
    H.fused_equals_split(monkeypatch, p, lambda target: _sampler(kind, d, target, T, _step(kind, d, lm), imd=_mh_scale(d, lm)), T,
                         seed=2024, atol=ATOL, rtol=RTOL, share=0.95)


# ------------------------------------------------------------------------- 4. NeuTra (VALU kernels)
@pytest.mark.parametrize('d,nh', [(4, 4), (5, 8), (8, 16), (25, 32), (64, 8), (64, 32), (128, 16), (130, 8), (256, 4),
                                  (512, 8)])
def test_neutra_gradient_matches_fp64_autograd(dev, d, nh):
    """Against fp64 autograd through oracle/flow.py and the loop of SVU64, at latents whose images under the
    near-identity flow are model-like (the starts).  Tolerance: relative 2e-4 of (1 + max |.|) per row."""
    p, _lm = _record(d, 130, 5 + d)
    H.neutra_gradient_matches_autograd(dev, p.pot, p.ref, p.x0, nh, 'd=%d H=%d' % (d, nh), flow_seed=3, bound=2e-4)


@pytest.mark.parametrize('d,nh', [(8, 8), (64, 16), (128, 8)])
def test_neutra_hmc_fused_matches_oracle(dev, monkeypatch, d, nh):
    p, lm = _record(d, 96, 61 + d)
    H.neutra_hmc_fused_matches_oracle(monkeypatch, p, H.flow_pair(d, 9, n_hidden=nh), T=3, L=4, h=0.2 / math.sqrt(lm), seed=12,
                                      atol=1e-3, share=0.93, accept_slack=6)


def test_neutra_wide_conditioner_takes_the_split_path_and_matches_the_oracle(dev):
    d = 64
    p, lm = _record(d, 96, 62)
    H.neutra_wide_takes_the_split_path(dev, p, H.flow_pair(d, 9, n_hidden=64), T=3, L=4, h=0.2 / math.sqrt(lm), seed=12,
                                       atol=1e-3, share=0.93)


# ------------------------------------------------------------------------- 5. device warmup against the fp64 controller
@pytest.mark.parametrize('kind,d,n,W,every', [('mala', 25, 140, 12, 1), ('hmc', 25, 150, 16, 2), ('mala', 130, 70, 8, 1)])
def test_warmup_controller_transitions_and_handoff(dev, monkeypatch, kind, d, n, W, every):
    """As tests/test_gpu_warmup.py does for the other kinds."""
    p, lm = _record(d, n, 7 + d)
    H.warmup_matches_controller(monkeypatch, p, kind, W=W, T=6, L=4, every=every, h0=0.3 * _step(kind, d, lm), imd0=torch.ones(d),
                                seed=4242 + d, what='sv %s d=%d n=%d every=%d' % (kind, d, n, every), ties=0.05)


# ------------------------------------------------------------------------- 6. refused entry points, bad descriptors
def test_refusing_entry_points_answer_unsupported(dev):
    from nfmc_amd import hip
    d = 64
    pot, _ref, _t, x0 = _problem(d, 256, 4)
    pd = pot.descriptor(dev)
    assert pd.kind == hip.POT_STOCHASTIC_VOLATILITY and pd.n_components == d - 3
    H.refusing_entry_points(dev, pot, x0, functools.partial(H.flow_pair, d))


def test_philox7_and_bad_descriptors_are_refused(dev):
    """A NULL y or (alpha, beta), T not d - 3 or < 1, and c_mu or c_sigma not positive and finite are argument errors."""
    from nfmc_amd import hip
    d = 25
    pot, _ref, _t, x0 = _problem(d, 128, 8)
    bad = [('a', 0), ('b', 0), ('n_components', 0), ('n_components', d - 2), ('n_components', d - 4), ('n_components', -1),
           ('a_scalar', 0.0), ('a_scalar', -1.0), ('a_scalar', float('inf')), ('b_scalar', 0.0), ('b_scalar', float('nan'))]
    H.bad_descriptors_are_refused(dev, pot, x0, H.flow_pair(d)[0], [(f, v, hip.EINVAL) for f, v in bad])


# ------------------------------------------------------------------------- 7. determinism and sharding
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
def test_determinism_and_sharding(dev, kind):
    d, T = 20, 8
    p, lm = _record(d, 300, 44)
    H.determinism_and_sharding(lambda: _sampler(kind, d, p.pot, T, _step(kind, d, lm)), p.x0, T, d, seed=7, world=2)


@pytest.mark.parametrize('kind', ['mala', 'mh', 'hmc'])
def test_overflowing_proposals_are_rejected_and_counted(dev, kind):
    """Steps far past stability: proposals reach s < -44 or h_t < -88, where w = e^{-2s} or e^{-h_t} overflows fp32, so U
    of the proposal is inf or NaN and the log ratio is not finite.  The adjusted kernels reject every such proposal and
    count it as non-finite (n_nonfinite_log_ratios), as for the existing kinds; the kept states stay finite."""
    d, n, T = 16, 512, 10
    pot, ref, _t, x0 = _problem(d, n, 3)
    h = {'mala': 1e4, 'mh': 0.0, 'hmc': 50.0}[kind]
    s = _sampler(kind, d, pot, T, h, L=3, imd=torch.full((d,), 1e6, dtype=torch.float64))
    s.seed = 5
    out = s.sample(x0, show_progress=False)
    st = out.statistics
    assert st.n_attempted_trajectories == n * T
    assert torch.isfinite(out.samples).all()
    assert torch.isfinite(out.mean).all()
    print(kind, 'non-finite', st.n_nonfinite_log_ratios, 'accepted', st.n_accepted_trajectories)
    assert st.n_nonfinite_log_ratios > n * T // 2
    assert st.n_accepted_trajectories + st.n_nonfinite_log_ratios <= n * T


# ------------------------------------------------------------------------- 8. correctness without an oracle
def test_long_hmc_run_satisfies_the_stein_identities(dev, monkeypatch):
    """T = 20, 65536 chains, the informative Beta(20, 1.5) prior on (phi + 1)/2 of Kim, Shephard and Chib (1998): after a
    device warmup (step size and mass diagonal) a long fused HMC run, every 500th of 10000 states per chain kept.  Under
    the target E[dU/dx_c] = 0 and E[x_c dU/dx_c] = 1 for every coordinate (integration by parts).  Both hold within 5
    standard errors, estimated across chains from per-chain averages, for every coordinate but s = log sigma, where
    E[dU/ds] is printed and not asserted: the centred parameterisation mixes slowly in sigma at T = 20, and the same run on
    the autograd split path gave the same z-scores for s (and, with phi uniform, for r), so that bias belongs to the
    sampler on this posterior, not to the kernels."""
    from nfmc_amd.potentials import StochasticVolatility
    d, n, W, T, L = 23, 65536, 2000, 10000, 8
    _pot, _ref, _t, x0 = _problem(d, n, 2020, spread=0.2)
    y = _pot.y
    pot, ref = StochasticVolatility(y, phi_prior=(20.0, 1.5)), SVU64(y, alpha=20.0, beta=1.5)
    s = _sampler('hmc', d, pot, T, 0.3 * _step('hmc', d, _lmax(ref, x0[:512])), L=L)
    s.params.n_warmup_iterations = W
    s.params.thinning = 500
    s.seed = 99
    spy = _Spy(monkeypatch)
    x1 = s.warmup(x0, show_progress=False).running_samples.last_sample.cpu()
    out = s.sample(x1, show_progress=False)
    assert not spy.calls
    acc = out.statistics.n_accepted_trajectories / (n * T)
    print('acceptance', acc, 'step', s.kernel.step_size)
    assert 0.4 < acc < 1.0, acc
    kept = out.samples.reshape(-1, n, d).double()                     # (20, n, d)
    assert kept.shape[0] == T // 500
    g = ref.grad(kept.reshape(-1, d)).reshape(kept.shape)
    for name, stat, want in (('E[dU/dx]', g, 0.0), ('E[x dU/dx]', kept * g, 1.0)):
        per_chain = stat.mean(0)                                       # (n, d)
        m = per_chain.mean(0)
        se = per_chain.std(0) / math.sqrt(n)
        print(name, ((m - want) / se).tolist())
        ok = (m - want).abs() < 5 * se
        ok[1] = True                                                   # s = log sigma: see the docstring
        assert bool(ok.all()), (name, (m - want).tolist(), se.tolist())


def test_sample_jump_mala_recovers_the_simulating_parameters(dev):
    """End to end: sample(..., strategy='jump_mala') on a T = 500 series simulated at mu = -1, sigma = 0.25, phi = 0.95.
    Each constrained posterior mean (over chains and kept states) lies within 4 posterior standard deviations of the
    simulating value."""
    from nfmc_amd import sample
    d, n = 503, 4096
    pot, ref, _t, x0 = _problem(d, n, 500)
    h = 0.3 * d ** (-1 / 3) / _lmax(ref, x0[:256])
    out = sample(pot, flow='realnvp', strategy='jump_mala', n_iterations=40, n_chains=n, x0=x0, show_progress=False,
                 seed=3, inner_kernel_kwargs={'step_size': h}, inner_param_kwargs={'n_iterations': 10})
    kept = out.samples.reshape(-1, n, d)
    assert torch.isfinite(kept).all()
    kept = kept[kept.shape[0] // 2:].reshape(-1, d).double()
    mu, sigma, phi, _h = pot.constrain(kept)
    for name, v, want in (('mu', mu, MU), ('sigma', sigma, SIGMA), ('phi', phi, PHI)):
        print(name, float(v.mean()), float(v.std()), want)
        assert abs(float(v.mean()) - want) < 4 * float(v.std()), name
