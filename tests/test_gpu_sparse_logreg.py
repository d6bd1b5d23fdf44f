"""GPU: sparse logistic regression (NFMC_POT_SPARSE_LOGISTIC_REGRESSION) on the fused HIP kernels against the fp64 CPU
oracle, with the target restated in fp64 (tests/sparse_logreg_fp64.py).

Every problem is a synthetic data set drawn from the model (standardised X, three nonzero coefficients), X scaled by
2 / sqrt(N) so that the data curvature stays O(1) at every N; chains start at sparse_logreg_fp64.start_states.  The oracle
samplers evaluate the model's log densities from torch.distributions in fp64 (sparse_logreg_fp64.model_u64, U up to one
constant: independent of both the kernels and the class); values are checked against the loops of SLRU64.  Step sizes
scale with the largest diagonal Hessian entry at the start (90th percentile over the chains).

Tolerances are the logistic-regression tests' (tests/test_gpu_logreg.py):
  states        atol 1e-3 + rtol 1e-4
  decisions     tie-aware: a chain whose fp64 |log u - log ratio| falls under MARGIN at any of its transitions is
                excluded; the excluded share must stay under 10 %, all other chains must match.

d = 2 D + 1 reaches every default (CPL, LPC) layout choose_cfg picks: d = 3 -> (4, 1), 5 -> (4, 2), 9 -> (4, 4), 25 ->
(4, 8), 51 -> (8, 8), 101 -> (8, 16), 255 -> (8, 32), 401 -> (8, 64), 1023 -> (16, 64), capacities 4 to 1024.  The compact
LDS tile holds 8192 / capacity rows (2048 at d = 3, 8 at d = 1023); N covers 1, 63, 64, 65, 1000 and N past one tile.

Flow-proposal cases (section 3 and 3b).  The horseshoe's mode in the log scales is degenerate, so from d = 25 the
proposals sit about the mean of the file's starts with 0.3 of the conditional standard deviations there (_flow_centre).
The fp64 oracle alone accepts 0.059 to 0.405 of the jumps and up to 0.490 of the IMH proposals of section 3 (none at the
spline d = 9, a flow about the origin), and in the matrix 0.214 to 0.583 up to capacity 128 and 0.305 to 0.464 above; at
most 2.1 % of the chains of a case are within MARGIN of a tie.  Some proposals are hopeless (fp64 log ratios down to
-9074, in the matrix -88): every case sets skip_below_minus_50.
"""
import ctypes as C
import functools
import math

import pytest
import torch

import target_harness as H
from sparse_logreg_fp64 import SLRU64, log_gamma_moments, model_u64, prior_draws, start_states, synthetic
from target_harness import Spy as _Spy, flow_pair as _flow_pair

pytestmark = pytest.mark.gpu

MARGIN = 2e-3
ATOL, RTOL = 1e-3, 1e-4
SKIP = True     # skip_below_minus_50 of the flow-MH cases: a proposal's local scales can be far off: see the docstring


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


def _problem(d, N, n, seed, spread=1.0):
    """(potential, fp64 loop, fp64 oracle target, x0 fp32 (n, d))"""
    from nfmc_amd.potentials import SparseLogisticRegression
    D = (d - 1) // 2
    X, y, _ = synthetic(N, D, seed, scale=2.0 / math.sqrt(N))
    x0 = start_states(D, n, seed + 1, spread)
    return SparseLogisticRegression(X, y), SLRU64(X, y), functools.partial(model_u64, X=X, y=y), x0.float()


def _lmax(ref, x0):
    return float(torch.quantile(ref.hess_diag(x0.double()).abs().amax(dim=1), 0.9))


def _record(d, N, n, seed, spread=1.0):
    """the problem as the harness takes it, and the curvature its steps scale with"""
    pot, ref, target, x0 = _problem(d, N, n, seed, spread)
    return H.Problem(pot, ref, target, x0, d, 'd=%d N=%d' % (d, N)), _lmax(ref, x0)


_compare = functools.partial(H.compare_states, margin=MARGIN, atol=ATOL, rtol=RTOL)
# finite fp64 log ratios above -50 only: H.compare_decisions says why
_compare_decisions = functools.partial(H.compare_decisions, skip_below_minus_50=True)
_sampler = functools.partial(H.mcmc_sampler, imd_kinds=('mh',))      # Langevin and HMC keep the unit mass diagonal
_oracle = functools.partial(H.oracle_trace, imd_kinds=('mh',))


def _mh_scale(d, lm):
    return torch.full((d,), 0.5 / math.sqrt(d * lm), dtype=torch.float64)


def _step(kind, d, lm):
    """MALA h ~ d^(-1/3) / lambda_max; HMC h ~ d^(-1/4) / sqrt(lambda_max)"""
    if kind in ('hmc', 'uhmc'):
        return {'hmc': 0.5, 'uhmc': 0.3}[kind] * d ** (-1 / 4) / math.sqrt(lm)
    return {'mala': 0.5, 'ula': 0.1, 'mh': 0.0}[kind] * d ** (-1 / 3) / lm


KINDS = ['mala', 'ula', 'mh', 'hmc', 'uhmc']
# (d, N): every default layout; N = 1, 63, 64, 65, 1000, and N past one tile (2048 rows at d = 3, 16 at d = 401,
# 8 at d = 1023)
GRID = [(3, 1), (3, 2100), (5, 63), (9, 64), (25, 65), (51, 1000), (101, 65), (255, 63), (401, 40), (1023, 1),
        (1023, 64)]


def _against_oracle(check, monkeypatch, kind, d, N, n, T, problem_seed, **kw):
    p, lm = _record(d, N, n, problem_seed)
    h, imd = _step(kind, d, lm), _mh_scale(d, lm)
    check(monkeypatch, p, kind, T, _sampler(kind, d, p.pot, T, h, imd=imd),
          lambda noise: _oracle(kind, p.x0, p.target, T, h, noise, imd=imd), compare=_compare, decisions=_compare_decisions, **kw)


# ------------------------------------------------------------------------- 1. fused kernels vs fp64 oracle, replayed noise
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('d,N', GRID)
def test_mcmc_replay_matches_oracle(dev, monkeypatch, kind, d, N):
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, d, N, 96, 4, d + N, torch_seed=d + N,
                    what='%s d=%d N=%d' % (kind, d, N))


# ------------------------------------------------------------------------- 2. native Philox streams
@pytest.mark.parametrize('kind,d,N', [('mala', 51, 1000), ('ula', 9, 65), ('mh', 101, 300), ('hmc', 25, 129),
                                      ('uhmc', 5, 1100), ('hmc', 1023, 20), ('mala', 401, 63), ('hmc', 3, 2100)])
def test_mcmc_native_stream_matches_oracle(dev, monkeypatch, kind, d, N):
    _against_oracle(H.native_matches_oracle, monkeypatch, kind, d, N, 160, 5, d + 1, seed=777 + d,
                    what='native %s d=%d N=%d' % (kind, d, N))


# ------------------------------------------------------------------------- 3. jump_mala and imh
@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('d,N', [(5, 300), (25, 1000), (51, 64)])
def test_jump_mala_native_stream_matches_oracle(dev, monkeypatch, fuse_tail, d, N):
    n, T = 192, 3
    p, lm = _record(d, N, n, 3 + d)
    q, flows = H.flow_inputs(p, d, n, centre=_flow_centre(p))
    H.jump_mala_matches_oracle(monkeypatch, q, T=T, Kin=4, seed=31337, h=0.3 * d ** (-1 / 3) / lm, imd=None, fuse_tail=fuse_tail,
                               spline=False, atol=ATOL, rtol=RTOL, share=0.95, jump_slack=max(2, int(0.03 * n * T)), margin=MARGIN,
                               skip_below_minus_50=SKIP, flows=flows)


@pytest.mark.parametrize('d,N,spline', [(3, 64, False), (25, 1000, False), (101, 65, False), (255, 40, False),
                                        (9, 300, True), (51, 63, True)])
def test_imh_runs_on_the_sequential_flow_mh_kernel(dev, monkeypatch, d, N, spline):
    """Affine and spline ('c-rqnsf') instantiations of the register flow-MH kernel for kind 7.  The flows are
    near the identity, so starts with a narrow spread give a useful share of accepted proposals."""
    p, _lm = _record(d, N, 256, 9 + d, spread=0.5)
    q, flows = H.flow_inputs(p, d, 256, 3 if spline else 9, spline=spline, centre=_flow_centre(p))
    H.imh_matches_oracle(monkeypatch, q, T=6, seed=4711 + d, flow_seed=3 if spline else 9, spline=spline, compare=_compare,
                         what='%s imh d=%d N=%d' % ('c-rqnsf' if spline else 'realnvp', d, N), margin=MARGIN,
                         skip_below_minus_50=SKIP, flows=flows)

# ------------------------------------------------------------------------- 3b. the flow-MH matrix
FLOW_DIMS = {4: 3, 8: 7, 16: 13, 32: 25, 64: 51, 128: 101, 256: 201, 512: 301}      # d = 2 D + 1
FLOW_SKIP_CAPS = (4, 8, 16, 32, 64, 128, 256, 512)    # some proposals are hopeless at every capacity: see the docstring
FLOW_CASES = H.flow_cases(FLOW_DIMS)
FLOW_TESTS = ('test_jump_mala_native_stream_matches_oracle', 'test_imh_runs_on_the_sequential_flow_mh_kernel',
              'test_flow_mh_matrix')
# the 120 KB LDS bound: two affine coupling layers of width 8 at the ragged capacity 512 are 132 KB by themselves, two
# spline layers of width 8 at capacity 64 are 111 KB and this kind's tile of X sits behind them
FLOW_REFUSED = {'mh-cap512-d301-h8', 'jump_mala-cap512-d301-h8', 'mh-cap64-d51-h8-spline', 'mh-cap64-d51-h8-cpl8-spline'}
FLOW_SHRINK = 0.3


@functools.lru_cache(maxsize=None)
def _flow_problem(d, N):
    """one object per distinct problem of the flow tests: the fit of the proposal's centre is kept per object"""
    return _record(d, N, 96, 9 + d, spread=0.5)


def _flow_centre(p):
    """The horseshoe's mode in the log scales is degenerate: the proposals sit about the mean of the file's starts, FLOW_SHRINK of
    the conditional standard deviations there"""
    return H.local_fit(p, FLOW_SHRINK, at='starts')


@pytest.mark.parametrize('case', FLOW_CASES, ids=H.flow_case_id)
def test_flow_mh_matrix(dev, monkeypatch, case):
    """H.flow_cases: every flow-MH layout, sibling, width and coupling, the unadjusted carry path and the jump tails, with
    decisions and log ratios compared row by row (H.compare_flow_mh).  The inner steps of the jump cases shrink with the
    proposal (FLOW_SHRINK^2 for MALA, FLOW_SHRINK for HMC), so that a chain is still inside it when the jump comes."""
    d = case.d
    p, lm = _flow_problem(d, (65, 300, 1000, 63)[int(math.log2(case.cap)) % 4])
    H.run_flow_case(dev, monkeypatch, p, case, margin=MARGIN, compare=_compare, atol=ATOL, rtol=RTOL,
                    h_mala=FLOW_SHRINK ** 2 * 0.3 * d ** (-1 / 3) / lm, h_hmc=FLOW_SHRINK * _step('hmc', d, lm),
                    refused=H.flow_case_id(case) in FLOW_REFUSED, centre=_flow_centre(p), skip_caps=FLOW_SKIP_CAPS)


# ------------------------------------------------------------------------- 4. fused equals split
@pytest.mark.parametrize('kind,d,N', [('mala', 51, 1000), ('hmc', 9, 200), ('mh', 25, 63), ('hmc', 101, 65)])
def test_fused_equals_split(dev, monkeypatch, kind, d, N):
    T = 6
    p, lm = _record(d, N, 200, 17 + d)
    H.fused_equals_split(monkeypatch, p, lambda target: _sampler(kind, d, target, T, _step(kind, d, lm), imd=_mh_scale(d, lm)), T,
                         seed=2024, atol=ATOL, rtol=RTOL, share=0.95)


# ------------------------------------------------------------------------- 5. NeuTra (VALU kernels)
@pytest.mark.parametrize('d,nh,N', [(3, 4, 1), (5, 8, 63), (9, 16, 64), (25, 32, 65), (51, 8, 1000), (129, 16, 100),
                                    (255, 4, 40), (511, 8, 30)])
def test_neutra_gradient_matches_fp64_autograd(dev, d, nh, N):
    """Against fp64 autograd through oracle/flow.py and the loops of SLRU64, at the starts.  Tolerance: relative 2e-4 of
    (1 + max |.|) per row."""
    p, _lm = _record(d, N, 130, 5 + d)
    H.neutra_gradient_matches_autograd(dev, p.pot, p.ref, p.x0, nh, 'd=%d H=%d N=%d' % (d, nh, N), flow_seed=3, bound=2e-4)


@pytest.mark.parametrize('d,nh,N', [(9, 8, 200), (51, 16, 300)])
def test_neutra_hmc_fused_matches_oracle(dev, monkeypatch, d, nh, N):
    p, lm = _record(d, N, 96, 61 + d)
    H.neutra_hmc_fused_matches_oracle(monkeypatch, p, _flow_pair(d, 9, n_hidden=nh), T=3, L=4, h=0.2 / math.sqrt(lm), seed=12,
                                      atol=1e-3, share=0.93, accept_slack=6)


def test_neutra_wide_conditioner_takes_the_split_path_and_matches_the_oracle(dev):
    d = 51
    p, lm = _record(d, 200, 96, 62)
    H.neutra_wide_takes_the_split_path(dev, p, _flow_pair(d, 9, n_hidden=64), T=3, L=4, h=0.2 / math.sqrt(lm), seed=12,
                                       atol=1e-3, share=0.93)


def test_dlmc_borrows_the_gradient_step_and_matches_the_oracle(dev, monkeypatch):
    from nfmc_amd.samplers import dlmc as mod
    from oracle import samplers as osamp
    d, N, n, T, seed = 9, 500, 128, 3, 4242
    pot, ref, target, x0 = _problem(d, N, n, 71)
    f, of = _flow_pair(d, 3)
    f.fit = lambda *a, **k: None
    nll = lambda x: 0.125 * torch.sum(x ** 2, dim=-1)   # noqa: E731
    calls = {'launch_flow_mh': 0, 'split_flow_mh': 0}

    def spy(name):
        fn = getattr(mod, name)

        def wrapped(*a, **k):
            calls[name] += 1
            return fn(*a, **k)
        monkeypatch.setattr(mod, name, wrapped)
    for name in list(calls):
        spy(name)
    s = mod.DLMC((d,), pot, nll, mod.DLMCKernel((d,), flow=f, step_size=0.05), mod.DLMCParameters(n_iterations=T))
    s.seed = seed
    out = s.sample(x0, show_progress=False)
    assert s.last_route == 'borrowed'                        # grad U by autograd, not nfmc_dlmc_step_f32
    assert calls == {'launch_flow_mh': T, 'split_flow_mh': 0}   # the MH step on the flow-MH kernel
    tr = osamp.dlmc_sample(x0, target, nll, of, T, 0.05, noise=osamp.PhiloxNoise(seed, dtype=torch.float64))
    got = out.samples.cpu().double().reshape(T, n, d)
    same = (got - tr.stacked()).abs().amax(dim=(0, 2)) < 1e-3
    assert same.float().mean() >= 0.95, float(same.float().mean())
    assert abs(out.statistics.n_accepted_trajectories - tr.n_accepted) <= 0.03 * n * T


# ------------------------------------------------------------------------- 6. device warmup against the fp64 controller
@pytest.mark.parametrize('kind,d,N,n,W,every', [('mala', 25, 300, 140, 12, 1), ('hmc', 25, 65, 150, 16, 2),
                                                ('mala', 101, 64, 70, 8, 1)])
def test_warmup_controller_transitions_and_handoff(dev, monkeypatch, kind, d, N, n, W, every):
    """As tests/test_gpu_warmup.py does for the other kinds."""
    p, lm = _record(d, N, n, 7 + d)
    H.warmup_matches_controller(monkeypatch, p, kind, W=W, T=6, L=4, every=every, h0=0.3 * _step(kind, d, lm), imd0=torch.ones(d),
                                seed=4242 + d, what='slr %s d=%d n=%d every=%d' % (kind, d, n, every), ties=0.05)


# ------------------------------------------------------------------------- 7. refused entry points, bad descriptors
def test_refusing_entry_points_answer_unsupported(dev):
    from nfmc_amd import hip
    d, N = 51, 300
    pot, _ref, _t, x0 = _problem(d, N, 256, 4)
    pd = pot.descriptor(dev)
    assert pd.kind == hip.POT_SPARSE_LOGISTIC_REGRESSION and pd.n_components == N
    H.refusing_entry_points(dev, pot, x0, functools.partial(_flow_pair, d))


def test_philox7_and_bad_descriptors_are_refused(dev):
    """A NULL X or y, N < 1, a misaligned X, an even d, and a or b not positive and finite are argument errors."""
    from nfmc_amd import hip
    d = 25
    pot, _ref, _t, x0 = _problem(d, 100, 128, 8)
    bad = [('a', 0), ('b', 0), ('n_components', 0), ('n_components', -1), ('a', 'misaligned'), ('a_scalar', 0.0), ('a_scalar', -1.0),
           ('a_scalar', float('inf')), ('b_scalar', 0.0), ('b_scalar', float('nan'))]
    H.bad_descriptors_are_refused(dev, pot, x0, _flow_pair(d)[0], [(f, v, hip.EINVAL) for f, v in bad])
    x = x0.to(dev)
    a = H.mala_args(dev, pot, x)
    a.d = d - 1                                                                     # an even d
    assert int(hip.lib().nfmc_mala_steps_f32(C.byref(a), hip.stream())) == hip.EINVAL
    torch.cuda.synchronize()
    assert torch.equal(x, x0.to(dev))


# ------------------------------------------------------------------------- 8. determinism and sharding
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
def test_determinism_and_sharding(dev, kind):
    d, T = 21, 8
    p, lm = _record(d, 700, 300, 44)
    H.determinism_and_sharding(lambda: _sampler(kind, d, p.pot, T, _step(kind, d, lm)), p.x0, T, d, seed=7, world=2)


@pytest.mark.parametrize('kind', ['mala', 'mh', 'hmc'])
def test_overflowing_proposals_are_rejected_and_counted(dev, kind):
    """Steps far past stability: proposals reach scales whose exponentials (e^{s + l_j}, e^{l_j}, e^s) or logits z
    overflow fp32, so U of the proposal is inf or NaN and the log ratio is not finite.  The adjusted kernels reject every
    such proposal and count it as non-finite (n_nonfinite_log_ratios), as for the existing kinds; the kept states stay
    finite."""
    d, N, n, T = 15, 100, 512, 10
    pot, ref, _t, x0 = _problem(d, N, n, 3)
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


# ------------------------------------------------------------------------- 9. correctness without an oracle
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
def test_prior_stays_stationary(dev, monkeypatch, kind):
    """X = 0: the data term is the constant N log 2, so the posterior is the prior.  65536 chains start at exact prior
    draws (a = b = 2, light tails) and run a few hundred fused transitions.  A kernel that leaves the target invariant
    keeps them there however well it mixes: the mean and the variance of every w_j, l_j and s still match (0, 1) for w_j
    and (digamma(a) - log b, trigamma(a)) for l_j and s, within 5 standard errors (the variance's from the fourth sample
    moment)."""
    from nfmc_amd.potentials import SparseLogisticRegression
    D, N, n, a, b = 12, 7, 65536, 2.0, 2.0
    d = 2 * D + 1
    pot = SparseLogisticRegression(torch.zeros(N, D), torch.arange(N) % 2, scale_shape=a, scale_rate=b)
    x0 = prior_draws(D, n, a, b, 2024).float()
    T = 300
    h = 0.15 if kind == 'mala' else 0.12
    s = _sampler(kind, d, pot, T, h, L=8)
    s.params.store_samples = False
    s.seed = 31
    spy = _Spy(monkeypatch)
    out = s.sample(x0, show_progress=False)
    assert not spy.calls
    acc = out.statistics.n_accepted_trajectories / (n * T)
    print(kind, 'acceptance', acc)
    assert 0.5 < acc < 1.0, acc
    x = out.running_samples.last_sample.cpu().double()
    assert x.shape == (n, d) and bool(torch.isfinite(x).all())
    assert not torch.equal(x, x0.double())
    lm, lv = log_gamma_moments(a, b)
    mean_t = torch.tensor([0.0 if c % 2 == 0 and c < 2 * D else lm for c in range(d)], dtype=torch.float64)
    var_t = torch.tensor([1.0 if c % 2 == 0 and c < 2 * D else lv for c in range(d)], dtype=torch.float64)
    m = x.mean(0)
    v = x.var(0)
    m4 = ((x - m) ** 4).mean(0)
    z_m = (m - mean_t) / torch.sqrt(v / n)
    z_v = (v - var_t) / torch.sqrt((m4 - v * v) / n)
    print(kind, 'z of the means', [round(t, 2) for t in z_m.tolist()])
    print(kind, 'z of the variances', [round(t, 2) for t in z_v.tolist()])
    assert bool((z_m.abs() < 5).all()), z_m.tolist()
    assert bool((z_v.abs() < 5).all()), z_v.tolist()


def test_sample_jump_mala_recovers_the_sparse_signal(dev):
    """End to end: sample(..., strategy='jump_mala') on N = 1000 simulated rows, D = 25 standardised features, three
    nonzero coefficients.  Posterior means of beta (over chains and the second half of the kept states): every nonzero
    coefficient keeps its sign and lies more than 3 posterior standard deviations from 0; every null one lies within 4
    posterior standard deviations of 0, and closer to 0 than the smallest nonzero one."""
    from nfmc_amd import sample
    from nfmc_amd.potentials import SparseLogisticRegression
    N, D, n = 1000, 25, 4096
    d = 2 * D + 1
    X, y, beta_true = synthetic(N, D, 2025)
    pot, ref = SparseLogisticRegression(X, y), SLRU64(X, y)
    x0 = start_states(D, n, 2026, spread=0.5).float()
    h = 0.3 * d ** (-1 / 3) / _lmax(ref, x0[:256])
    out = sample(pot, flow='realnvp', strategy='jump_mala', n_iterations=40, n_chains=n, x0=x0, show_progress=False,
                 seed=3, inner_kernel_kwargs={'step_size': h}, inner_param_kwargs={'n_iterations': 10})
    kept = out.samples.reshape(-1, n, d)
    assert torch.isfinite(kept).all()
    kept = kept[kept.shape[0] // 2:].reshape(-1, d).double()
    beta = pot.constrain(kept)[3]
    mean, sd = beta.mean(0), beta.std(0)
    nz = beta_true != 0
    print('true', beta_true[nz].tolist(), 'mean', mean[nz].tolist(), 'sd', sd[nz].tolist())
    print('null |mean| / sd max', float((mean[~nz].abs() / sd[~nz]).max()))
    assert bool((torch.sign(mean[nz]) == torch.sign(beta_true[nz])).all())
    assert bool((mean[nz].abs() > 3 * sd[nz]).all())
    assert bool((mean[~nz].abs() < 4 * sd[~nz]).all())
    assert float(mean[~nz].abs().max()) < float(mean[nz].abs().min())
