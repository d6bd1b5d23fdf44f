"""GPU: DiffusionBridge (NFMC_POT_DIFFUSION_BRIDGE) on the fused HIP kernels against the fp64 CPU oracle, with the target
restated in fp64 as a loop over t (tests/diffusion_fp64.py).  Section by section the GMRF file (tests/test_gpu_gmrf.py).

Problems (diffusion_fp64.problem_data): a series simulated from the model itself, about a third of the entries not
observed (seeded), for six models: the Lorenz-63 bridge at the Inference Gym's values (m = 3, dt = 0.02, sigma = 0.1, so
om = 1 / (sigma^2 dt) = 5000), the double well (cubic, m = 1 and m = 3), FitzHugh-Nagumo (m = 2), an Ornstein-Uhlenbeck
pair (m = 2) and Brownian motion (m = 1); each with fixed scales and with unknown ones under the LogNormal(-1, 0.25)
prior.  Starts are `prior_draws`, rounded to fp32; the two largest shapes start about the generating path
(diffusion_fp64.starts_near_truth), where a prior draw of 1022 steps sits at U = 1e6.

Step sizes, lambda = the largest entry of the Hessian's diagonal over the starts (diffusion_fp64.step_lambda, closed
form): mala 0.5 d^(-1/3) / lambda, ula 0.1 d^(-1/3) / lambda, mh proposal scale 0.5 / sqrt(d lambda), hmc
0.5 d^(-1/4) / sqrt(lambda) with L = 5, uhmc 0.3 d^(-1/4) / sqrt(lambda): the stochastic-volatility file's rule.

Tolerances are the GMRF and stochastic-volatility files': MARGIN 2e-3, ATOL 1e-3 + RTOL 1e-4, the harness's 10 % cap on
near-ties, and H.compare_decisions with its 8 ulp(fp32) `mag` term.  mag(x) = |U(x)| + sum_i |x_i dU/dx_i (x)| from the
fp64 oracle: the kernel's state is an fp32 rounding of the oracle's, every coordinate half an ulp off, and with om = 5000
and |X| up to 20 on the Lorenz attractor that rounding alone moves U by 1e-7 sum_i |x_i dU/dx_i|, far more than 8 ulp of
|U| (U is a sum of small squares of differences of large numbers).  The stochastic-volatility file adds its cancelling
terms to mag for the same reason.

The sizes: T = 2 (every step first and last: d = 2, 4, 6, 8), m = 3 at T = 8 and 21 (d = 24, 26, 63, 65: a step's
components straddle quads and lanes), and one size per default layout up to d = 1023 (m = 3, T = 341) and d = 1024
(m = 1, T = 1022, unknown scales).

With these inputs the fp64 oracle alone (the replay grid, 96 chains, 4 transitions; mala, mh and hmc) accepts 0.73 to 1.0 of
the proposals, keeps every log ratio finite and puts at most 2.1 % of the chains of a run within 2e-3 of a tie (at most
5.2 % within the widened margin of the Lorenz cases: _margin).

Flow-proposal cases (sections 3a and 3b).  Neighbouring steps are tied with the precision om, so no independent proposal
at the marginal scales of a Laplace fit is ever accepted (fp64 log ratios down to -5e4 at d = 6): the proposals sit about
the mean of starts near the generating path, 0.3 of the conditional standard deviations there (_flow_centre), and the
inner steps of the jumps shrink with them, as in the stochastic-volatility file.  The fp64 oracle alone then accepts 0.016
to 0.205 of the jumps and 0.193 to 0.468 of the IMH proposals of section 3a and 0.016 to 0.565 in the matrix, with at most
2.1 % of the chains of a case within MARGIN of a tie.  Some proposals are hopeless (fp64 log ratios down to -119 in the
matrix): every case sets skip_below_minus_50.  Their log-ratio tolerance carries two more terms from the oracle alone
(_sensitive): the flow's own fp32 error at the case's proposals, 4 x the measured figure as H.spline_c has it for the
spline cases (5.4e-4 at the Lorenz d = 24 case, under 1e-4 elsewhere), and what the fp32 rounding of the states does to U
(H.u_sensitivity_of's form) and, for the jumps, the same measured figure of log q at the jump's start (_logq_figure).
"""
import functools
import math

import pytest
import torch

import target_harness as H
from diffusion_fp64 import COMBOS, fp32_figure, make_pair, problem_data, shape_of, starts_near_truth, step_lambda
from target_harness import Spy as _Spy, flow_pair as _flow_pair

pytestmark = pytest.mark.gpu

MARGIN = 2e-3
ATOL, RTOL = 1e-3, 1e-4


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


class _Built:
    """What the harness takes (pot, ref, target, x0, d, name) with the problem's data and lambda."""

    def __init__(self, d, model, m, unknown, seed, n, x0_seed, event_shape, near_truth):
        self.data = problem_data(shape_of(d, m, unknown), m, model, seed, unknown)
        self.pot, self.ref = make_pair(self.data, event_shape)
        self.target = self.ref
        x0 = starts_near_truth(self.data, self.pot, n, x0_seed) if near_truth else self.pot.prior_draws(n, x0_seed)
        self.x0 = x0.float()
        self.d, self.model, self.m, self.unknown = d, model, m, unknown
        self.name = '%s m=%d %s d=%d' % (model, m, 'unknown' if unknown else 'fixed', d)
        self.lam = step_lambda(self.ref, self.x0)


@functools.lru_cache(maxsize=None)
def _Problem(d, model, m, unknown, seed, n, x0_seed, event_shape=None, near_truth=False):
    """One object per distinct problem, shared by the tests that use it and left unchanged."""
    return _Built(d, model, m, unknown, seed, n, x0_seed, event_shape, near_truth)


FP32_FACTOR = 4.0      # the SPLINE_C_FACTOR precedent: see _margin


def _margin(p, tr):
    """The near-tie margin of a run: MARGIN, or FP32_FACTOR times the worst |U(fp32(x)) - U(x)| of the fp64 oracle over the
    starts and the oracle's own kept states (diffusion_fp64.fp32_figure) where that is larger.  The kernels keep the state
    in fp32.  With om = 5000 and |X| up to 50 on the Lorenz attractor, U is a sum of T m terms om e^2 / 2 ~ 1 whose
    e = X_t - X_{t-1} - dt f, about 0.014, carries the rounding of X, ulp(48) = 3.8e-6: up to 3e-4 per term, which no
    evaluation from an fp32 state can avoid.  Measured on the CPU at this file's inputs (the figure, not 4 x it): under
    2.3e-4 for every model but the Lorenz bridge, whose replay cases give 1.2e-3 (d = 63), 1.1e-2 (d = 65, unknown
    scales, prior draws at U = 1e3), 2.7e-3 (d = 252) and 5.2e-3 (d = 1023); the fp64 oracle alone then has at most
    5.2 % of the chains of a case inside the margin (mala, d = 252), elsewhere at most 3.1 %."""
    states = torch.cat([p.x0.double()[None], tr.stacked().double()])
    return max(MARGIN, FP32_FACTOR * fp32_figure(p.ref, states))


def _compare_for(p):
    def compare(got, tr, what):
        margin = _margin(p, tr)
        if margin > MARGIN:
            print('%s: near-tie margin %.2e' % (what, margin))
        return H.compare_states(got, tr, what, margin=margin, atol=ATOL, rtol=RTOL)
    return compare


_sampler = functools.partial(H.mcmc_sampler, imd_kinds=('mh',))      # Langevin and HMC keep the unit mass diagonal
_oracle = functools.partial(H.oracle_trace, imd_kinds=('mh',))


def _mag(ref, x):
    """|U(x)| + sum_i |x_i dU/dx_i (x)|: see the docstring"""
    x = x.double()
    return ref(x).abs() + (x * ref.grad(x)).abs().sum(1)


def _compare_decisions(rec, tr, kind, x0, ref, what):
    H.compare_decisions(rec, tr, kind, x0, ref, what, mag=functools.partial(_mag, ref))


def _mh_scale(p):
    return torch.full((p.d,), 0.5 / math.sqrt(p.d * p.lam), dtype=torch.float64)


def _step(kind, p):
    if kind in ('hmc', 'uhmc'):
        return {'hmc': 0.5, 'uhmc': 0.3}[kind] * p.d ** (-1 / 4) / math.sqrt(p.lam)
    return {'mala': 0.5, 'ula': 0.1, 'mh': 0.0}[kind] * p.d ** (-1 / 3) / p.lam


def _against_oracle(check, monkeypatch, kind, p, T, event_shape=None, **kw):
    h, imd = _step(kind, p), _mh_scale(p)
    shape = p.d if event_shape is None else event_shape
    check(monkeypatch, p, kind, T, _sampler(kind, shape, p.pot, T, h, imd=imd),
          lambda noise: _oracle(kind, p.x0, p.target, T, h, noise, imd=imd, label=p.name), compare=_compare_for(p),
          decisions=_compare_decisions, **({} if event_shape is None else {'event_shape': event_shape}), **kw)


KINDS = list(H.KINDS)
# (d, model, m, unknown): T = 2 at every m and with scales; m = 3 at T = 8 and 21; then one size per default layout
SHAPES = [(2, 'cubic', 1, False), (4, 'fitzhugh_nagumo', 2, False), (6, 'lorenz63', 3, False), (8, 'lorenz63', 3, True),
          (4, 'brownian', 1, True), (24, 'lorenz63', 3, False), (26, 'cubic', 3, True), (63, 'lorenz63', 3, False),
          (65, 'lorenz63', 3, True), (14, 'fitzhugh_nagumo', 2, True), (100, 'ou', 2, False), (130, 'cubic', 1, True),
          (252, 'lorenz63', 3, False), (500, 'fitzhugh_nagumo', 2, False)]
BIG = [(1023, 'lorenz63', 3, False), (1024, 'brownian', 1, True)]


def _id(s):
    return '%s-m%d-%s-d%d' % (s[1], s[2], 'unknown' if s[3] else 'fixed', s[0])


# ------------------------------------------------------------------------- 1. fused kernels vs fp64 oracle, replayed noise
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=_id)
def test_mcmc_replay_matches_oracle(dev, monkeypatch, kind, shape):
    d, model, m, unknown = shape
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, _Problem(d, model, m, unknown, 10 * d + 1, 96, d + 2), 4,
                    torch_seed=d, what='%s %s' % (kind, _id(shape)))


@pytest.mark.parametrize('kind', ['mala', 'hmc'])
@pytest.mark.parametrize('shape', BIG, ids=_id)
def test_the_largest_shapes(dev, monkeypatch, kind, shape):
    """d = 1023 (m = 3, T = 341) and d = 1024 (m = 1, T = 1022, unknown scales): the layout (16, 64), four register quads
    per lane and the lane wrap; 32 chains x 2 transitions."""
    d, model, m, unknown = shape
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, _Problem(d, model, m, unknown, 5, 32, 7, near_truth=True), 2,
                    torch_seed=d,
                    what='%s %s' % (kind, _id(shape)))


@pytest.mark.parametrize('kind,model,shape', [('mala', 'lorenz63', (7, 3)), ('hmc', 'fitzhugh_nagumo', (16, 2))])
def test_two_dimensional_event_shape(dev, monkeypatch, kind, model, shape):
    """A (T, m) path through event_shape=: the kernels see the flattened d = T m."""
    d = shape[0] * shape[1]
    p = _Problem(d, model, shape[1], False, 77, 96, 5, event_shape=shape)
    assert p.pot.event_shape == shape
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, p, 4, event_shape=shape, torch_seed=d,
                    what='%s %s %s' % (kind, shape, model))


# ------------------------------------------------------------------------- 2. every drift, fixed and unknown scales
@pytest.mark.parametrize('unknown', [False, True])
@pytest.mark.parametrize('model,m', COMBOS)
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
def test_every_drift_and_scale_mode(dev, monkeypatch, kind, model, m, unknown):
    d = 10 * m + (2 if unknown else 0)
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, _Problem(d, model, m, unknown, 3 * d + 1, 96, d + 2), 4,
                    torch_seed=d, what='%s %s m=%d %s' % (kind, model, m, unknown))


# ------------------------------------------------------------------------- 3. native Philox streams
@pytest.mark.parametrize('kind,shape', [('mala', (24, 'lorenz63', 3, False)), ('ula', (8, 'lorenz63', 3, True)),
                                        ('mh', (130, 'cubic', 1, True)), ('hmc', (65, 'lorenz63', 3, True)),
                                        ('uhmc', (4, 'fitzhugh_nagumo', 2, False)), ('hmc', (500, 'fitzhugh_nagumo', 2, False))],
                         ids=lambda v: v if isinstance(v, str) else _id(v))
def test_mcmc_native_stream_matches_oracle(dev, monkeypatch, kind, shape):
    d, model, m, unknown = shape
    _against_oracle(H.native_matches_oracle, monkeypatch, kind, _Problem(d, model, m, unknown, 7 * d + 3, 160, d), 5,
                    seed=777 + d, what='native %s %s' % (kind, _id(shape)))


# ------------------------------------------------------------------------- 3a. jump, imh
FLOW_SHRINK = 0.3
SKIP = True     # skip_below_minus_50 of the flow-MH cases: an independent proposal of a whole path is at times hopeless
                # (fp64 log ratios down to -119 in the matrix): as in tests/test_gpu_sv.py


@functools.lru_cache(maxsize=None)
def _flow_problem(d, model, m, unknown, n=96):
    """one object per distinct problem of the flow tests, started about the generating path: the fit of the proposal's
    centre is kept per object (H.laplace_fit / H.local_fit)"""
    return _Problem(d, model, m, unknown, 5 * d + 7, n, 9, near_truth=True)


def _flow_centre(p):
    """Neighbouring steps of a path are tied to each other with the precision om (5000 for the Lorenz bridge), so the
    marginal scales of a Laplace fit give an independent proposal no chance (the fp64 oracle alone: log ratios down to
    -5e4 at d = 6), and with unknown scales the joint mode sits far down in log sigma.  The proposals sit about the mean of
    the starts instead, FLOW_SHRINK of the conditional standard deviations there (the stochastic-volatility file's
    choice)."""
    return H.local_fit(p, FLOW_SHRINK, at='starts')


def _flow_steps(p):
    """inner steps of the jump cases: they shrink with the proposal (tests/test_gpu_sv.py)"""
    return FLOW_SHRINK ** 2 * 0.3 * p.d ** (-1 / 3) / p.lam, FLOW_SHRINK * _step('hmc', p)


def _state_sensitivity(steps, target):
    """(T, n): H.u_sensitivity_of at the proposals x' plus the same 4 ulp(fp32) sum_i |x_i dU/dx_i| at the states x the
    transitions start from: the kernel's x is an fp32 state too (an accepted fp32 proposal, or the end of fp32 inner
    transitions), and the U(x) it carries was formed there."""
    at_x = []
    for js in steps:
        x = js.x.detach().clone().requires_grad_(True)
        u = target(x)
        g, = torch.autograd.grad(torch.where(torch.isfinite(u), u, torch.zeros_like(u)).sum(), x)
        at_x.append(4 * 2.0 ** -24 * (g.abs() * x.detach().abs()).sum(1))
    return H.u_sensitivity_of(steps, target) + torch.stack(at_x)


def _logq_figure(steps, of):
    """The worst |log q_fp32(fp32(x)) - log q(x)| at the states x a JUMP starts from: the oracle flow cast to fp32 on the
    CPU, at the state rounded to fp32, against itself in fp64.  After the inner transitions the kernel's x is no proposal
    whose log q is carried: log q(x) is formed by the flow's forward pass at an fp32 state, and with proposal scales of
    0.003 about |X| up to 20 that pass maps x to 330 x - 6600.  H.spline_c measures the same at the proposals x' only.
    Measured at the jump cases of section 3a: 1.8e-4 (Lorenz, d = 6), 2.3e-5 (cubic, d = 26), 5.1e-5 (OU, d = 64); the
    first-order bound 4 ulp sum_i |x_i d log q / dx_i| gives 9.6e-4, 2.0e-4 and 2.7e-4 there, the same size as 4 x these."""
    import copy
    f32 = copy.deepcopy(of).float()
    worst = 0.0
    with torch.no_grad():
        for js in steps:
            x = js.x.reshape(js.x.shape[0], *of.event_shape)
            diff = (f32.log_prob(x.float()).double() - of.log_prob(x)).abs()
            worst = max(worst, float(diff[torch.isfinite(diff)].max()))
    return worst


def _sensitive(monkeypatch, p, of, jump=False):
    """Hands every H.compare_flow_mh of the test two terms that come from the fp64 oracle alone.
    u_sensitivity = _state_sensitivity: the proposal is an fp32 flow image, each coordinate a few roundings off, and
    dU/dX = om e is 70 per coordinate for the Lorenz bridge (om = 5000): 1e-3 of U per coordinate where |X| = 20, which the
    magnitudes of H.flow_mh_tolerance do not see.  The particles file passes the harness's term for its r^-12 potential.
    For a jump (jump=True) FP32_FACTOR times _logq_figure is added to c: the same measurement at the jump's start x.
    Every flow test of this file calls this first, so the tolerance of H.run_flow_case, H.jump_mala_matches_oracle and
    H.imh_matches_oracle here is the harness's own plus these terms, never less; the files the tolerances come from
    (tests/test_gpu_sv.py, tests/test_gpu_gmrf.py) run the helpers unpatched.
    c = H.spline_c for the affine flows too: the proposals sit 0.3 conditional standard deviations (0.003) about a path
    with |X| up to 20, so the flow's first layer maps x to 330 x - 6600 and fp32 loses three digits of log q there; the
    oracle flow cast to fp32 against itself in fp64 at the case's proposals gives 5.4e-4 at the Lorenz d = 24 case and
    9.2e-5 at d = 6 (under 1e-4 for the other models), and SPLINE_C_FACTOR = 4 times that, never less than affine_c,
    is the flow's part of the tolerance as it is for every file's spline cases."""
    orig = H.compare_flow_mh

    def compare_flow_mh(got_m, got_lr, steps, what, **kw):
        if kw.get('u_sensitivity') is None:
            kw['u_sensitivity'] = _state_sensitivity(steps, p.target)
        kw['c'] = max(kw['c'], H.spline_c(p.d, of, steps)[0])
        if jump:
            kw['c'] = kw['c'] + FP32_FACTOR * _logq_figure(steps, of)
        return orig(got_m, got_lr, steps, what, **kw)
    monkeypatch.setattr(H, 'compare_flow_mh', compare_flow_mh)


def _flow_compare_for(p):
    """H.compare_states with the near-tie margin widened by the largest u_sensitivity of the run (see _sensitive): a
    decision the kernel may not know is no decision to follow."""
    def compare(got, tr, what):
        steps = getattr(tr, 'flow_steps', None)
        sens = float(_state_sensitivity(steps, p.target).max()) if steps else 0.0
        return H.compare_states(got, tr, what, margin=MARGIN + sens, atol=ATOL, rtol=RTOL)
    return compare


@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('shape', [(6, 'lorenz63', 3, False), (26, 'cubic', 3, True), (64, 'ou', 2, False)], ids=_id)
def test_jump_mala_native_stream_matches_oracle(dev, monkeypatch, fuse_tail, shape):
    d, model, m, unknown = shape
    n, T = 192, 3
    p = _flow_problem(d, model, m, unknown, n)
    q, flows = H.flow_inputs(p, d, n, from_d=0, centre=_flow_centre(p))      # a centred flow at every d
    _sensitive(monkeypatch, p, flows[1], jump=True)
    H.jump_mala_matches_oracle(monkeypatch, q, T=T, Kin=4, seed=31337, h=_flow_steps(p)[0], imd=None, fuse_tail=fuse_tail,
                               spline=False, atol=ATOL, rtol=RTOL, share=0.95, jump_slack=max(2, int(0.03 * n * T)),
                               margin=MARGIN, skip_below_minus_50=SKIP, flows=flows)


@pytest.mark.parametrize('shape,spline', [((4, 'fitzhugh_nagumo', 2, False), False), ((24, 'lorenz63', 3, False), False),
                                          ((130, 'cubic', 1, True), False), ((252, 'cubic', 3, False), False),
                                          ((6, 'lorenz63', 3, False), True), ((34, 'fitzhugh_nagumo', 2, True), True)],
                         ids=lambda v: ('spline' if v else 'affine') if isinstance(v, bool) else _id(v))
def test_imh_runs_on_the_sequential_flow_mh_kernel(dev, monkeypatch, shape, spline):
    """Affine and spline ('c-rqnsf') instantiations of the register flow-MH kernel for kind 14."""
    d, model, m, unknown = shape
    p = _flow_problem(d, model, m, unknown, 256)
    q, flows = H.flow_inputs(p, d, 256, 3 if spline else 9, spline=spline, from_d=0, centre=_flow_centre(p))
    _sensitive(monkeypatch, p, flows[1])
    H.imh_matches_oracle(monkeypatch, q, T=6, seed=4711 + d, flow_seed=3 if spline else 9, spline=spline,
                         compare=_flow_compare_for(p), what='%s imh %s' % ('c-rqnsf' if spline else 'realnvp', _id(shape)), margin=MARGIN,
                         skip_below_minus_50=SKIP, flows=flows)


# ------------------------------------------------------------------------- 3b. the flow-MH matrix
# capacity -> the problem in it: d = T m (+ 2) is ragged in every capacity but 4 (T >= 2 leaves d = 2, 3, 4 there)
# (the Lorenz bridge at the small capacities only: at d = 300 the fp32 proposal alone moves its U by up to 0.08, see
# _sensitive; its long paths are section 1's)
FLOW_SHAPES = {4: (3, 'cubic', 1, False), 8: (6, 'lorenz63', 3, False), 16: (14, 'fitzhugh_nagumo', 2, True),
               32: (26, 'lorenz63', 3, True), 64: (50, 'ou', 2, False), 128: (101, 'cubic', 3, True),
               256: (200, 'fitzhugh_nagumo', 2, False), 512: (300, 'cubic', 3, False)}
FLOW_CASES = H.flow_cases({cap: s[0] for cap, s in FLOW_SHAPES.items()})
FLOW_TESTS = ('test_jump_mala_native_stream_matches_oracle', 'test_imh_runs_on_the_sequential_flow_mh_kernel',
              'test_flow_mh_matrix')
# the 120 KB LDS bound: two affine coupling layers of width 8 at the ragged capacity 512 are 132 KB by themselves
FLOW_REFUSED = {'mh-cap512-d300-h8', 'jump_mala-cap512-d300-h8'}
FLOW_SKIP_CAPS = (4, 8, 16, 32, 64, 128, 256, 512)    # some proposals are hopeless at every capacity: see SKIP


@pytest.mark.parametrize('case', FLOW_CASES, ids=H.flow_case_id)
def test_flow_mh_matrix(dev, monkeypatch, case):
    """H.flow_cases: every flow-MH layout, sibling, width and coupling, the unadjusted carry path and the jump tails, with
    decisions and log ratios compared row by row (H.compare_flow_mh, with the oracle-derived terms of _sensitive added to
    its tolerance)"""
    p = _flow_problem(*FLOW_SHAPES[case.cap])
    h_mala, h_hmc = _flow_steps(p)
    of = H.centred_flow_pair(p, 5, case.n_hidden, case.spline, case.n_layers, scale=H.flow_case_scale(case),
                             centre=_flow_centre(p))[1]           # the pair run_flow_case builds: nothing is drawn
    _sensitive(monkeypatch, p, of, jump=case.family.startswith('jump'))
    H.run_flow_case(dev, monkeypatch, p, case, margin=MARGIN, atol=ATOL, rtol=RTOL, h_mala=h_mala, h_hmc=h_hmc,
                    compare=_flow_compare_for(p), refused=H.flow_case_id(case) in FLOW_REFUSED, centre=_flow_centre(p), skip_caps=FLOW_SKIP_CAPS)


@pytest.mark.parametrize('cap', [64, 128, 256])
def test_flowb_override_launches_what_more_than_4096_chains_get(dev, monkeypatch, cap):
    """a staged kind (its exchange rows sit behind the flow image)"""
    p = _flow_problem(*FLOW_SHAPES[cap])
    f, _of = H.centred_flow_pair(p, 5, 8, scale=0.2 if p.d < 200 else 0.05, centre=_flow_centre(p))
    H.flowb_override_equals_production(dev, monkeypatch, H.centred(p, 4160, 6, _flow_centre(p)), f, lpc=cap // 8, T=3, seed=99)


# ------------------------------------------------------------------------- 4. fused equals split
@pytest.mark.parametrize('kind,shape', [('mala', (26, 'cubic', 3, True)), ('hmc', (9, 'lorenz63', 3, False)),
                                        ('mh', (64, 'ou', 2, False))], ids=lambda v: v if isinstance(v, str) else _id(v))
def test_fused_equals_split(dev, monkeypatch, kind, shape):
    """The object runs fused (no split-path transition, and the fused launch is seen to happen), the same object behind
    a plain lambda takes the split path for every transition; both agree."""
    d, model, m, unknown = shape
    T = 6
    p = _Problem(d, model, m, unknown, 17 * d, 200, 17)
    launches = []

    def make(target):
        s = _sampler(kind, d, target, T, _step(kind, p), imd=_mh_scale(p))
        cls = type(s)
        orig = cls._launch
        monkeypatch.setattr(cls, '_launch', lambda self, *a, **k: launches.append(target is p.pot) or orig(self, *a, **k))
        return s
    H.fused_equals_split(monkeypatch, p, make, T, seed=2024, atol=ATOL, rtol=RTOL, share=0.95)
    assert launches and all(launches), launches      # fused launches happened, and only for the potential object


# ------------------------------------------------------------------------- 5. NeuTra (VALU kernels)
@pytest.mark.parametrize('unknown', [False, True])
@pytest.mark.parametrize('n_steps,m,nh', [(2, 1, 4), (2, 2, 8), (3, 3, 16), (8, 3, 32), (32, 2, 8), (21, 3, 32), (64, 2, 16),
                                          (43, 3, 8), (256, 1, 4)])
def test_neutra_gradient_matches_fp64_autograd(dev, n_steps, m, nh, unknown):
    """On a perturbed RealNVP; the model rotates with the shape.  T m = 64 and 128 are the shapes the matrix-core kernels
    would take for the other kinds.  Tolerance: relative 2e-4 of (1 + max |.|) per row."""
    model = {1: ('cubic', 'brownian'), 2: ('fitzhugh_nagumo', 'ou'), 3: ('lorenz63', 'cubic')}[m][(n_steps + nh) % 2]
    d = n_steps * m + (2 if unknown else 0)
    p = _Problem(d, model, m, unknown, 11 * d + nh, 130, d)
    H.neutra_gradient_matches_autograd(dev, p.pot, p.ref, p.x0, nh, '%s d=%d H=%d' % (p.name, d, nh), flow_seed=3, bound=2e-4)


@pytest.mark.parametrize('shape,nh', [((8, 'lorenz63', 3, True), 8), ((64, 'fitzhugh_nagumo', 2, False), 16),
                                      ((128, 'cubic', 1, False), 8)], ids=lambda v: str(v) if isinstance(v, int) else _id(v))
def test_neutra_hmc_fused_matches_oracle(dev, monkeypatch, shape, nh):
    d, model, m, unknown = shape
    p = _Problem(d, model, m, unknown, 13 * d, 96, 61)
    H.neutra_hmc_fused_matches_oracle(monkeypatch, p, _flow_pair(d, 9, n_hidden=nh), T=3, L=4, h=0.2 / math.sqrt(p.lam),
                                      seed=12, atol=1e-3, share=0.93, accept_slack=6)


def test_neutra_wide_conditioner_takes_the_split_path_and_matches_the_oracle(dev):
    d = 64
    p = _Problem(d, 'ou', 2, False, 29, 96, 62)
    H.neutra_wide_takes_the_split_path(dev, p, _flow_pair(d, 9, n_hidden=64), T=3, L=4, h=0.2 / math.sqrt(p.lam), seed=12,
                                       atol=1e-3, share=0.93)


# ------------------------------------------------------------------------- 6. device warmup against the fp64 controller
@pytest.mark.parametrize('kind,shape,n,W,every', [('mala', (24, 'lorenz63', 3, False), 140, 12, 1),
                                                  ('hmc', (26, 'cubic', 3, True), 150, 16, 2),
                                                  ('mala', (130, 'cubic', 1, True), 70, 8, 1)],
                         ids=lambda v: str(v) if not isinstance(v, tuple) else _id(v))
def test_warmup_controller_transitions_and_handoff(dev, monkeypatch, kind, shape, n, W, every):
    """As tests/test_gpu_warmup.py does for the other kinds."""
    d, model, m, unknown = shape
    p = _Problem(d, model, m, unknown, 7 + d, n, 7)
    H.warmup_matches_controller(monkeypatch, p, kind, W=W, T=6, L=4, every=every, h0=0.3 * _step(kind, p), imd0=torch.ones(d),
                                seed=4242 + d, what='diffusion %s %s n=%d every=%d' % (kind, _id(shape), n, every), ties=0.05)


# ------------------------------------------------------------------------- 7. refused entry points, bad descriptors
@pytest.mark.parametrize('unknown', [False, True])
def test_refusing_entry_points_answer_unsupported(dev, unknown):
    from nfmc_amd import hip
    d = 63 + (2 if unknown else 0)
    p = _Problem(d, 'lorenz63', 3, unknown, 4, 256, 4)
    pd = p.pot.descriptor(dev)
    assert pd.kind == hip.POT_DIFFUSION_BRIDGE == 14 and pd.n_components == 21
    assert pd.a_scalar == (22.0 if unknown else 18.0)
    H.refusing_entry_points(dev, p.pot, p.x0, functools.partial(_flow_pair, d))
    H.fit_step_refuses(dev, p.pot, p.x0, _flow_pair(d)[0])
    H.limits_are_unchanged()


def test_philox7_and_bad_descriptors_are_refused(dev):
    """A NULL header or rows, T < 2, an invalid code, an m that does not fit the drift and d != T m + 2 [unknown] are
    argument errors; a misaligned header or rows is an alignment error."""
    from nfmc_amd import hip
    d = 26                                                       # cubic, m = 3, T = 8, unknown scales: code 0 + 4 + 16
    p = _Problem(d, 'cubic', 3, True, 8, 128, 8)
    b = p.pot.descriptor(dev).b
    assert p.pot.descriptor(dev).a_scalar == 20.0
    bad = [('a', 0, hip.EINVAL), ('b', 0, hip.EINVAL), ('a', 'misaligned', hip.EALIGN), ('b', b + 4, hip.EALIGN),
           ('b', b + 8, hip.EALIGN), ('n_components', 0, hip.EINVAL), ('n_components', 1, hip.EINVAL), ('n_components', -3, hip.EINVAL),
           ('n_components', 7, hip.EINVAL), ('n_components', 9, hip.EINVAL),                      # d != T m + 2
           ('a_scalar', 16.0, hip.EINVAL),                                                # fixed scales: d != T m
           ('a_scalar', 3.0, hip.EINVAL), ('a_scalar', 7.0, hip.EINVAL), ('a_scalar', 23.0, hip.EINVAL),   # drift code 3
           ('a_scalar', 21.0, hip.EINVAL), ('a_scalar', 5.0, hip.EINVAL),                 # fitzhugh_nagumo at m = 3, m = 1
           ('a_scalar', 14.0, hip.EINVAL), ('a_scalar', 6.0, hip.EINVAL),                 # lorenz63 at m = 2, m = 1
           ('a_scalar', 28.0, hip.EINVAL), ('a_scalar', 32.0, hip.EINVAL),                # m = 4 and past the codes
           ('a_scalar', 20.5, hip.EINVAL), ('a_scalar', -1.0, hip.EINVAL), ('a_scalar', float('nan'), hip.EINVAL)]
    ok = [('a_scalar', 20.0), ('a_scalar', 22.0)]                                         # cubic / lorenz63 at m = 3, unknown
    H.bad_descriptors_are_refused(dev, p.pot, p.x0, _flow_pair(d)[0], bad, ok)


# ------------------------------------------------------------------------- 8. determinism and sharding, overflow
@pytest.mark.parametrize('kind,shape', [('mala', (23, 'lorenz63', 3, True)), ('hmc', (20, 'fitzhugh_nagumo', 2, False))],
                         ids=lambda v: v if isinstance(v, str) else _id(v))
def test_determinism_and_sharding(dev, kind, shape):
    d, model, m, unknown = shape
    T = 8
    p = _Problem(d, model, m, unknown, 44, 300, 44)
    H.determinism_and_sharding(lambda: _sampler(kind, d, p.pot, T, _step(kind, p)), p.x0, T, d, seed=7, world=2)


@pytest.mark.parametrize('kind', ['mala', 'mh', 'hmc'])
def test_overflowing_scales_are_rejected_and_counted(dev, kind):
    """Unknown scales, every chain started at p = log sigma = -50: e^(-2p) overflows fp32, so U of the state and of every
    proposal near it is inf or NaN and no log ratio is finite.  The adjusted kernels reject every such proposal and count
    it as non-finite; the kept states stay finite (they are the starts)."""
    d, n, T = 26, 512, 6
    p = _Problem(d, 'cubic', 3, True, 3, n, 3)
    x0 = p.x0.clone()
    x0[:, d - 2] = -50.0
    s = _sampler(kind, d, p.pot, T, {'mala': 1e-6, 'mh': 0.0, 'hmc': 1e-6}[kind], L=3,
                 imd=torch.full((d,), 1e-6, dtype=torch.float64))
    s.seed = 5
    out = s.sample(x0, show_progress=False)
    st = out.statistics
    assert st.n_attempted_trajectories == n * T
    assert torch.isfinite(out.samples).all()
    print(kind, 'non-finite', st.n_nonfinite_log_ratios, 'accepted', st.n_accepted_trajectories)
    assert st.n_nonfinite_log_ratios == n * T and st.n_accepted_trajectories == 0
    assert torch.equal(out.samples.reshape(T, n, d)[-1], x0)


# ------------------------------------------------------------------------- 9. the Gaussian counterpart
@pytest.mark.parametrize('kind,model,m', [('mala', 'ou', 2), ('hmc', 'brownian', 1)])
def test_bridge_and_gaussian_forms_follow_the_same_oracle(dev, monkeypatch, kind, model, m):
    """A linear drift with fixed scales and its gaussian() counterpart (kind 4, the d x d precision streamed through LDS)
    under the same replayed noise: each matches the oracle, and their kept states agree to the state tolerance."""
    from nfmc_amd import hip
    d, T = 12 * m, 4
    p = _Problem(d, model, m, False, 10 * d + 1, 96, d + 2)
    dense = p.pot.gaussian()
    assert dense.descriptor(dev).kind == hip.POT_GAUSSIAN_FULL and p.pot.descriptor(dev).kind == hip.POT_DIFFUSION_BRIDGE
    h = _step(kind, p)
    got, keep = [], []
    for pot in (p.pot, dense):
        out, tr, _rec, spy = H.replay_run(monkeypatch, _sampler(kind, d, pot, T, h),
                                          lambda noise: _oracle(kind, p.x0, p.target, T, h, noise), p.x0, d, False)
        assert not spy.calls
        got.append(out.samples.reshape(T, p.x0.shape[0], d))
        keep.append(_compare_for(p)(got[-1], tr, '%s %s' % (kind, type(pot).__name__)))
    both = keep[0] & keep[1]
    torch.testing.assert_close(got[0][:, both], got[1][:, both], atol=ATOL, rtol=RTOL)


# ------------------------------------------------------------------------- 10. known answers, long fused runs
N_LONG, T_LONG, L_LONG, THIN = 4096, 2000, 8, 8


def _long_run(monkeypatch, pot, x0, T, L, h, seed, fuse='auto'):
    """T HMC transitions from the starts x0 (n, d), every THIN-th state stored: (the stored states of the second half
    (K, n, d) fp64, acceptance).  fuse='auto': the object on the fused kernels, no split-path transition; 'never': the same
    object behind a plain lambda, every transition on the autograd split path."""
    n = x0.shape[0]
    target = pot if fuse == 'auto' else (lambda x: pot(x))
    s = _sampler('hmc', pot.event_shape, target, T, h, L=L)
    s.params.thinning = THIN
    s.seed, s.fuse = seed, fuse
    spy = _Spy(monkeypatch)
    out = s.sample(x0.float().reshape((n,) + pot.event_shape), show_progress=False)
    assert len(spy.calls) == (0 if fuse == 'auto' else T)
    acc = out.statistics.n_accepted_trajectories / (n * T)
    kept = out.samples.reshape(-1, n, pot.dim)
    assert kept.shape[0] == T // THIN
    return kept[kept.shape[0] // 2:].double(), acc


def _start_correlation(per_chain, x0):
    """per coordinate, the correlation across the chains between a per-chain average and the chain's start"""
    a, b = per_chain - per_chain.mean(0), x0.double() - x0.double().mean(0)
    return (a * b).sum(0) / (a.norm(dim=0) * b.norm(dim=0))


def test_the_prior_alone_has_the_variances_of_a_random_walk(dev, monkeypatch):
    """Nothing observed and zero drift: the target is the Gaussian random walk itself, Var X_{t,c} = s0^2 + t sigma^2 dt.
    m = 2, T = 12 (d = 24), 4096 chains started from exact draws (prior_draws), 2000 fused HMC transitions (L = 8), the
    first half discarded, every 8th state kept.  The mean over the chains of each chain's time average of (X - mu0)^2
    against the exact variance, within 5 standard errors taken from the spread across the chains."""
    from nfmc_amd.potentials import DiffusionBridge
    T, m, s0, sig, dt, mu0 = 12, 2, 0.5, 0.4, 0.5, 0.3
    pot = DiffusionBridge(torch.full((T, m), float('nan')), drift='cubic', drift_params=(0.0, 0.0), dt=dt,
                          innovation_scale=sig, observation_scale=1.0, initial_mean=mu0, initial_scale=s0)
    assert pot.n_observed == 0
    x0 = pot.prior_draws(N_LONG, 3)
    lam = max(1.0 / s0 ** 2, 2.0 / (sig * sig * dt))             # the Hessian's diagonal, constant here
    kept, acc = _long_run(monkeypatch, pot, x0, T_LONG, L_LONG, (T * m) ** (-1 / 4) / math.sqrt(lam), 2718)
    per_chain = ((kept - mu0) ** 2).mean(0)
    est, se = per_chain.mean(0), per_chain.std(0) / math.sqrt(N_LONG)
    want = (s0 ** 2 + torch.arange(T, dtype=torch.float64) * sig * sig * dt).repeat_interleave(m)
    z = (est - want) / se
    print('acceptance %.3f, worst |z| %.2f' % (acc, float(z.abs().max())))
    assert 0.5 < acc <= 1.0, acc
    assert bool((z.abs() < 5).all()), z.tolist()


def test_the_lorenz_bridge_has_the_posterior_means_of_the_split_path(dev, monkeypatch):
    """The Lorenz preset at T = 10 (d = 30) with initial_scale = observation_scale = 0.2: the same HMC run (4096 chains from
    prior_draws, 2000 transitions, L = 8, step 1.2 / sqrt(4 om), every 8th state of the second half kept), once on the
    fused kernels and once on the autograd split path with another seed.  Every posterior mean agrees within 5 combined
    standard errors (from the per-chain time averages), and in both runs the per-chain averages have forgotten the
    starts (|correlation| under 0.3 in every coordinate), so the comparison is of two samples of the posterior and
    not of the shared prior draws with themselves.

    Why these scales and this step.  With the preset's own initial_scale = observation_scale = 1 the level of the whole
    path is held by the prior of X_0 alone: a collective direction of precision 1/10 beside fast ones of 4 om = 20000, and
    the fp64 oracle alone (256 of these starts) still has correlations with the starts of up to 0.94 after 500
    transitions at L = 24 and 0.70 at L = 32; no trajectory the split path can afford in a test forgets them.  With both
    scales at 0.2 the slowest direction is 25 times stiffer.  The fp64 oracle alone at this step and L (acceptance 0.65):
    the correlation across 256 chains between a chain's state and its start lies in -0.001 .. 0.244 at transition 500
    and in -0.013 .. 0.080 at transition 1000 (the sampling noise of 256 chains is 0.06), and that of the second half's
    per-chain mean in -0.083 .. 0.058: forgotten before the kept half begins.  The split run makes this the one slow
    test of the file, about 20 s: 16000 leapfrog steps through autograd, which the issue's case (4096 chains, a few
    thousand transitions, the split path) costs."""
    from nfmc_amd.potentials import DiffusionBridge
    pot = DiffusionBridge.lorenz_bridge(n_steps=10, seed=1, initial_scale=0.2, observation_scale=0.2)
    assert pot.dim == 30
    x0 = pot.prior_draws(N_LONG, 5)
    lam = 4.0 / (pot.innovation_scale ** 2 * pot.dt)
    h = 1.2 / math.sqrt(lam)
    means, ses = [], []
    for fuse, seed in (('auto', 2718), ('never', 314)):
        kept, acc = _long_run(monkeypatch, pot, x0, T_LONG, L_LONG, h, seed, fuse)
        per_chain = kept.mean(0)
        corr = _start_correlation(per_chain, x0)
        print('%s: acceptance %.3f, correlation with the starts %.3f .. %.3f' % (fuse, acc, float(corr.min()), float(corr.max())))
        assert 0.3 < acc <= 1.0, (fuse, acc)
        assert bool((corr.abs() < 0.3).all()), (fuse, corr.tolist())
        means.append(per_chain.mean(0))
        ses.append(per_chain.std(0) / math.sqrt(N_LONG))
    z = (means[0] - means[1]) / torch.sqrt(ses[0] ** 2 + ses[1] ** 2)
    print('worst |z| %.2f' % float(z.abs().max()))
    assert bool((z.abs() < 5).all()), z.tolist()
