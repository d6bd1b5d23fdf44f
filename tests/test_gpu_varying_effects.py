"""GPU: the varying-effects regression (NFMC_POT_VARYING_EFFECTS) on the fused HIP kernels against the fp64 CPU oracle,
with the target restated in fp64 over the raw observations (tests/varying_effects_fp64.py).

A problem is (model, C): 'both' = radon with varying intercepts and slopes (d = 2 C + 5), 'int' = varying intercepts and a
shared slope, 'slo' = a shared intercept and varying slopes (d = C + 4), 'es' = varying intercepts alone with known noise
(d = C + 2; C = 8 is eight schools itself, Rubin's data), optionally with known noise ('scalar' / 'vector') and
non-centered.  Data: VaryingEffectsRegression.synthetic(C, 2 C + 7, a seed per model and C).  Chains start at
varying_effects_fp64.start_states(seed = d + 1): the generating state (for eight schools: theta = y, mu = mean(y),
tau = std(y)) plus about one posterior standard deviation per coordinate.  The oracle samplers evaluate the model's log
densities from torch.distributions in fp64 over the observations (model_u64: independent of the kernels, the class and the
sufficient statistics).  The mass diagonals come from H = the median over the starts of the positive fp64 diagonal Hessian:
MALA inv_mass_diag = sqrt(H) with step min(0.5, 2.5 d^(-1/3)), HMC 1 / H with step min(0.4, 1.6 d^(-1/4)) and 5 leapfrog
steps (2 at d = 1023), MH 0.5 / sqrt(d H); ula and uhmc take a quarter of the mala and hmc steps (with no rejection the
oracle's own chains leave fp64 at C <= 4 otherwise: 1e300 within four transitions).  The caps are this posterior's: it is a funnel, and at d < 10 the
item-response tests' uncapped steps send a tenth to a quarter of the oracle's own HMC trajectories to a NaN energy.

Tolerances are the item-response tests' (tests/test_gpu_irt.py):
  states        atol 1e-3 + rtol 1e-4
  decisions     tie-aware: a chain whose fp64 |log u - log ratio| falls under MARGIN = 2e-3 at any of its transitions is
                excluded; the excluded share must stay under 10 %, all other chains must match.
The oracle ALONE, run on the CPU with these starts and steps over the whole grid of test 1 (mala, mh and hmc), excludes at
most 2.1 % of the chains (two of 96), under the 5 % the starts and steps were chosen for; its acceptance is 0.39 to 0.92
for mala, 0.70 to 0.81 for mh and 0.76 to 0.98 for hmc (1.0 at d = 1023, two leapfrog steps).  _compare prints the share of
every case.

Shapes: 'both' at C = 1, 2, 5, 6, 14, 30, 62, 126, 254, 509 is d = 7, 9, 15, 17, 33, 65, 129, 257, 513, 1023, the default
layouts (4, 2), (4, 4), (4, 4), (4, 8), (8, 8), (8, 16), (8, 32), (8, 64), (16, 64), (16, 64)
(tests/test_host_varying_effects.py asks the library); 2 C mod 4 is 2 for odd and 0 for even C, so the five globals start
mid-quad and on a quad boundary; with known noise d = 2 C + 4 = 16 and 32 fill their layouts with no padding.  'int' and
'slo' at C = 1, 2, 3, 4, 13, 61 put the four globals at every residue of C mod 4; 'es' at C = 1, 2 is layout (4, 1).

Flow-proposal cases (sections 3, 4 and 4b): from d = 25 on a flow centred by a Laplace fit (H.flow_inputs); the matrix
uses the non-centred parameterisation, because the Laplace fit of the centred one ends in the funnel's neck, where the
fp64 oracle alone accepts nothing.  The oracle alone accepts up to 0.326 of the jumps and up to 0.253 of the IMH proposals
of sections 3 and 4 (none at the small centred shapes, on a flow about the origin), and in the matrix 0.089 to 0.419 up to
capacity 128 and 0.281 to 0.391 above; under 1 % of the chains of a case are within MARGIN of a tie.  A proposal's log
scales can be far off (fp64 log ratios down to -73300, in the matrix -8090): every case sets skip_below_minus_50.
"""
import functools
import math

import pytest
import torch

import target_harness as H
from target_harness import Spy as _Spy, flow_pair as _flow_pair
from varying_effects_fp64 import VFX64, model_u64, start_states

pytestmark = pytest.mark.gpu

MARGIN = 2e-3
ATOL, RTOL = 1e-3, 1e-4

MODELS = {'both': ('varying', 'varying'), 'int': ('varying', 'shared'), 'slo': ('shared', 'varying'), 'es': ('varying', 'none')}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda', 0)


class _Problem:
    """potential, fp64 restatement, fp64 oracle target, starts x0 fp32 (n, d), H (d,) fp64"""

    def __init__(self, model, Cn, n, known=None, centered=True):
        from nfmc_amd.potentials import VaryingEffectsRegression
        ia, sl = MODELS[model]
        N = 2 * Cn + 7
        known = 'vector' if model == 'es' and known is None else known
        kw = dict(intercepts=ia, slopes=sl, centered=centered)
        if model == 'es' and Cn == 8:
            pot = VaryingEffectsRegression.eight_schools(centered=centered)
            y = pot.y
            theta, mu, tau = y, y.mean(), y.std()
            truth = pot.pack(a=theta if centered else (theta - mu) / tau, mu_a=mu, s_a=tau.log())
        else:
            if known == 'scalar':
                kw['noise_scale'] = 0.8
            elif known == 'vector':
                kw['noise_scale'] = 0.5 + torch.arange(N, dtype=torch.float64) / N
            seed = Cn + {'both': 1000, 'int': 2000, 'slo': 3000, 'es': 4000}[model] + (500 if known else 0) + (250 if not centered else 0)
            pot, truth = VaryingEffectsRegression.synthetic(Cn, N, seed, **kw)
        self.pot, self.truth, self.d = pot, truth, pot.event_size
        okw = dict(y=pot.y, group=pot.group, intercepts=ia, slopes=sl, noise_scale=pot.noise_scale, centered=centered,
                   location_scale=pot.location_scale, scale_scale=pot.scale_scale)
        self.ref = VFX64(x=pot.x, **okw)
        self.target = functools.partial(model_u64, xcov=pot.x, **okw)
        x0 = start_states(self.ref, truth, n, self.d + 1)
        self.x0 = x0.float()
        self.H = self.ref.hess_diag(x0).median(0).values
        self.name = '%s C=%d d=%d%s%s' % (model, Cn, self.d, ' known-' + known if known else '', '' if centered else ' non-centered')

    def imd(self, kind):
        if kind in ('mala', 'ula'):
            return torch.sqrt(self.H)
        if kind in ('hmc', 'uhmc'):
            return 1 / self.H
        return 0.5 / torch.sqrt(self.d * self.H)

    def step(self, kind):
        f = 0.25 if kind in ('ula', 'uhmc') else 1.0      # no rejection to stop a chain that runs down the funnel
        if kind in ('mala', 'ula'):
            return f * min(0.5, 2.5 * self.d ** (-1 / 3))
        return f * min(0.4, 1.6 * self.d ** (-1 / 4)) if kind in ('hmc', 'uhmc') else 0.0


@functools.lru_cache(maxsize=None)
def _problem(model, Cn, n, known=None, centered=True):
    return _Problem(model, Cn, n, known, centered)


_compare = functools.partial(H.compare_states, margin=MARGIN, atol=ATOL, rtol=RTOL)
# finite fp64 log ratios above -50 only: H.compare_decisions says why
_compare_decisions = functools.partial(H.compare_decisions, skip_below_minus_50=True)


def _sampler(kind, p, T, L=5, target=None, h=None, imd=None):
    """every kind with the problem's mass diagonal of that kind"""
    return H.mcmc_sampler(kind, p.d, p.pot if target is None else target, T, p.step(kind) if h is None else h, L,
                          p.imd(kind) if imd is None else imd, imd_kinds=H.KINDS)


def _oracle(kind, p, T, noise, L=5):
    return H.oracle_trace(kind, p.x0, p.target, T, p.step(kind), noise, L, p.imd(kind).float().double(), imd_kinds=H.KINDS,
                          label='%s %s' % (kind, p.name))


KINDS = ['mala', 'ula', 'mh', 'hmc', 'uhmc']
# (model, C, known noise, centered)
GRID = ([('both', c, None, True) for c in (1, 2, 5, 6, 14, 30, 62, 126, 254, 509)]
        + [(m, c, None, True) for m in ('int', 'slo') for c in (1, 2, 3, 4, 13, 61)]
        + [('es', 8, None, True), ('es', 1, None, True), ('es', 2, None, True)]
        + [('both', 5, None, False), ('both', 30, None, False), ('int', 13, None, False), ('slo', 4, None, False),
           ('es', 8, None, False)]
        + [('both', 6, 'vector', True), ('both', 14, 'scalar', False), ('int', 3, 'vector', True)])
IDS = ['%s-%d%s%s' % (m, c, '-' + k if k else '', '' if cen else '-nc') for m, c, k, cen in GRID]


def _against_oracle(check, monkeypatch, kind, p, T, L=5, **kw):
    check(monkeypatch, p, kind, T, _sampler(kind, p, T, L=L), lambda noise: _oracle(kind, p, T, noise, L=L), compare=_compare,
          decisions=_compare_decisions, **kw)


# ------------------------------------------------------------------------- 1. fused kernels vs fp64 oracle, replayed noise
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('model,Cn,known,centered', GRID, ids=IDS)
def test_mcmc_replay_matches_oracle(dev, monkeypatch, kind, model, Cn, known, centered):
    p = _problem(model, Cn, 96, known, centered)
    _against_oracle(H.replay_matches_oracle, monkeypatch, kind, p, 4, L=2 if p.d == 1023 else 5, torch_seed=p.d,
                    what='%s %s' % (kind, p.name))


# ------------------------------------------------------------------------- 2. native Philox streams
@pytest.mark.parametrize('kind,model,Cn,known,centered', [('mala', 'both', 30, None, True), ('ula', 'int', 3, None, True),
                                                           ('mh', 'both', 62, None, True), ('hmc', 'both', 5, None, False),
                                                           ('uhmc', 'es', 8, None, True), ('hmc', 'slo', 13, None, True),
                                                           ('mala', 'both', 6, 'vector', True)])
def test_mcmc_native_stream_matches_oracle(dev, monkeypatch, kind, model, Cn, known, centered):
    p = _problem(model, Cn, 96, known, centered)
    _against_oracle(H.native_matches_oracle, monkeypatch, kind, p, 4, seed=777 + p.d, what='native %s %s' % (kind, p.name))


# ------------------------------------------------------------------------- 3. jump_mala
SKIP = True     # skip_below_minus_50 of the flow-MH cases: a proposal's log scales can be far off: see the docstring


@pytest.mark.parametrize('fuse_tail', [False, True])
@pytest.mark.parametrize('model,Cn,centered', [('both', 5, True), ('int', 13, False), ('both', 14, True)])
def test_jump_mala_native_stream_matches_oracle(dev, monkeypatch, fuse_tail, model, Cn, centered):
    n, T = 192, 3
    p = _problem(model, Cn, n, None, centered)
    q, flows = H.flow_inputs(p, p.d, n, from_d=0, centre=H.local_fit(p, 0.3))     # see the docstring
    # under d = 25 the inner steps shrink with the proposal (0.3^2): the fp64 oracle alone otherwise has every jump below -59
    H.jump_mala_matches_oracle(monkeypatch, q, T=T, Kin=4, seed=31337, h=(0.09 if p.d < 25 else 1.0) * p.step('mala'),
                               imd=p.imd('mala').float(),
                               fuse_tail=fuse_tail, spline=False, atol=ATOL, rtol=RTOL, share=0.95,
                               jump_slack=max(2, int(0.03 * n * T)), margin=MARGIN, skip_below_minus_50=SKIP, flows=flows)


# ------------------------------------------------------------------------- 4. imh on the sequential flow-MH kernel
@pytest.mark.parametrize('model,Cn,centered,spline', [('es', 1, True, False), ('both', 6, True, False), ('both', 30, False, False),
                                                      ('int', 13, True, False), ('both', 5, True, True), ('slo', 13, True, True),
                                                      ('es', 8, False, True)])
def test_imh_runs_on_the_sequential_flow_mh_kernel(dev, monkeypatch, model, Cn, centered, spline):
    """Affine and spline ('c-rqnsf') instantiations of the register flow-MH kernel for kind 10."""
    p = _problem(model, Cn, 192, None, centered)
    q, flows = H.flow_inputs(p, p.d, 192, 3 if spline else 9, spline=spline, from_d=0, centre=H.local_fit(p, 0.3))
    H.imh_matches_oracle(monkeypatch, q, T=5, seed=4711 + p.d, flow_seed=3 if spline else 9, spline=spline, compare=_compare,
                         what='%s imh %s' % ('c-rqnsf' if spline else 'realnvp', p.name), margin=MARGIN, skip_below_minus_50=SKIP,
                         flows=flows)


# ------------------------------------------------------------------------- 4b. the flow-MH matrix
# capacity -> (model, groups): d = C + 2 ('es'), C + 4 ('int'), 2 C + 5 ('both').  The non-centred parameterisation: the
# Laplace fit of the centred one ends in the funnel's neck, where the fp64 oracle alone accepts nothing
FLOW_MODELS = {4: ('es', 1), 8: ('es', 5), 16: ('both', 4), 32: ('both', 10), 64: ('int', 46), 128: ('both', 48),
               256: ('int', 196), 512: ('both', 148)}
FLOW_DIMS = {4: 3, 8: 7, 16: 13, 32: 25, 64: 50, 128: 101, 256: 200, 512: 301}
FLOW_CASES = H.flow_cases(FLOW_DIMS)
FLOW_TESTS = ('test_jump_mala_native_stream_matches_oracle', 'test_imh_runs_on_the_sequential_flow_mh_kernel',
              'test_flow_mh_matrix')
# the 120 KB LDS bound: two affine coupling layers of width 8 at the ragged capacity 512 are 132 KB by themselves
FLOW_REFUSED = {'mh-cap512-d301-h8', 'jump_mala-cap512-d301-h8'}


@pytest.mark.parametrize('case', FLOW_CASES, ids=H.flow_case_id)
def test_flow_mh_matrix(dev, monkeypatch, case):
    """H.flow_cases: every flow-MH layout, sibling, width and coupling, the unadjusted carry path and the jump tails, with
    decisions and log ratios compared row by row (H.compare_flow_mh); the inner kernels with the problem's mass diagonals"""
    p = _problem(*FLOW_MODELS[case.cap], 96, None, False)
    H.run_flow_case(dev, monkeypatch, p, case, margin=MARGIN, compare=_compare, atol=ATOL, rtol=RTOL, h_mala=p.step('mala'),
                    h_hmc=p.step('hmc'), imd=lambda kind: p.imd(kind).float(), refused=H.flow_case_id(case) in FLOW_REFUSED,
                    skip_caps=tuple(FLOW_DIMS))


@pytest.mark.parametrize('cap', [64, 128, 256])
def test_flowb_override_launches_what_more_than_4096_chains_get(dev, monkeypatch, cap):
    """an unstaged kind (its data is read from global memory; nothing sits behind the flow image)"""
    p = _problem(*FLOW_MODELS[cap], 96, None, False)
    f, _of = H.centred_flow_pair(p, 5, 8, scale=0.1 if p.d < 200 else 0.05)
    H.flowb_override_equals_production(dev, monkeypatch, H.centred(p, 4160, 6), f, lpc=cap // 8, T=3, seed=99)


# ------------------------------------------------------------------------- 5. fused equals split
@pytest.mark.parametrize('kind,model,Cn,centered', [('mala', 'both', 30, True), ('hmc', 'both', 5, False), ('mh', 'int', 13, True),
                                                    ('hmc', 'slo', 61, True)])
def test_fused_equals_split(dev, monkeypatch, kind, model, Cn, centered):
    T = 4
    p = _problem(model, Cn, 96, None, centered)
    H.fused_equals_split(monkeypatch, p, lambda target: _sampler(kind, p, T, target=target), T, seed=2024, atol=ATOL, rtol=RTOL,
                         share=0.95)


# ------------------------------------------------------------------------- 6. NeuTra gradient (VALU kernels)
@pytest.mark.parametrize('model,Cn,known,centered,nh', [('es', 1, None, True, 4), ('both', 2, None, True, 8), ('both', 5, None, False, 16),
                                                        ('int', 13, None, True, 32), ('slo', 13, None, False, 8),
                                                        ('both', 30, None, True, 16), ('both', 6, 'vector', True, 4),
                                                        ('es', 8, None, True, 32)])
def test_neutra_gradient_matches_fp64_autograd(dev, model, Cn, known, centered, nh):
    """Against fp64 autograd through oracle/flow.py and the model over the observations, at the starts.  Tolerance:
    relative 2e-4 of (1 + max |.|) per row."""
    p = _problem(model, Cn, 96, known, centered)
    H.neutra_gradient_matches_autograd(dev, p.pot, p.ref, p.x0, nh, '%s H=%d' % (p.name, nh), flow_seed=3, bound=2e-4)


# ------------------------------------------------------------------------- 7. NeuTra trajectories, wide conditioner
@pytest.mark.parametrize('model,Cn,centered,nh', [('both', 5, True, 8), ('int', 13, False, 16), ('both', 30, True, 16)])
def test_neutra_hmc_fused_matches_oracle(dev, monkeypatch, model, Cn, centered, nh):
    p = _problem(model, Cn, 96, None, centered)
    H.neutra_hmc_fused_matches_oracle(monkeypatch, p, _flow_pair(p.d, 9, n_hidden=nh), T=3, L=4,
                                      h=0.2 / math.sqrt(float(p.H.max())), seed=12, atol=1e-3, share=0.93, accept_slack=6)


def test_neutra_wide_conditioner_takes_the_split_path_and_matches_the_oracle(dev):
    p = _problem('both', 14, 96)
    H.neutra_wide_takes_the_split_path(dev, p, _flow_pair(p.d, 9, n_hidden=64), T=3, L=4, h=0.2 / math.sqrt(float(p.H.max())),
                                       seed=12, atol=1e-3, share=0.93)


# ------------------------------------------------------------------------- 8. device warmup against the fp64 controller
@pytest.mark.parametrize('kind,model,Cn,centered,n,W,every', [('mala', 'both', 5, True, 140, 12, 1),
                                                              ('hmc', 'es', 8, False, 150, 16, 2),
                                                              ('mala', 'both', 30, True, 70, 8, 1)])
def test_warmup_controller_transitions_and_handoff(dev, monkeypatch, kind, model, Cn, centered, n, W, every):
    """As tests/test_gpu_warmup.py does for the other kinds: the controller state after the device warmup against
    oracle.samplers.replay_controller over the kernel's kept states and accept counts, every warmup transition and the
    sampling run after it shadowed in fp64.  The hmc case is eight schools, non-centered: dual averaging starts by
    doubling the step, and with an unknown noise scale and a unit mass diagonal (radon 'int', 'slo' and 'both' at C = 13,
    14) the fp64 oracle's OWN warmup then sends 18 to 35 % of the trajectories to a NaN energy (e^{-2 s_y} feeds back
    into s_y's momentum), which the shadow counts as near-ties; on eight schools it sends none."""
    p = _problem(model, Cn, n, None, centered)
    d, lm = p.d, float(p.H.max())
    h0 = 0.3 * (0.5 * d ** (-1 / 4) / math.sqrt(lm) if kind == 'hmc' else 0.5 * d ** (-1 / 3) / lm)
    H.warmup_matches_controller(monkeypatch, p, kind, W=W, T=6, L=4, every=every, h0=h0, imd0=torch.ones(d), seed=4242 + d,
                                what='vfx %s %s n=%d every=%d' % (kind, p.name, n, every), ties=0.05)


# ------------------------------------------------------------------------- 9. refused entry points, bad descriptors
def test_refusing_entry_points_answer_unsupported(dev):
    from nfmc_amd import hip
    p = _problem('both', 14, 256)
    pot = p.pot
    pd = pot.descriptor(dev)
    assert pd.kind == hip.POT_VARYING_EFFECTS == 10 and pd.n_components == 14
    assert pd.a_scalar == 10.0 and pd.b_scalar == float(pot.n_obs)                  # varying + 4 varying + 8, N
    assert pd.a % 16 == 0 and pot.descriptor(dev).a == pd.a and pot.descriptor(dev).b == pd.b   # cached per device
    H.refusing_entry_points(dev, pot, p.x0, functools.partial(_flow_pair, p.d))


def test_the_fit_step_refuses_kind_10(dev):
    p = _problem('both', 6, 96)
    H.fit_step_refuses(dev, p.pot, p.x0, _flow_pair(p.d)[0])


def test_philox7_and_bad_descriptors_are_refused(dev):
    """check_vfx's codes: a NULL a or b, C < 1, a layout code that is none of the 16 (no varying side, mode 3, slope-only,
    fractional, negative, 64, NaN), a C that does not give d, and N = 0, negative, inf or NaN with unknown noise are
    EINVAL; a misaligned a is EALIGN."""
    from nfmc_amd import hip
    p = _problem('both', 6, 128)
    d = p.d
    assert d == 17
    bad = [('a', 0), ('b', 0), ('n_components', 0), ('n_components', -1), ('n_components', 5), ('n_components', 7), ('n_components', d + 1),
           ('n_components', 2 ** 30),
           ('a_scalar', 5.0),      # shared + shared: no varying side
           ('a_scalar', 8.0),      # no intercept side
           ('a_scalar', 11.0),     # mode_a = 3
           ('a_scalar', 14.0),     # mode_b = 3
           ('a_scalar', 10.5), ('a_scalar', -1.0), ('a_scalar', 64.0 + 10.0), ('a_scalar', float('nan')),
           ('a_scalar', 2.0),      # a valid code of another d (C + 3 = 9)
           ('a_scalar', 26.0),     # known noise: d would be 16
           ('b_scalar', 0.0), ('b_scalar', -3.0), ('b_scalar', float('inf')), ('b_scalar', float('nan'))]
    H.bad_descriptors_are_refused(dev, p.pot, p.x0, _flow_pair(d)[0],
                                  [(f, v, hip.EINVAL) for f, v in bad] + [('a', 'misaligned', hip.EALIGN)],
                                  ok=[('a_scalar', 42.0)])                           # the same shape, non-centered: well formed


def test_limits_are_unchanged(dev):
    H.limits_are_unchanged()


# ------------------------------------------------------------------------- 11. determinism and sharding
@pytest.mark.parametrize('kind', ['mala', 'hmc'])
def test_determinism_and_sharding(dev, kind):
    T = 8
    p = _problem('both', 14, 300)
    H.determinism_and_sharding(lambda: _sampler(kind, p, T), p.x0, T, p.d, seed=7, world=2)


# ------------------------------------------------------------------------- 12. overflow
@pytest.mark.parametrize('kind', ['mala', 'mh', 'hmc'])
def test_overflowing_starts_are_rejected_and_counted(dev, kind):
    """Centered chains with s_a = -60: e^{-2 s_a} = e^{120} overflows fp32, U(x) is inf, every log ratio is inf - inf or
    worse.  The adjusted kernels reject every proposal and count it as non-finite (n_nonfinite_log_ratios), as for the
    existing kinds; the states stay where they are, finite."""
    n, T = 256, 5
    p = _problem('both', 5, n)
    x0 = p.x0.clone()
    x0[:, p.pot.group_block + p.pot.names.index('s_a')] = -60.0
    s = _sampler(kind, p, T, L=3, h=0.01, imd=torch.ones(p.d, dtype=torch.float64))
    s.seed = 5
    out = s.sample(x0, show_progress=False)
    st = out.statistics
    assert st.n_attempted_trajectories == n * T
    assert torch.isfinite(out.samples).all()
    assert torch.equal(out.samples.reshape(T, n, p.d)[-1], x0)
    assert st.n_accepted_trajectories == 0 and st.n_nonfinite_log_ratios == n * T


# ------------------------------------------------------------------------- 13. statistics through the public entry
SE_MULTIPLE = 6


def test_eight_schools_posterior_mean_fused_against_split(dev, monkeypatch):
    """sample(eight_schools(centered=False), strategy='jump_hmc') with 4096 chains, fused and on the split path
    (fuse='never', the object behind a plain lambda, same seed and starts): the posterior mean of mu over the final
    states.  Both runs draw the same Philox numbers, so their chains agree until a rounding difference flips a decision;
    from there two chains are, at worst, independent draws.  The difference of the two means is then bounded by that of
    two independent runs, whose standard error is sqrt(2) se with se = the split run's own between-chain standard error
    of mu, std / sqrt(4096).  SE_MULTIPLE = 6 of se is 4.2 of that standard error: a false alarm has probability about
    2e-5, and a kernel whose mu gradient or prior term were wrong would move the mean by a fraction of the posterior
    standard deviation = 64 se."""
    from nfmc_amd import sample
    from nfmc_amd.potentials import VaryingEffectsRegression
    from nfmc_amd.samplers import jump
    pot = VaryingEffectsRegression.eight_schools(centered=False)
    n, d = 4096, 10
    g = torch.Generator().manual_seed(8)
    x0 = torch.randn(n, d, generator=g)
    x0[:, 8] = 4.0 + 3.0 * x0[:, 8]
    x0[:, 9] = 1.0 + 0.5 * x0[:, 9]
    means, ses, splits = [], [], []
    for target, fuse in ((pot, 'auto'), (lambda x: pot(x), 'never')):
        spy = _Spy(monkeypatch)
        out = sample(target, event_shape=(d,), flow='realnvp', strategy='jump_hmc', n_iterations=8, n_chains=n, x0=x0,
                     show_progress=False, seed=17, fuse=fuse,
                     inner_kernel_kwargs={'step_size': 0.25, 'n_leapfrog_steps': 5}, inner_param_kwargs={'n_iterations': 5})
        splits.append(len(spy.calls))
        x = out.running_samples.last_sample.cpu().double().reshape(n, d)
        assert bool(torch.isfinite(x).all())
        mu = pot.unpack(x)['mu_a']
        means.append(float(mu.mean()))
        ses.append(float(mu.std() / math.sqrt(n)))
    assert splits[0] == 0 and splits[1] > 0                      # the first run fused, the second on the split path
    print('posterior mean of mu: fused %.4f, split %.4f, split se %.4f' % (means[0], means[1], ses[1]))
    assert abs(means[0] - means[1]) <= SE_MULTIPLE * ses[1], (means, ses)
    assert 0.0 < means[1] < 9.0                                  # the textbook posterior mean of mu is about 4.4
